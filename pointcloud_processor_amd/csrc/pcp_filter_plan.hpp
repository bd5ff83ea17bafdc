// Which voxel chain a filter call runs, in which order it falls back, and the chains' sizes
// (DESIGN.md §6a).  Plain host C++ (no HIP dependency): pcp_filter.hip asks filter_plan() once per
// call and launches what it answers, and tests/native/filter_plan_selftest.cpp checks the rule
// and the geometries stand-alone.  The sizes below are shared with the kernels.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace pcp {

#ifndef PCP_CROP_TILE
#define PCP_CROP_TILE 4096
#endif
constexpr int kCropTile = PCP_CROP_TILE;   // points per crop tile (build knob)
constexpr int kST = 512;            // threads of the sort-tile kernels (8 waves)
#ifndef PCP_SORT_ITEMS
#define PCP_SORT_ITEMS 8
#endif
constexpr int kSortItems = PCP_SORT_ITEMS;   // keys per thread per sort tile
constexpr int kSortTile = kST * kSortItems;
constexpr int kGroup = 16;          // sort tiles per prefix group (radix digit prefix sums)
constexpr int kDigitBits = 9;       // radix digit: 512 bins, 3 passes for the C3 crop box
constexpr int kBins = 1 << kDigitBits;
constexpr int kMaxPasses = 4;       // ceil(32 / 9)
constexpr int kMaxClouds = 64;      // clouds (result slots) of a call
constexpr int kMaxGroupTiles = 32;  // crop tiles per pass-0 sort tile, at most
// up to kBatch clouds per launch, passed BY VALUE: pointers loaded from kernel arguments are
// known to be global (global_load, independent waits), which a table in memory would lose
constexpr int kBatch = 8;
#ifndef PCP_BK_BITS
#define PCP_BK_BITS 11
#endif
#ifndef PCP_BK_SUB
#define PCP_BK_SUB 12
#endif
constexpr int kBkBits = PCP_BK_BITS;      // target: ~2^kBkBits buckets per cloud
constexpr int kBkSubMax = PCP_BK_SUB;     // sub-key bits at most (LDS table of 2^kBkSubMax + 1)
constexpr int kBkMax = 4096;              // buckets per cloud at most
// bkv layout: [0, kBkChunkOff) per-bucket (voxels, item offset), then per-64-bucket voxel sums
constexpr uint32_t kBkChunkOff = kBatch * kBkMax;
constexpr int kBkGt = 15;                 // crop tiles per group at most
#ifndef PCP_BK_T3
#define PCP_BK_T3 512
#endif
constexpr int kBkT3 = PCP_BK_T3;          // k_bk_sort threads (build knob)
constexpr int kBkNg = kBkT3;              // groups per cloud at most (one per k_bk_sort thread)

struct Box {
    double x0, x1, y0, y1, z0, z1;
};

// ---- the crop box's voxel bound ---------------------------------------------------------------
// The voxel keys of points inside a finite box are below nv = prod(floor((hi - lo) / leaf) + 3).
struct VoxelBound {
    bool finite;   // every face finite
    double nv;     // (meaningful when finite)
};
inline VoxelBound voxel_bound(const Box &b, float leaf) {
    const double lo[3] = {b.x0, b.y0, b.z0}, hi[3] = {b.x1, b.y1, b.z1};
    VoxelBound v{true, 1.0};
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) v.finite = false;
        else v.nv *= std::floor((hi[a] - lo[a]) / (double)leaf) + 3.0;
    }
    return v;
}
// bits that hold every value below nv (32 at most)
inline int bits_for(double nv) {
    int bits = 0;
    while (bits < 32 && std::ldexp(1.0, bits) < nv) ++bits;
    return bits;
}
inline int passes_for(int bits) { return std::max(1, (bits + kDigitBits - 1) / kDigitBits); }
// radix passes needed for the voxel keys: from the crop box when it is finite, else all 32 bits
inline int radix_passes(const Box &b, float leaf) {
    const VoxelBound v = voxel_bound(b, leaf);
    return passes_for(v.finite ? bits_for(v.nv) : 32);
}
// The cloud certainly voxelises: a non-empty input and a finite crop box whose voxel keys fit 31
// bits (then PCL's int32 guard cannot fire on the cropped points' smaller bbox) -- a centroid or
// emit kernel can write the merged records itself, no kernel has to read the parameters back.
inline bool certainly_voxelises(const Box &b, float leaf, uint64_t n) {
    if (n == 0 || !(leaf > 0.0f)) return false;
    const VoxelBound v = voxel_bound(b, leaf);
    return v.finite && v.nv < 2147483647.0;
}

// ---- the chains' geometries (sizes only: the caller reserves the bytes and fills its job) -----
// n: the cloud's points; nb: its crop tiles; clouds: the clouds of the call (they share the CUs).

// The LSD fast chain's key geometry (box finite, leaf > 0, n > 0): box floor kb = floor(lo * inv)
// - 2 per axis (a margin for the float product p * inv of a point just inside the box), dims past
// floor(hi * inv) + 1 -- the bound of the keys the crop forms, not voxel_bound()'s; not ok when
// the keys or the float integers would not be exact (|values| >= 2^23, or DX * DY * DZ >= 2^31).
struct FastGeometry {
    bool ok;
    float kinv, kb[3];
    uint32_t kdx, kdxy;
    int passes;
    uint32_t gt, ng;       // crop tiles per group, groups
    size_t skeys_bytes;    // the keys in the crop tiles' slots, then [nb][kBins] digit-0 counts
};
inline FastGeometry fast_geometry(const Box &b, float leaf, uint64_t n, uint32_t nb, int clouds,
                                  int num_cus) {
    FastGeometry g{};
    if (n == 0 || !(leaf > 0.0f)) return g;
    const float inv = 1.0f / leaf;
    const double invd = (double)inv;
    const double lo[3] = {b.x0, b.y0, b.z0}, hi[3] = {b.x1, b.y1, b.z1};
    double dim[3];
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return g;
        const double f0 = std::floor(lo[a] * invd) - 2.0, f1 = std::floor(hi[a] * invd) + 2.0;
        if (std::fabs(f0) >= 8388608.0 || std::fabs(f1) >= 8388608.0 || !(f1 > f0)) return g;
        g.kb[a] = (float)f0;
        dim[a] = f1 - f0 + 1.0;
    }
    const double nv = dim[0] * dim[1] * dim[2];
    if (!(nv < 2147483647.0)) return g;
    g.kinv = inv;
    g.kdx = (uint32_t)dim[0];
    g.kdxy = (uint32_t)dim[0] * (uint32_t)dim[1];
    g.passes = passes_for(bits_for(nv));
    // groups: every group of every cloud in one round of one-block-per-CU blocks (the pass-0
    // scatter's LDS admits one per CU), at least 8 crop tiles each
    const uint32_t cus = (uint32_t)std::max(num_cus, 1);
    g.gt = std::min<uint32_t>(kMaxGroupTiles,
                              std::max<uint32_t>(8, (nb * (uint32_t)clouds + cus - 1) / cus));
    g.ng = (nb + g.gt - 1) / g.gt;
    g.skeys_bytes = (size_t)nb * kCropTile * 4 + (size_t)nb * kBins * 4 + 256;
    g.ok = true;
    return g;
}

// The bucket chain's sizes (the cloud certainly voxelises): groups of gt crop tiles (<= kBkNg per
// cloud), rows for the most buckets the cropped bbox can need.  bk_gt: PCP_BK_GT (0: one round
// of blocks); bk_pts: PCP_BK_PTS (0: buckets from the voxel count only).
struct BucketGeometry {
    bool ok;
    uint32_t gt, ng;       // crop tiles per group, groups
    int bkpb;              // bits(n / bk_pts): bs >= bits(nvox) - bkpb (64: unused)
    uint32_t nbkcap;       // buckets the rows and the look-back words are sized for
    size_t skeys_bytes;    // [ng][nbkcap + 1] rows
    size_t stat_bytes;     // the look-back words of a call's clouds
};
inline BucketGeometry bucket_geometry(const Box &b, float leaf, uint64_t n, uint32_t nb,
                                      int clouds, int num_cus, int bk_gt, int bk_pts) {
    BucketGeometry g{};
    if (!certainly_voxelises(b, leaf, n)) return g;
    const double nv = voxel_bound(b, leaf).nv;
    const uint32_t cus = (uint32_t)std::max(num_cus, 1);
    // one round of blocks for all groups of the call, at most kBkGt tiles (< 64 Ki points) each;
    // a frame that packs >= 8 tiles per group anyway takes 14: fewer, longer runs per bucket for
    // k_bk_sort to gather (C3: 314 -> 304 MB per frame, same time), still one round
    uint32_t gt = std::max<uint32_t>(1, (nb * (uint32_t)clouds + cus - 1) / cus);
    if (gt >= 8) gt = std::max<uint32_t>(gt, 14);
    if (bk_gt > 0) gt = (uint32_t)bk_gt;   // PCP_BK_GT (A/B)
    gt = std::min<uint32_t>(gt, kBkGt);
    const uint32_t ng = (nb + gt - 1) / gt;
    if (ng > (uint32_t)kBkNg) return g;
    // device: bs = clamp(max(bits(nvox) - kBkBits, bits(nvox) - bkpb), 0, kBkSubMax), nbk =
    // ceil(nvox / 2^bs) <= 2^min(kBkBits, bkpb), or ceil(nvox / 2^kBkSubMax) where bs is clamped
    int pb = 64;
    if (bk_pts > 0) pb = bits_for((double)std::max<uint64_t>(n / (uint64_t)bk_pts, 1));
    const double cap = std::max(std::ldexp(1.0, std::min(kBkBits, pb)),
                                std::ceil(nv / std::ldexp(1.0, kBkSubMax)));
    g.gt = gt;
    g.ng = ng;
    g.bkpb = pb;
    g.nbkcap = (uint32_t)std::min<double>(cap, (double)kBkMax);
    g.skeys_bytes = (size_t)ng * (g.nbkcap + 1) * 4 + 256;
    g.stat_bytes = ((size_t)kBkChunkOff + kBatch * kBkMax / 64) * 8;
    g.ok = true;
    return g;
}

// ---- the plan of one call --------------------------------------------------------------------
enum class FilterChain { General, Fast, Bucket };
enum class FilterEntry { CropBox, VoxelGrid, CropVoxel, FilterMerge, FilterMergeNodes };
// who writes the merged records: nobody (no merge, or the caller emits once the size is known to
// fit), the chain's last kernel (k_seg_centroid / k_bk_emit), or a separate k_emit_rgb
enum class FilterEmit { None, InChain, Separate };
// A geometry of one cloud.  AllocFailed is set by the caller after a failed reservation; it then
// asks for the plan again and goes on at the same attempt.
enum class Geo : uint8_t { Available, Unavailable, AllocFailed };

struct FilterPlanIn {
    FilterEntry entry;
    int fm_fast;            // PCP_FM_FAST as pcp_create normalised it: 0, 1 or 2
    bool fm_host_out;       // PCP_FM_HOST_OUT
    bool use_graphs;
    bool want_idx;          // pcp_crop_box: the kept indices are wanted
    bool idx_out;           // pcp_voxel_grid: voxel_idx or voxel_count is wanted
    bool dev_in, dev_out;   // pcp_filter_merge's PCP_MEM_DEVICE_* flags
    bool over_cap;          // the summed input sizes exceed cap (the output might not fit)
    int clouds;
    bool voxelises[kMaxClouds];   // certainly_voxelises(), per cloud
    Geo bucket[kMaxClouds], fast[kMaxClouds];
};

struct FilterAttempt {
    FilterChain chain;
    FilterEmit emit;
    bool sizes_pinned;       // the kernels store the result sizes into pinned memory
    bool centroids_pinned;   // ... and the cloud's centroids
};
// a[0] runs first; a[1] runs when a[0], a bucket chain, set its redo flag (no other chain does)
struct FilterPlan {
    int n;
    FilterAttempt a[2];
    bool graphable;          // the first attempt may be captured into a graph and replayed
};

inline FilterPlan filter_plan(const FilterPlanIn &in) {
    // Bucket / Fast and InChain need one launch batch of clouds that all certainly voxelise
    bool vox = in.clouds <= kBatch, bucket = true, fast = true;
    for (int i = 0; i < in.clouds; ++i) {
        vox = vox && in.voxelises[i];
        bucket = bucket && in.bucket[i] == Geo::Available;
        fast = fast && in.fast[i] == Geo::Available;
    }
    // the emit needs the sizes first when the output might not fit (device output only)
    const bool emit_now = !(in.dev_out && in.over_cap);
    bool sure = false;   // a chain that skips the parameter kernels may run
    FilterAttempt quick{}, general{};
    switch (in.entry) {
    case FilterEntry::CropBox:
    case FilterEntry::VoxelGrid:
    case FilterEntry::CropVoxel:
        // one host cloud, no merge: the centroids alone (no indices, no counts) through a quick
        // chain land in pinned memory with their sizes; an available geometry implies certainty
        sure = in.entry != FilterEntry::CropBox && !in.want_idx && !in.idx_out;
        quick = FilterAttempt{FilterChain::Fast, FilterEmit::None, true, true};
        general = FilterAttempt{FilterChain::General, FilterEmit::None, false, false};
        break;
    case FilterEntry::FilterMerge: {
        sure = emit_now && vox;
        // no kernel reads the sizes back when the chain emits: they go straight to pinned memory
        const bool pinned = sure && in.fm_host_out;
        quick = FilterAttempt{FilterChain::Fast, FilterEmit::InChain, pinned, false};
        general = FilterAttempt{FilterChain::General,
                                !emit_now ? FilterEmit::None
                                : vox     ? FilterEmit::InChain
                                          : FilterEmit::Separate,
                                pinned, false};
        break;
    }
    case FilterEntry::FilterMergeNodes:
        // only k_bk_emit writes a cloud's own centroids beside the merged records, so this entry
        // has no LSD fast attempt: what does not take the bucket chain, a redo included, runs
        // the general chain with a separate emit and copies the centroids down
        sure = vox;
        fast = false;
        quick = FilterAttempt{FilterChain::Bucket, FilterEmit::InChain, true, true};
        general = FilterAttempt{FilterChain::General, FilterEmit::Separate, false, false};
        break;
    }
    FilterPlan p{};
    if (sure && in.fm_fast == 2 && bucket) {
        p.a[p.n] = quick;
        p.a[p.n++].chain = FilterChain::Bucket;
    }
    if (sure && in.fm_fast >= 1 && fast) {
        p.a[p.n] = quick;
        p.a[p.n++].chain = FilterChain::Fast;
    } else {
        p.a[p.n++] = general;
    }
    p.graphable = in.entry == FilterEntry::FilterMerge && in.dev_in && in.dev_out && emit_now &&
                  in.use_graphs;
    return p;
}

}  // namespace pcp
