// Stand-alone check of pcp_filter_plan.hpp (no GPU, no HIP).
// 1. filter_plan() against the decision code it replaced.  old_*() restate, as plain if-chains,
//    the five places of pcp_filter.hip that decided which voxel chain runs: run_single's mode
//    loop, pcp_filter_merge's block (lsd_jobs, bucket, landed, graphable, the eager redo),
//    pcp_filter_merge_nodes' block (bucket, else the general chain with a separate emit),
//    enqueue_all's second decision from the jobs' bk / fast flags, and crop_voxel_impl's
//    J.fast || J.bk test of where the result lives.  The new side walks filter_plan()'s attempts
//    the way run_attempts does.  Per case the two must give the same sequence of (chain, emit
//    mode, sizes pinned, centroids pinned) and the same graph-capturable answer, over
//      entry {5} x fm_fast {0, 1, 2} x fm_host_out x use_graphs x clouds {1, 2, 8, 9, 64}
//      x dev_in x dev_out x upper > cap x want_idx x idx / count outputs wanted
//      x certainly voxelises {all, all but the first, all but the last cloud}
//      x bucket geometry, x fast geometry {available for all, unavailable / allocation failed for
//        the first / the last cloud} x redo flag
//    (pcp_crop_box, pcp_voxel_grid and pcp_crop_voxel take one cloud: their cases have one,
//    whatever the clouds value of the product).
//    An allocation failure is met by the walk when it applies the geometry (the plan is asked
//    again); the same fact handed to filter_plan() up front must give the same sequence.
// 2. voxel_bound / radix_passes / certainly_voxelises / fast_geometry / bucket_geometry against
//    a restatement of the replaced radix_passes, fast_geometry, bucket_geometry and
//    emit_in_centroid, over boxes that reach every early return (see boxes()).
// Build: c++ -std=c++17 -ffp-contract=off -I pointcloud_processor_amd/csrc
//        tests/native/filter_plan_selftest.cpp   (add -fsanitize=undefined for a sanitizer run)
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pcp_filter_plan.hpp"

using namespace pcp;

struct Att {
    FilterChain chain;
    FilterEmit emit;
    bool sizes_pinned, centroids_pinned;
    bool operator==(const Att &o) const {
        return chain == o.chain && emit == o.emit && sizes_pinned == o.sizes_pinned &&
               centroids_pinned == o.centroids_pinned;
    }
};
struct Trace {
    std::vector<Att> v;
    bool graphable = false;
    bool operator==(const Trace &o) const { return v == o.v && graphable == o.graphable; }
};

struct Case {
    FilterEntry entry;
    int fm_fast;
    bool fm_host_out, use_graphs;
    int k;
    bool dev_in, dev_out, over_cap, want_idx, idx_out;
    bool cv[kMaxClouds];      // certainly voxelises
    int bst[kMaxClouds];      // bucket geometry: 0 available, 1 unavailable, 2 allocation failed
    int fst[kMaxClouds];      // fast geometry, the same
    bool redo;                // a bucket chain sets its redo flag
};

// ---- the replaced code, restated ----------------------------------------------------------
// the jobs' flags as the callers set them (CloudJob::bk, ::fast)
struct Flags {
    bool bk[kMaxClouds], fast[kMaxClouds];
};
static Flags plain_flags() {
    Flags f;
    std::memset(&f, 0, sizeof f);
    return f;
}
static int old_batches(int k) { return (k + 8 - 1) / 8; }
// emit_in_centroid(bts): one batch, every cloud's per-cloud test (part 2 compares that test)
static bool old_emit_in_centroid(const Case &c) {
    if (old_batches(c.k) != 1) return false;
    for (int i = 0; i < c.k; ++i)
        if (!c.cv[i]) return false;
    return true;
}
// bucket_geometry / fast_geometry returned false for an unavailable geometry and for a failed
// allocation alike
static bool old_bucket_geometry(const Case &c, int i, Flags &f) {
    if (c.bst[i] != 0) return false;
    f.bk[i] = true;
    f.fast[i] = false;
    return true;
}
static bool old_fast_geometry(const Case &c, int i, Flags &f) {
    if (c.fst[i] != 0) return false;
    f.fast[i] = true;
    return true;
}
// enqueue_all: which enqueue_* ran, and who wrote the merged records
static void old_enqueue_all(const Case &c, const Flags &f, bool emit_out, FilterChain &chain,
                            FilterEmit &emit) {
    const int nb = old_batches(c.k);
    const int k0 = c.k < 8 ? c.k : 8;   // bts[0].k
    bool all_bucket = nb == 1 && k0 != 0;
    for (int i = 0; i < k0 && all_bucket; ++i)
        if (!f.bk[i]) all_bucket = false;
    if (all_bucket) {
        chain = FilterChain::Bucket;
        emit = emit_out ? FilterEmit::InChain : FilterEmit::None;
        return;
    }
    if (!emit_out && nb == 1) {
        bool fast = k0 > 0;
        for (int i = 0; i < k0; ++i) fast = fast && f.fast[i];
        if (fast) {
            chain = FilterChain::Fast;
            emit = FilterEmit::None;
            return;
        }
    }
    if (emit_out && old_emit_in_centroid(c)) {
        bool fast = true;
        for (int i = 0; i < k0; ++i) fast = fast && f.fast[i];
        chain = fast ? FilterChain::Fast : FilterChain::General;
        emit = FilterEmit::InChain;
        return;
    }
    chain = FilterChain::General;   // enqueue_chain per batch, then enqueue_emit per batch
    emit = emit_out ? FilterEmit::Separate : FilterEmit::None;
}

static Trace old_run_single(const Case &c, bool fast_ok) {
    Trace t;
    const Flags jobs = plain_flags();
    for (int mode = c.fm_fast; fast_ok && !c.want_idx && mode > 0; --mode) {
        Flags F = jobs;
        const bool geo = mode == 2 ? old_bucket_geometry(c, 0, F) : old_fast_geometry(c, 0, F);
        if (!geo) continue;
        Att a;
        old_enqueue_all(c, F, false, a.chain, a.emit);
        a.sizes_pinned = true;                       // read_results(ctx, res_h, 1, &ri, true, ...)
        a.centroids_pinned = F.fast[0] || F.bk[0];   // crop_voxel_impl: J.fast || J.bk
        t.v.push_back(a);
        if (mode == 2 && c.redo) continue;
        return t;
    }
    Att a;
    old_enqueue_all(c, jobs, false, a.chain, a.emit);
    a.sizes_pinned = false;
    a.centroids_pinned = jobs.fast[0] || jobs.bk[0];
    t.v.push_back(a);
    return t;
}

static Trace old_filter_merge(const Case &c) {
    Trace t;
    const bool emit_now = !(c.dev_out && c.over_cap);
    const Flags plain = plain_flags();
    Flags jobs = plain;
    auto lsd_jobs = [&]() {
        Flags fj = plain;
        bool all = true;
        for (int i = 0; i < c.k && all; ++i) all = old_fast_geometry(c, i, fj);
        return all ? fj : plain;
    };
    bool bucket = false;
    if (emit_now && c.fm_fast && old_emit_in_centroid(c)) {
        Flags fj = plain;
        bucket = c.fm_fast == 2;
        for (int i = 0; i < c.k && bucket; ++i) bucket = old_bucket_geometry(c, i, fj);
        jobs = bucket ? fj : lsd_jobs();
    }
    t.graphable = c.dev_in && c.dev_out && emit_now && c.use_graphs;
    const bool landed = emit_now && c.fm_host_out && old_emit_in_centroid(c);
    Att a;
    // (the captured launch passed obuf; graphable implies emit_now)
    old_enqueue_all(c, jobs, t.graphable ? true : emit_now, a.chain, a.emit);
    a.sizes_pinned = landed;
    a.centroids_pinned = false;   // the records go to the output buffer
    t.v.push_back(a);
    if (bucket && c.redo) {
        jobs = lsd_jobs();
        old_enqueue_all(c, jobs, true, a.chain, a.emit);
        t.v.push_back(a);
    }
    return t;
}

static Trace old_filter_merge_nodes(const Case &c) {
    Trace t;
    const Flags jobs = plain_flags();
    bool done = false;
    if (c.fm_fast == 2 && old_emit_in_centroid(c)) {
        Flags fj = jobs;
        bool bucket = true;
        for (int i = 0; i < c.k && bucket; ++i) bucket = old_bucket_geometry(c, i, fj);
        if (bucket) {
            Att a;
            old_enqueue_all(c, fj, true, a.chain, a.emit);
            a.sizes_pinned = true;       // res_h
            a.centroids_pinned = true;   // keep16
            t.v.push_back(a);
            done = !c.redo;
        }
    }
    if (!done)   // enqueue_chain per batch, enqueue_emit per batch, then the copies down
        t.v.push_back(Att{FilterChain::General, FilterEmit::Separate, false, false});
    return t;
}

static Trace old_trace(const Case &c) {
    switch (c.entry) {
    case FilterEntry::CropBox: return old_run_single(c, false);
    case FilterEntry::VoxelGrid:
    case FilterEntry::CropVoxel: return old_run_single(c, !c.idx_out);
    case FilterEntry::FilterMerge: return old_filter_merge(c);
    case FilterEntry::FilterMergeNodes: return old_filter_merge_nodes(c);
    }
    return Trace{};
}

// ---- the new rule, walked as run_attempts walks it -----------------------------------------
static FilterPlanIn facts(const Case &c, bool failures_known) {
    FilterPlanIn in{};
    in.entry = c.entry;
    in.fm_fast = c.fm_fast;
    in.fm_host_out = c.fm_host_out;
    in.use_graphs = c.use_graphs;
    in.want_idx = c.want_idx;
    in.idx_out = c.idx_out;
    in.dev_in = c.dev_in;
    in.dev_out = c.dev_out;
    in.over_cap = c.over_cap;
    in.clouds = c.k;
    auto geo = [&](int st) {
        return st == 1 ? Geo::Unavailable
                       : st == 2 && failures_known ? Geo::AllocFailed : Geo::Available;
    };
    for (int i = 0; i < c.k; ++i) {
        in.voxelises[i] = c.cv[i];
        in.bucket[i] = geo(c.bst[i]);
        in.fast[i] = geo(c.fst[i]);
    }
    return in;
}
static Trace new_trace(const Case &c, bool failures_known) {
    FilterPlanIn in = facts(c, failures_known);
    FilterPlan plan = filter_plan(in);
    Trace t;
    t.graphable = plan.graphable;
    for (int n = 0; n < plan.n; ++n) {
        const FilterAttempt &a = plan.a[n];
        bool ok = true;
        for (int i = 0; i < c.k && ok; ++i) {   // the appliers: the first failed allocation
            if (a.chain == FilterChain::Bucket && c.bst[i] == 2) {
                in.bucket[i] = Geo::AllocFailed;
                ok = false;
            } else if (a.chain == FilterChain::Fast && c.fst[i] == 2) {
                in.fast[i] = Geo::AllocFailed;
                ok = false;
            }
        }
        if (!ok) {
            plan = filter_plan(in);
            --n;
            continue;
        }
        t.v.push_back(Att{a.chain, a.emit, a.sizes_pinned, a.centroids_pinned});
        if (a.chain != FilterChain::Bucket || !c.redo) break;
    }
    return t;
}

static void print_trace(const char *who, const Trace &t) {
    std::printf("  %s: graphable %d", who, (int)t.graphable);
    for (const Att &a : t.v)
        std::printf(" (chain %d emit %d sizes %d centroids %d)", (int)a.chain, (int)a.emit,
                    (int)a.sizes_pinned, (int)a.centroids_pinned);
    std::printf("\n");
}

static long check_plan(long &mismatches) {
    const int ks[] = {1, 2, 8, 9, 64};
    long cases = 0;
    Case c;
    for (int entry = 0; entry < 5; ++entry)
    for (int fm = 0; fm < 3; ++fm)
    for (int bits = 0; bits < 256; ++bits)   // the eight yes / no inputs
    for (int k : ks)
    for (int cvp = 0; cvp < 3; ++cvp)
    for (int bp = 0; bp < 5; ++bp)
    for (int fp = 0; fp < 5; ++fp) {
        c.entry = (FilterEntry)entry;
        c.fm_fast = fm;
        c.fm_host_out = bits & 1;
        c.use_graphs = bits & 2;
        c.dev_in = bits & 4;
        c.dev_out = bits & 8;
        c.over_cap = bits & 16;
        c.want_idx = bits & 32;
        c.idx_out = bits & 64;
        c.redo = bits & 128;
        if (entry < 3) k = 1;   // (k is the loop's copy)
        c.k = k;
        for (int i = 0; i < k; ++i) {
            c.cv[i] = true;
            c.bst[i] = 0;
            c.fst[i] = 0;
        }
        if (cvp) c.cv[cvp == 1 ? 0 : k - 1] = false;
        if (bp) c.bst[bp % 2 ? 0 : k - 1] = bp <= 2 ? 1 : 2;
        if (fp) c.fst[fp % 2 ? 0 : k - 1] = fp <= 2 ? 1 : 2;
        ++cases;
        const Trace o = old_trace(c), n = new_trace(c, false), n2 = new_trace(c, true);
        if (o == n && o == n2) continue;
        if (++mismatches <= 10) {
            std::printf("MISMATCH entry %d fm_fast %d bits %d k %d cv %d bucket %d fast %d\n", entry,
                        fm, bits, k, cvp, bp, fp);
            print_trace("old", o);
            print_trace("new", n);
            print_trace("new, failures known", n2);
        }
    }
    return cases;
}

// ---- part 2: the bound and the geometries ---------------------------------------------------
static int old_radix_passes(const Box &b, float leaf) {
    const double lo[3] = {b.x0, b.y0, b.z0}, hi[3] = {b.x1, b.y1, b.z1};
    double nv = 1.0;
    int bits = 32;
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) finite = false;
        else nv *= std::floor((hi[a] - lo[a]) / (double)leaf) + 3.0;
    }
    if (finite) {
        bits = 0;
        while (bits < 32 && std::ldexp(1.0, bits) < nv) ++bits;
    }
    return std::max(1, (bits + kDigitBits - 1) / kDigitBits);
}
// make_job's J.passes
static int old_job_passes(const Box &b, float leaf, uint64_t n) {
    return (leaf > 0.0f && n > 0) ? old_radix_passes(b, leaf) : 0;
}
static bool old_fast(const Box &box, float leaf, uint64_t n, uint32_t nb, int clouds, int num_cus,
                     FastGeometry &g) {
    if (n == 0 || !(leaf > 0.0f)) return false;
    const float inv = 1.0f / leaf;
    const double invd = (double)inv;
    const double lo[3] = {box.x0, box.y0, box.z0}, hi[3] = {box.x1, box.y1, box.z1};
    double dim[3];
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return false;
        const double f0 = std::floor(lo[a] * invd) - 2.0, f1 = std::floor(hi[a] * invd) + 2.0;
        if (std::fabs(f0) >= 8388608.0 || std::fabs(f1) >= 8388608.0 || !(f1 > f0)) return false;
        g.kb[a] = (float)f0;
        dim[a] = f1 - f0 + 1.0;
    }
    const double nv = dim[0] * dim[1] * dim[2];
    if (!(nv < 2147483647.0)) return false;
    int bits = 0;
    while (bits < 31 && std::ldexp(1.0, bits) < nv) ++bits;
    g.skeys_bytes = (size_t)nb * kCropTile * 4 + (size_t)nb * kBins * 4 + 256;
    g.kinv = inv;
    g.kdx = (uint32_t)dim[0];
    g.kdxy = (uint32_t)dim[0] * (uint32_t)dim[1];
    g.passes = std::max(1, (bits + kDigitBits - 1) / kDigitBits);
    const uint32_t cus = (uint32_t)std::max(num_cus, 1);
    g.gt = std::min<uint32_t>(kMaxGroupTiles,
                              std::max<uint32_t>(8, (nb * (uint32_t)clouds + cus - 1) / cus));
    g.ng = (nb + g.gt - 1) / g.gt;
    return true;
}
static bool old_bucket(const Box &box, float leaf, uint64_t n, uint32_t nb, int clouds,
                       int num_cus, int bk_gt, int bk_pts, BucketGeometry &g) {
    if (n == 0 || !(leaf > 0.0f)) return false;
    const double lo[3] = {box.x0, box.y0, box.z0}, hi[3] = {box.x1, box.y1, box.z1};
    double nv = 1.0;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return false;
        nv *= std::floor((hi[a] - lo[a]) / (double)leaf) + 3.0;
    }
    if (!(nv < 2147483647.0)) return false;
    const uint32_t cus = (uint32_t)std::max(num_cus, 1);
    uint32_t gt = std::max<uint32_t>(1, (nb * (uint32_t)clouds + cus - 1) / cus);
    if (gt >= 8) gt = std::max<uint32_t>(gt, 14);
    if (bk_gt > 0) gt = (uint32_t)bk_gt;
    gt = std::min<uint32_t>(gt, kBkGt);
    const uint32_t ng = (nb + gt - 1) / gt;
    if (ng > (uint32_t)kBkNg) return false;
    int pb = 64;
    if (bk_pts > 0) {
        const uint64_t tgt = std::max<uint64_t>(n / (uint64_t)bk_pts, 1);
        pb = 0;
        while ((1ull << pb) < tgt) ++pb;
    }
    const double cap = std::max(std::ldexp(1.0, std::min(kBkBits, pb)),
                                std::ceil(nv / std::ldexp(1.0, kBkSubMax)));
    const uint32_t nbkcap = (uint32_t)std::min<double>(cap, (double)kBkMax);
    g.skeys_bytes = (size_t)ng * (nbkcap + 1) * 4 + 256;
    g.stat_bytes = ((size_t)kBkChunkOff + kBatch * kBkMax / 64) * 8;
    g.bkpb = pb;
    g.gt = gt;
    g.ng = ng;
    g.nbkcap = nbkcap;
    return true;
}
// emit_in_centroid's test of one cloud
static bool old_voxelises(const Box &b, float leaf, uint64_t n) {
    const int passes = old_job_passes(b, leaf, n);
    if (n == 0 || !(leaf > 0.0f) || passes <= 0 || passes * kDigitBits > 31 + kDigitBits - 1)
        return false;
    const double lo[3] = {b.x0, b.y0, b.z0}, hi[3] = {b.x1, b.y1, b.z1};
    double nv = 1.0;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return false;
        nv *= std::floor((hi[a] - lo[a]) / (double)leaf) + 3.0;
    }
    if (!(nv < 2147483647.0)) return false;
    return true;
}

struct LeafBox {
    Box b;
    float leaf;
};
static std::vector<LeafBox> boxes() {
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<LeafBox> v;
    const Box bench{0.0, 15.0, -10.0, 10.0, -1.5, 10.0};   // bench.py's C3 box and C1_BOX
    for (float leaf : {0.05f, 0.2f, 0.0f, -1.0f}) v.push_back({bench, leaf});
    v.push_back({Box{-inf, inf, -inf, inf, -inf, inf}, 0.2f});   // pcp_voxel_grid's box
    v.push_back({Box{0.0, inf, -10.0, 10.0, -1.5, 10.0}, 0.2f});
    v.push_back({Box{0.0, 15.0, -10.0, 10.0, nan, 10.0}, 0.2f});
    v.push_back({Box{15.0, 0.0, -10.0, 10.0, -1.5, 10.0}, 0.2f});    // inverted
    v.push_back({Box{15.0, -2.0, -10.0, 10.0, -1.5, 10.0}, 1.0f});   // inverted: f1 <= f0
    // leaf 1: voxel_bound = (s + 3)^3 crosses 2^31 between s = 1287 and 1288 in z; the fast
    // geometry's (s + 5)^3 between s = 1285 and 1286
    for (int s = 1283; s <= 1290; ++s) {
        v.push_back({Box{0.0, (double)s, 0.0, (double)s, 0.0, (double)s}, 1.0f});
        v.push_back({Box{0.0, 1287.0, 0.0, 1287.0, 0.0, (double)s}, 1.0f});
    }
    // |floor(lo / leaf) - 2| and |floor(hi / leaf) + 2| around 2^23
    for (int d = -3; d <= 3; ++d) {
        v.push_back({Box{-8388606.0 + d, -8388500.0, 0.0, 5.0, 0.0, 5.0}, 1.0f});
        v.push_back({Box{8388500.0, 8388606.0 + d, 0.0, 5.0, 0.0, 5.0}, 1.0f});
    }
    return v;
}

static long check_geometry(long &mismatches) {
    // n: empty, one point, a C1 scan, a C3 cloud, past kBkNg groups of kBkGt tiles, the most
    const uint64_t ns[] = {0, 1, 28800, 5000000, 40000000, 2147483647ull};
    long cases = 0;
    auto bad = [&](const char *what, const LeafBox &lb, uint64_t n) {
        if (++mismatches <= 10)
            std::printf("MISMATCH %s: box %g %g %g %g %g %g leaf %g n %llu\n", what, lb.b.x0,
                        lb.b.x1, lb.b.y0, lb.b.y1, lb.b.z0, lb.b.z1, (double)lb.leaf,
                        (unsigned long long)n);
    };
    int fast_ok = 0, bucket_ok = 0, fast_only = 0, bucket_only = 0;
    for (const LeafBox &lb : boxes())
        for (uint64_t n : ns) {
            const uint64_t ncap = n ? n : 1;
            const uint32_t nb = n ? (uint32_t)((ncap + kCropTile - 1) / kCropTile) : 0;   // J.nb
            ++cases;
            const int op = old_job_passes(lb.b, lb.leaf, n);
            const int np = (lb.leaf > 0.0f && n > 0) ? radix_passes(lb.b, lb.leaf) : 0;
            if (op != np) bad("radix_passes", lb, n);
            if (old_voxelises(lb.b, lb.leaf, n) != certainly_voxelises(lb.b, lb.leaf, n))
                bad("certainly_voxelises", lb, n);
            for (int clouds : {1, 2})
                for (int cus : {256, 1}) {
                    FastGeometry og{};
                    const bool ook = old_fast(lb.b, lb.leaf, n, nb, clouds, cus, og);
                    const FastGeometry g = fast_geometry(lb.b, lb.leaf, n, nb, clouds, cus);
                    ++cases;
                    fast_ok += g.ok;
                    if (ook != g.ok ||
                        (ook && !(og.kinv == g.kinv && og.kb[0] == g.kb[0] && og.kb[1] == g.kb[1] &&
                                  og.kb[2] == g.kb[2] && og.kdx == g.kdx && og.kdxy == g.kdxy &&
                                  og.passes == g.passes && og.gt == g.gt && og.ng == g.ng &&
                                  og.skeys_bytes == g.skeys_bytes)))
                        bad("fast_geometry", lb, n);
                    for (int bk_gt : {0, 1, 15, 40})
                        for (int bk_pts : {0, 64, 512}) {
                            BucketGeometry ob{};
                            const bool bok =
                                old_bucket(lb.b, lb.leaf, n, nb, clouds, cus, bk_gt, bk_pts, ob);
                            const BucketGeometry b =
                                bucket_geometry(lb.b, lb.leaf, n, nb, clouds, cus, bk_gt, bk_pts);
                            ++cases;
                            bucket_ok += b.ok;
                            fast_only += g.ok && !b.ok;
                            bucket_only += b.ok && !g.ok;
                            if (bok != b.ok ||
                                (bok && !(ob.gt == b.gt && ob.ng == b.ng && ob.bkpb == b.bkpb &&
                                          ob.nbkcap == b.nbkcap &&
                                          ob.skeys_bytes == b.skeys_bytes &&
                                          ob.stat_bytes == b.stat_bytes)))
                                bad("bucket_geometry", lb, n);
                        }
                }
        }
    // every kind of answer was reached
    if (!fast_ok || !bucket_ok || !fast_only || !bucket_only) {
        std::printf("MISMATCH coverage: fast %d bucket %d fast only %d bucket only %d\n", fast_ok,
                    bucket_ok, fast_only, bucket_only);
        ++mismatches;
    }
    // the benchmark's frames: C3 (two 5 M-point clouds, leaf 0.05) and C1 (leaf 0.2), 256 CUs
    const Box bench{0.0, 15.0, -10.0, 10.0, -1.5, 10.0};
    for (float leaf : {0.05f, 0.2f})
        for (int clouds : {1, 2}) {
            const uint64_t n = 5000000;
            const uint32_t nb = (uint32_t)((n + kCropTile - 1) / kCropTile);
            const FastGeometry g = fast_geometry(bench, leaf, n, nb, clouds, 256);
            const BucketGeometry b = bucket_geometry(bench, leaf, n, nb, clouds, 256, 0, 512);
            std::printf("bench leaf %g clouds %d: passes %d, fast ok %d passes %d gt %u ng %u, "
                        "bucket ok %d gt %u ng %u bkpb %d nbkcap %u\n",
                        (double)leaf, clouds, radix_passes(bench, leaf), (int)g.ok, g.passes, g.gt,
                        g.ng, (int)b.ok, b.gt, b.ng, b.bkpb, b.nbkcap);
            if (!g.ok || !b.ok || !certainly_voxelises(bench, leaf, n)) ++mismatches;
        }
    return cases;
}

int main() {
    static_assert(kBatch == 8 && kMaxClouds == 64, "old_batches() restates the batch size");
    long mismatches = 0;
    const long plan_cases = check_plan(mismatches);
    const long geo_cases = check_geometry(mismatches);
    std::printf("%ld plan cases, %ld geometry cases, %ld mismatches\n", plan_cases, geo_cases,
                mismatches);
    if (mismatches) return 1;
    std::printf("ok\n");
    return 0;
}
