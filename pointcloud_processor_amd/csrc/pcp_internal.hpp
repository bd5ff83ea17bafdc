// pcp_internal.hpp -- shared host/device declarations of libpcp (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "pcp_abi.h"
#include "pcp_fan_pick.hpp"
#include "pcp_knobs.hpp"

namespace pcp {
struct CopyPool;

// ---------------------------------------------------------------------------------------
// reference constants (virtual_lidar.cpp:100-114)
// ---------------------------------------------------------------------------------------
constexpr double kPi = 3.14159265358979323846;
constexpr double kMinDistance = 0.5;
constexpr double kRayStep = 0.3;
constexpr double kVisRadius = 0.08;
constexpr double kRayRadius = kVisRadius * 0.7;     // radiusSearch radius at :782
constexpr double kRelaxedRadius = kVisRadius * 3.0; // :743
constexpr double kMinElevation = -85.0 * kPi / 180.0;
constexpr double kMaxElevation = 85.0 * kPi / 180.0;
constexpr double kCellMargin = 4e-3;   // conservative margin of the stencil
constexpr double kQueryMargin = 1e-3;

// ---------------------------------------------------------------------------------------
// device buffer and pinned (page-locked) host staging buffer, both grow-only.  A buffer that must
// grow is reallocated with 25 % headroom (and at least 64 KiB): a hipFree synchronizes the whole
// device, so a per-frame chain whose sizes wander (C5) must converge to few reallocations instead
// of one per new maximum.  Every reallocation is counted process-wide (pcp_alloc_stats).  Small
// per-call H2D / D2H transfers from a pinned buffer skip the runtime's pageable staging copy.
// A buffer owns its memory: move-only, freed by its destructor; release() drops it mid-life.
// ---------------------------------------------------------------------------------------
void note_realloc(size_t bytes, bool pinned);
uint64_t alloc_count(int which);   // 0 device, 1 pinned reallocations, 2 bytes allocated

constexpr size_t kHeadroomMax = 16u << 20;   // first allocations below this get +25 %

template <bool Pinned>
struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~Buf() { release(); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        const bool grow = cap != 0;
        release();
        size_t want = std::max<size_t>(bytes, Pinned ? 4096 : 256);
        // message-sized buffers start with the headroom a growth would add: streamed clouds
        // vary by a few percent frame to frame, and each growth is a free + malloc in a frame
        if (grow || want < kHeadroomMax) want = std::max<size_t>(want + want / 4, 64u << 10);
        hipError_t e = Pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        note_realloc(want, Pinned);
        return e;
    }
    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};
using DevBuf = Buf<false>;
using PinnedBuf = Buf<true>;

// ---------------------------------------------------------------------------------------
// Uniform-grid spatial index (replaces pcl::KdTreeFLANN).  Points sorted by cell, cell
// start offsets (prefix sum, ncell+1 entries), and a dilated occupancy bitmask: bit of
// cell c = any point in the 2x2x2 block whose lower corner is c.  Cells are padded by one
// on every side so that a stencil whose lower corner falls outside [0, n-2] is provably
// empty.  See DESIGN.md "Terrain index".
// ---------------------------------------------------------------------------------------
struct GridView {               // POD passed to kernels by value
    const float4 *pts;          // x, y, z, bitcast(original index)
    const uint32_t *start;      // ncell + 1
    const uint32_t *occ2;       // dilated occupancy bits, (ncell + 31) / 32 words
    double ox, oy, oz;          // origin (lower corner of cell 0)
    double inv_c, c;
    double lo_x, lo_y, lo_z;    // origin + r_q + margin (stencil lower corner offset)
    int32_t nx, ny, nz;
    uint32_t n_pts;
    // tight bbox of the points, inflated by r_q + margin: samples outside are empty
    double bx0, bx1, by0, by1, bz0, bz1;
    // float copies for the stencil-corner and clip arithmetic: their rounding (~1e-5 m) stays
    // far inside the 1 mm query margin, so the skips remain exact (Terrain index)
    float flo_x, flo_y, flo_z, finv_c;
    float fnx1, fny1, fnz1;     // n - 1 per axis
    float fb[6];                // clip box x0, x1, y0, y1, z0, z1
    // z band of each stencil corner's 2x2x2 block (z-sorted indices only, else null): u16 =
    // lo | hi << 8, the block's lowest / highest point z as conservative steps of kZq cells
    // above the block's floor (lo 0 = unbounded below, hi 255 = unbounded above; lo > hi =
    // empty block).  fzoff = (r_q + m) / c (stencil-corner offset), fzt = (r_q + 2 mm) / c.
    const uint16_t *occz;
    float fzoff, fzt;
    // block-major copy (null unless built): the points of each stencil corner's 2x2x2 block in
    // one run, descending z -- bpts[bstart[lin] .. bstart[lin + 1]); one directory load and one
    // early exit per scan instead of 4 + 8
    const uint32_t *bstart;
    const float4 *bpts;
    // fine-window copy (null unless built, pcp_fine.hip): fine cells of c / F
    // in x, y (F = ffine); the window of fine cell W = the points within r + m (xy) of W's
    // rectangle, one run in descending z ended by a sentinel, wpts.  One record per (fine cell
    // x, y, coarse corner z), x-fastest, frx x fry x frz (frz = nz - 1): {walk start, probe
    // thresholds lo | hi << 8} for the window's points in coarse z cells iz, iz + 1 -- the
    // march's probe and the scan's directory in one load.  fus_off = fzoff / kZq: the probe's
    // sample height above the block floor in kZq steps is frac(fz) / kZq + fus_off.
    const uint2 *frec;
    const float4 *wpts;
    uint32_t frx, fry, frz;
    float fus_off, ffine;
    int32_t ftile;              // records in 4 x 4 xy tiles (1) or split (2), PCP_FINE_TILE
    // ftile 2: the record split in two arrays of 8 x 8 xy tiles -- the probe's 2-byte
    // thresholds (one 128-byte line per tile) and the 4-byte walk start, read by candidates only.
    // fband is the thresholds' tight twin (pcp_fan_band.hpp, DESIGN.md §5 Skip 7: the same
    // layout, never looser), or the specified array itself (PCP_FAN_BAND=0, or no twin built)
    const uint16_t *fband;
    const uint32_t *fstart;     // fskip 1: walk start (28 bits) | skip (4 bits, << 28): entries
                                // of the run at or above oz + (iz + 1.5) c, skipped by a
                                // candidate whose q lies more than r below that height; fskip 2:
                                // start (25 bits) | skips at iz + 1.375 (4 bits, << 25) and
                                // iz + 1.6875 (3 bits, << 29)
    int32_t fskip;
    float fzc, fzo;             // c and oz in float (the skip test)
    int32_t wpack;              // wpts entries packed to 12 bytes (x, y, z), PCP_FINE_PACK
    // ftile 2: an empty record's high byte is its clearance code (pcp_fan_clear.hpp, DESIGN.md
    // §5 Skip 5); fclear = 0 (PCP_FAN_CLEAR=0, or no split records) leaves the march as it was.
    // fclr_cf = c / F, fclr_rb = r + m + 1e-6 max|coord| (rounded up)
    int32_t fclear;
    float fclr_cf, fclr_rb;
    // ftile 2: the windows' pivots (pcp_fan_pivot.hpp, DESIGN.md §5 Skip 6), one 12-byte
    // (x, y, z) record per fine cell in fptx x fpty 8 x 8 xy tiles (the band records' tiles
    // without the iz term); null (PCP_FAN_PIVOT=0, or no split records) leaves the march as it
    // was.  Read by the fan kernels only.
    const float *fpiv;
    uint32_t fptx, fpty;
    // the clip interval's slack each side, in samples (pcp_fan_clip.hpp, DESIGN.md §5 Skip 3):
    // kClipSlack, or 1 (PCP_FAN_CLIP=0), the whole sample the rule kept before
    float fclip_e;
};
constexpr float kZq = 2.0f / 250.0f;   // z band step, cells (2 cells = 250 steps)

struct GridIndex {
    bool present = false;        // a tree exists (KdTreeFLANN::Ptr non-null)
    uint64_t n_pts = 0;
    double r_q = 0.0;            // stencil radius the cell edge was sized for
    double c = 0.0;
    int32_t nx = 0, ny = 0, nz = 0;
    double bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
    DevBuf pts, start, occ2, occz, bstart, bpts, frec, wpts, fpiv, fband2;
    bool occz_ok = false;
    bool blk_ok = false;         // block-major copy built (bstart / bpts)
    bool blk_fail = false;       // copy unavailable for this index (size cap or allocation
                                 // failure): the scans keep the per-cell runs, no retry
    bool fine_ok = false;        // fine-window copy built (frec / wpts)
    bool fine_fail = false;      // fine copy past its caps / not allocated: no retry
    uint32_t frx = 0, fry = 0, frz = 0;
    int32_t wpack = 0;           // wpts as 12-byte (x, y, z) entries
    float ffine = 0.0f;
    int32_t ftile = 0;
    int32_t fskip = 1;           // walk-start skip thresholds (PCP_FINE_SKIP)
    bool fpiv_ok = false;        // pivot table built (fpiv; with the split records)
    bool fband_ok = false;       // the thresholds' tight twin built (fband2; with the split records)
    size_t fstart_off = 0;       // ftile 2: byte offset of the start array inside frec
    uint64_t fnent = 0;          // entries of wpts, sentinels included (pcp_debug_fine_copy)
    bool occ2_ok = false;        // occ2 built (only indices queried by stencil_any need it)
    // k: the fan knobs of the view (fan_clear, fan_pivot, fan_band, fan_clip_e).  The terrain
    // index is viewed with the context's; every other index runs with the defaults
    GridView view(const Knobs &k = Knobs{}) const;
};

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
struct ProfSlot {
    double total_ms = 0.0;
    uint64_t launches = 0;
};

struct CloudBufs {                 // one cloud's filter-pipeline scratch
    DevBuf xyz, idx, keys[2], sparse, sparse_idx, hist, out;
    DevBuf skeys;                  // the fast chain: crop tiles' keys + digit-0 rows
};

template <class T>
constexpr bool kMoveOnly = !std::is_copy_constructible_v<T> && std::is_nothrow_move_constructible_v<T>;
static_assert(kMoveOnly<DevBuf> && kMoveOnly<PinnedBuf>, "a buffer has one owner");
static_assert(kMoveOnly<GridIndex> && kMoveOnly<CloudBufs>, "move-only through their buffers");

struct PendingEvent {
    int kid;
    hipEvent_t a, b;
};

// the context's two streams, as its base: destroyed after every member, i.e. after the last free
struct CtxStreams {
    hipStream_t stream = nullptr;
    hipStream_t area_stream = nullptr;   // the async area setup's side stream (knob.area_side)
    ~CtxStreams() {
        if (area_stream) (void)hipStreamDestroy(area_stream);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace pcp

// Nothing here is freed by hand: the buffers free themselves, ~pcp_ctx (pcp_context.hip) drains
// the streams and destroys what is no buffer, the streams go last (CtxStreams).
struct pcp_ctx : pcp::CtxStreams {
    ~pcp_ctx();
    int device = 0;
    pcp::Knobs knob;             // the environment's settings, read once by pcp_create
    std::string err;
    // virtual_lidar state
    pcp::GridIndex terrain;      // raycast index (r_q = 0.056)
    uint64_t terrain_cloud_n = 0;  // current terrain cloud size (stale-tree semantics)
    uint64_t terrain_index_n = 0;  // input count of the cloud the current terrain index was built
                                   // from (an empty pcp_set_terrain keeps index and count)
    pcp::GridIndex aux;          // zx120 cloud index (r_q = 0.24)
    uint64_t aux_cloud_n = 0;
    uint64_t n_cells = 0;
    pcp::DevBuf cells_xyz, cells_nrm;
    pcp::DevBuf cells_n_d;           // the lattice's cell count on the device (k_lattice_compact)
    // pcp_set_excavation_area_async: the setup enqueued and not waited for; area_finish (the
    // next call that needs the cells on the host, or the tick after its own synchronisation)
    // settles the count and regrows + reruns the neighbour lists on an overflow
    bool area_pending = false;
    uint64_t cells_cap = 0;          // the lattice's points: an upper bound of n_cells
    uint32_t area_npts = 0, area_grid_a = 0, area_grid_c = 0;
    uint64_t area_total = 0;
    pcp::PinnedBuf area_host;        // the setup's landing: [cells, area list use, cell list use,
                                     // overflow, pool cursors]
    // the async setup's normals + lattice on a stream of their own (knob.area_side): forked from
    // ctx->stream after the indices, joined by the scoring (score_enqueue) or by area_finish, so
    // the terrain / zx120 index builds in between overlap the neighbour lists
    bool area_forked = false;        // side work enqueued and not yet joined into ctx->stream
    hipEvent_t area_fork_ev = nullptr, area_join_ev = nullptr;
    pcp::DevBuf lat_flags;           // the lattice's per-point flags (k_lattice_flags)
    // pcp_filter_merge_nodes' outputs in tc_host (pcp_filter_merge_landed), until tc_host's
    // next writer
    bool fm_land_valid = false;
    int fm_land_k = 0;
    const void *fm_land_merged = nullptr;
    std::vector<const float *> fm_land_filtered;
    pcp::PinnedBuf exc_land;
    // pcp_excavate_area_async called with null outputs: its records left in exc_land
    // (pcp_excavate_landed), until the next pcp_excavate* call
    bool exc_keep_valid = false;
    const void *exc_keep_terr = nullptr, *exc_keep_area = nullptr;
    // the carve's four counters, two sets used in turn: each call's k_gen_emit clears the set
    // the next call uses (no memset launch in front of it)
    pcp::DevBuf carve_ctr;
    int carve_ctr_sel = 0;
    bool carve_ctr_clean[2] = {false, false};
    // excavation area (pcp_set_excavation_area): indices for the normal radius (1.5 m) and the
    // lattice test radius (1.5 * grid_resolution), and the per-point normals
    pcp::GridIndex exc_norm, exc_near;
    pcp::DevBuf area_nrm;
    uint64_t area_n = 0;
    // the normals in the reference's summation order (knob.normals_exact): sorted neighbour lists,
    // their per-query {base, count}, cursors + overflow word; list entries the last call needed
    pcp::DevBuf nb_list, nb_meta, nb_ctl, nb_pts;   // nb_pts: input points by index
    pcp::DevBuf nb_list_c, nb_meta_c;                // the cells' lists
    pcp::DevBuf nb_sel;                              // cells left to the ordered path
    uint64_t nb_need_c = 0;
    bool nb_ctl_zero = false;                // nb_ctl's cursors known zero (cleared by the last call)
    uint64_t nb_need = 0;
    uint64_t normals_regrown = 0;
    // excavated-terrain carve (pcp_excavate): index of the input cloud + scratch
    pcp::GridIndex carve;
    pcp::DevBuf carve_buf;
    // the index builds' per-cell counters: all zero between builds (the build's scan clears what
    // it counted), so no build zeroes them; cell_cnt_dirty marks a build that stopped between
    // its count and its scan (the next one clears the buffer first)
    pcp::DevBuf cell_cnt;
    bool cell_cnt_dirty = false;
    pcp::DevBuf cell_cnt2;           // the second grid's counters of build_index_pair
    bool cell_cnt2_dirty = false;
    // the generated lattice (surface + area records, their height queries) on the device:
    // [GenPoint surf | GenPoint area | queries (G generated + n input) | area records].  It
    // depends on the parameters and the excavation pose alone; while carve_key matches, the
    // next call neither regenerates nor uploads it
    pcp::DevBuf carve_gen;
    double carve_key[16] = {};
    bool carve_gen_ok = false;
    uint32_t carve_G = 0;
    uint64_t carve_nsurf = 0, carve_narea = 0;
    // scratch
    pcp::DevBuf stage, scratch[8];
    pcp::DevBuf fan_tab, poses_d, steps_d, out_a, out_b, out_c, out_d, stats_d;
    pcp::PinnedBuf fan_host;                 // pinned staging of poses in / counts out
    // pcp_place_sensors (pcp_place.hip): the rounds' state, base / owner, round totals and alive
    // mask, and the pinned landing of its one download (its own: the scoring's buffers stay as
    // pcp_score_poses leaves and expects them)
    pcp::DevBuf place_d;
    pcp::PinnedBuf place_host;
    // pcp_place_pair (pcp_pairs.hip): its state, base / owner, singles, per-block bests and the
    // dense pair table (pair_d), the clamped transposed rows M [C][P16] (pair_m), and the pinned
    // landing of its one download (its own, as the placement's)
    pcp::DevBuf pair_d, pair_m;
    pcp::PinnedBuf pair_host;
    // pcp_place_refine (pcp_refine.hip): its state, cell_score / cell_owner and the evaluations'
    // tables (refine_d), the clamped rows, the leave-one-out slot rows and the per-block bests
    // (refine_m), and the pinned landing of its one download (its own, as the pair's)
    pcp::DevBuf refine_d, refine_m;
    pcp::PinnedBuf refine_host;
    // pcp_place_triple (pcp_triples.hip): its state, cell_score / cell_owner, the per-first-sensor
    // bests, the blocks' bests and the dense triple table (triple_d), and the pinned landing of its
    // one download; its pair phase runs in pair_d / pair_m, which no call reads across calls
    pcp::DevBuf triple_d;
    pcp::PinnedBuf triple_host;
    // pcp_place_aimed (pcp_aim.hip): its state, base / owner, the rounds' [P][A] totals and covered
    // counts and the alive mask (aim_d), the predicate's tables (aim_m), and the pinned staging of
    // the tables' upload and landing of its one download (its own, as the placement's)
    pcp::DevBuf aim_d, aim_m;
    pcp::PinnedBuf aim_host;
    // pcp_simulate_scan (pcp_scan.hip): wave bases, offsets, records, dense images, point mask and
    // counts, and the pinned landing of its downloads (its own: the fan's buffers stay as
    // pcp_raycast_fan leaves and expects them)
    pcp::DevBuf vscan_d;
    pcp::PinnedBuf vscan_host;
    // pcp_place_coverage (pcp_cover.hip): its state, counts, round gains, alive mask, the need
    // words, the poses' bitsets, the owners and the staged ROI bytes, and the pinned landing of its
    // downloads (its own, as the scan's)
    pcp::DevBuf cover_d;
    pcp::PinnedBuf cover_host;
    // pcp_place_coverage_pair (pcp_cover_pair.hip): the same block with one row of gains (the
    // singles), then its result record, partners, the pairs' intersection counts and the dense
    // table, and the pinned landing of its downloads (its own: cover_d stays as
    // pcp_place_coverage leaves it)
    pcp::DevBuf cpair_d;
    pcp::PinnedBuf cpair_host;
    // pcp_place_coverage_refine (pcp_cover_refine.hip): the same block again, then its state with
    // the moves, the evaluation's sums, the class rows and the dense tables, and the pinned
    // landing of its downloads (its own: cover_d and cpair_d stay as their calls leave them)
    pcp::DevBuf crefine_d;
    pcp::PinnedBuf crefine_host;
    // pcp_place_coverage_aimed (pcp_cover_aim.hip): the same block again, then its aim record,
    // the [K][n][A] gains, the aim counts, the column and ring tables, the ranks and the points'
    // aim masks, and the pinned landing of its downloads (its own: the three above stay as their
    // calls leave them)
    pcp::DevBuf caim_d;
    pcp::PinnedBuf caim_host;
    // pcp_place_coverage_weighted (pcp_cover_weight.hip): its weighted counts in front of the same
    // block (the staged bytes are the weights), then the weight's bit planes, and the pinned
    // landing of its downloads (its own: the four above stay as their calls leave them)
    pcp::DevBuf cweight_d;
    pcp::PinnedBuf cweight_host;
    pcp::PinnedBuf res_host;                 // pinned landing of the filter chain's sizes
    pcp::PinnedBuf fm_res_host;              // pcp_filter_merge's result sizes, stored by its
                                             // kernels themselves (fixed: a graph holds it)
    pcp::PinnedBuf small_host;               // pinned landing of small size readbacks
    // pcp_raycast_fan_keys: the query's completion (a caller's stream waits on it) -- the next
    // query waits for it before it reuses the pinned pose staging
    hipEvent_t keys_ev = nullptr;
    bool keys_pending = false;
    // one process per GPU (pcp_comm_init_rank): this rank's RCCL communicator (an ncclComm_t),
    // the key vector its collective reduces and the pinned landing of the reduced vector
    void *comm = nullptr;
    int comm_nranks = 0, comm_rank = 0;
    pcp::DevBuf comm_keys;
    pcp::PinnedBuf comm_host;
    hipEvent_t comm_ev[2] = {};
    // pinned upload ring (upload_async): host bytes copied here, then a stream-ordered DMA
    static constexpr int kUpRing = 4;
    pcp::PinnedBuf up_buf[kUpRing];
    hipEvent_t up_ev[kUpRing] = {};
    bool up_used[kUpRing] = {};
    int up_next = 0;
    int pin_held = -1;                       // ring slot held by pin_stage until pin_release
    pcp::PinnedBuf tc_host;                  // transform_concat / carve: records stored by the
                                             // kernels straight into pinned memory
    pcp::PinnedBuf cand_host;                // generate_candidates: poses + count in one readback
    // exclusive_scan_u32's one-pass form (knob.scan_onepass): the tiles' status words
    // (value | epoch, flag) and the ticket that orders the tiles; epoch = the call's number
    pcp::DevBuf scan_state;
    uint32_t scan_epoch = 0, scan_ticket = 0;
    // host copies of message-sized buffers split over helper threads (pcp_hostcopy.hip,
    // knob.copy_threads)
    pcp::CopyPool *copy_pool = nullptr;
    pcp::PinnedBuf cv_host;                  // pcp_crop_voxel's fast chain: centroids + result
                                             // sizes stored by the kernels (one round trip)
    int32_t fan_naz = -1, fan_nel = -1;      // cached fan direction tables
    double fan_elmin = 0.0, fan_elmax = 0.0;
    std::vector<double> fan_el_h;            // the beam table they were built from (a mounted
                                             // query's el_table); empty: the uniform formula
    double steps_end = -1e300;               // cached step table
    int steps_K = 0;
    double steps_first = 0.0, steps_last = 0.0;   // its first and last entries (steps_K > 0)
    std::vector<double> fan_se_h;            // host copy of the cached table's sin(elevation)
    int num_cus = 256;                       // multiprocessors of the device
    pcp::DevBuf bk_stat;                     // the bucket chain's per-bucket words
    int terrain_queries = 0;                 // queries since the last pcp_set_terrain
    // filter/merge scratch
    pcp::DevBuf f_in, f_misc;
    std::vector<pcp::CloudBufs> fbuf;        // per-cloud scratch of the filter pipeline
    // captured filter_merge pipeline (device-resident inputs), replayed while its key matches
    hipGraph_t fm_graph = nullptr;
    hipGraphExec_t fm_exec = nullptr;
    std::vector<uint8_t> fm_key;
    bool capturing = false;
    // profiling
    bool prof = false;
    pcp::ProfSlot slots[PCP_K_COUNT];
    std::vector<pcp::PendingEvent> pending;
    std::vector<hipEvent_t> event_pool;
};

namespace pcp {

// error helpers --------------------------------------------------------------------------
int set_err(pcp_ctx *ctx, int code, const char *fmt, ...);
int hip_fail(pcp_ctx *ctx, hipError_t e, const char *what, const char *file, int line);

#define PCP_HIP(ctx, expr)                                                       \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) return ::pcp::hip_fail((ctx), _e, #expr, __FILE__, __LINE__); \
    } while (0)

#define PCP_CHECK_LAUNCH(ctx) PCP_HIP(ctx, hipGetLastError())

// profiling: bracket launches on ctx->stream
struct ProfScope {
    pcp_ctx *ctx;
    int kid;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(pcp_ctx *c, int k, hipStream_t s = nullptr);
    ~ProfScope();
};
void prof_resolve(pcp_ctx *ctx);   // after a stream sync
void prof_count(pcp_ctx *ctx, int kid);   // one event of kid (launches + 1, no time), always

// profiling of ONE kernel through the events hipExtLaunchKernelGGL records around its own
// execution: unlike stream-ordered events on an idle queue, the interval excludes the host's
// submission gap before the launch (pass .a / .b to the launch; null when not profiling)
struct KernelTimer {
    pcp_ctx *ctx;
    int kid;
    hipEvent_t a = nullptr, b = nullptr;
    KernelTimer(pcp_ctx *c, int k);
    ~KernelTimer();
};

// index ----------------------------------------------------------------------------------
// zsort: points of each cell in descending z (needed by scan_stencil's early exit: the
// terrain and aux indices); the other indices' queries are order-free
// occ: build the dilated occupancy bits (stencil_any: the aux index; the fan's A/B variant 2)
// raw_io (nullable): *raw_io non-null = the cloud's bytes already device-readable there (a
// previous build's, or a caller's staging); on return *raw_io = where the bytes were read.  A
// message-sized cloud is read in place from the pinned ring (pin_stage): without raw_io the
// slot is released behind the extraction; with raw_io the caller releases it (pin_release)
// after its own last reader.  Larger clouds are DMA'd into ctx->stage.  raw_copy (nullable,
// with raw_io: *raw_io then pinned, device-readable memory): the records are also copied there
// -- by the extraction itself where it can (16-byte multiples) -- and *raw_io = raw_copy on
// return, so the caller's later kernels read device memory (the composed carve)
int build_index(pcp_ctx *ctx, GridIndex &g, const pcp_cloud_view &v, double r_q,
                bool zsort = true, bool occ = true, const unsigned char **raw_io = nullptr,
                unsigned char *raw_copy = nullptr);
// two order-free indices (no z order, no occupancy bits) of one message-sized cloud from one
// pass over its raw records, plus the caller's per-point preparation (prep_pts: (x, y, z, 0) by
// input index; prep_nrm: NaN normals of the non-finite points; both nullable).  *paired false
// (nothing done): the cloud is empty, has no finite point or is past the host-bbox size -- build
// them with build_index.  raw_io as build_index's
int build_index_pair(pcp_ctx *ctx, GridIndex &ga, double ra, GridIndex &gb, double rb,
                     const pcp_cloud_view &v, const unsigned char **raw_io, float4 *prep_pts,
                     float *prep_nrm, bool *paired);
// the block-major copy of a z-sorted index (GridView.bstart / bpts); no-op when built
int build_blocks(pcp_ctx *ctx, GridIndex &g);
// the fine-window copy of a z-sorted index (GridView.frec / wpts); no-op when built.  Marks
// fine_fail (no retry) past its size caps or on an allocation failure.
int build_fine(pcp_ctx *ctx, GridIndex &g);
// before a terrain query: build the terrain's block copy per PCP_TERRAIN_BLOCKS (0 never,
// 1 at the second query after pcp_set_terrain -- a terrain that is queried once, as in the
// per-frame chain, does not pay for it --, 2 at the first)
int terrain_blocks_before_query(pcp_ctx *ctx);

// scan: exclusive prefix sum of n uint32 values into out (n + 1 entries, out[n] = total).
// tmp must hold scan_tmp_bytes(n).
size_t scan_tmp_bytes(uint64_t n);
// out2 (optional, may alias in): a second copy of out[0 .. n), e.g. a scatter's cursors; with
// zero2 it is cleared instead (out2 = in: counters left zero for their next use)
// preset16 (nullable): n halfwords set to 0x00FF by the same pass (the sparse z bands' preset)
int exclusive_scan_u32(pcp_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n, void *tmp,
                       uint32_t *out2 = nullptr, bool zero2 = false, uint16_t *preset16 = nullptr);
// two such scans (tmp sized for the larger); two one-tile ones are a single launch
int exclusive_scan_u32_pair(pcp_ctx *ctx, const uint32_t *in_a, uint32_t *out_a, uint64_t n_a,
                            uint32_t *out2_a, const uint32_t *in_b, uint32_t *out_b, uint64_t n_b,
                            uint32_t *out2_b, void *tmp, bool zero2);

// pcp_debug_math's element-wise probes, enqueued on ctx->stream by the source that owns the
// probed device functions: the double ops (pcp_score.hip) and the float libm / normal ops
// (pcp_excav.hip).  Device pointers, n > 0 and a known op are the caller's to ensure.
int debug_math_f64(pcp_ctx *ctx, int op, const double *a, const double *b, uint64_t n, void *out,
                   int32_t *aux);
int debug_math_f32(pcp_ctx *ctx, int op, const float *a, const float *b, uint64_t n, float *out);

// fan query up to the per-pose sums, enqueued on ctx->stream (pcp_fan.hip): device results
// in flight on return, the caller synchronizes.  n > 0.
struct FanEnq {
    // input (pcp_raycast_fan_allreduce): k_fan_reduce also writes the one-collective vector --
    // keys[keys_lo + p] = (blocked << 32) | (keys_lo + p), ~0 in the other slots [0, keys_P]
    // (the health word at keys_P included), the units behind it at keys[keys_P + 1 + p]
    unsigned long long *keys = nullptr;
    uint32_t keys_lo = 0, keys_P = 0;
    // outputs
    uint32_t *blocked_d = nullptr;
    unsigned long long *units_d = nullptr;
    int16_t *fh_d = nullptr;
    uint32_t rays = 0;
    size_t stats_bytes = 0;
    unsigned long long *stats_d = nullptr;
    // the march's per-wave partials {blocked, units} left on the device, pose-major, of the
    // live waves only (slot = p * live_waves + ray / 64 - wave0; the waves outside [wave0, wave0
    // + live_waves) of a pose's `waves` were culled: no ray of theirs is blocked), and the step
    // table's length (pcp_simulate_scan resolves from them)
    const uint2 *wave_part = nullptr;
    uint32_t waves = 0, wave0 = 0, live_waves = 0;
    int K = 0;
    // doubles per staged pose row, set by fan_enqueue: kFanRow (pcp_fan_row.hpp), or kFanDirRow
    // of a mounted query (pcp_fan_dir.hpp); the pinned results start behind the rows
    uint32_t pose_row = 0;
    bool mounted = false;
};
struct FanOpts {
    bool want_fh = false;         // first hits [n][rays] to o.fh_d
    // burst > 0: the production kernel `burst` times back-to-back between two events, the
    // average launch time to *burst_ms (pcp_raycast_fan_burst)
    int burst = 0;
    double *burst_ms = nullptr;
    // k_fan_reduce stores the per-pose {units u64[n], blocked u32[n]} straight into the pinned
    // landing block (ctx->fan_host past the staged poses) instead of device memory; o.*_d stay
    // null
    bool host_out = false;
    // the mounted query (pcp_raycast_fan_mounted): `poses5` holds poses6 rows (x, y, z, roll,
    // pitch, yaw), the rays are pcp_fan_dir.hpp's, the launch covers the full grid; el_table
    // (nullable, [n_el] radians, finite: the caller checked): the rings' elevations
    bool mounted = false;
    const double *el_table = nullptr;
};
// mode: the plain query, or a diagnostic launch -- Stats: the march's four counters summed to
// o.stats_d[0..3]; Stamps: four clock stamps per (pose, wave) at o.stats_d, o.stats_bytes long.
// Which kernel runs on which grid is fan_pick()'s answer (pcp_fan_pick.hpp).
int fan_enqueue(pcp_ctx *ctx, const double *poses5, uint64_t n, const pcp_fan_params *fan,
                FanEnq &o, FanMode mode = FanMode::Plain, const FanOpts &opt = FanOpts{});
// a mounted query's beam table (nullable): PCP_E_INVALID for a non-finite entry
int fan_el_table_check(pcp_ctx *ctx, const char *what, const pcp_fan_params *fan,
                       const double *el_table);

// runOptimization's scoring up to the per-pose sums, enqueued on ctx->stream (pcp_score.hip)
struct ScoreEnq {
    int P = 0, C = 0;
    double *comb = nullptr;        // [P][C] mobile scores
    double *score_z = nullptr;     // [C] zx120 scores
    uint8_t *mbits = nullptr;      // [P][C] result bits of the poses
    uint8_t *zbits = nullptr;      // [C] result bits of the zx120 evaluation
    uint8_t *flags_d = nullptr;    // [C] cell flag bytes (caller fills)
    double *tot_d = nullptr;       // [P + 1] totals, row P = zx120
    int32_t *cov_d = nullptr;      // [P + 1]
    int32_t *stats = nullptr;      // 64 colour-statistics slots (device: atomics)
    int32_t *stats_host = nullptr; // zc: where the last flag block copies the finished stats
    bool zc = false;               // flags / totals / covered live in the pinned block itself
    const uint32_t *P_dev = nullptr;   // the device's pose count (rows P = capacity)
    const uint32_t *C_dev = nullptr;   // the device's cell count (C = the lattice's capacity:
                                       // a pcp_set_excavation_area_async still in flight)
    const double *poses_k = nullptr;   // the poses / zx120 pose k_score_cells read
    const double *zx_k = nullptr;
    // the query's block (poses_d on the device, res_host pinned, same offsets): poses at 0,
    // cell flags at fl_off, totals + covered (tc_bytes) ending at most at st_off, stats at
    // st_off, blk_bytes in all
    size_t tc_bytes = 0, st_off = 0, fl_off = 0, blk_bytes = 0;
};
// cell_flags (C bytes) travel with the poses when given (pcp_score_poses); k_score_cells zeroes
// the statistics
// fuse_tail: the row sums are left to the caller's k_sum_flags launch (pcp_score_poses)
// zc: the kernels read the poses and flags from the pinned block and store the flags, totals,
// covered counts and (via the last flag block) the statistics back into it -- no copies (only
// with fuse_tail and cells present)
// P_dev / poses_dev: the poses are on the device already (generated in the same stream), n =
// the rows' capacity and *P_dev their count (pcp_generate_and_score)
int score_enqueue(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                  const pcp_vl_params *p, ScoreEnq &o, const uint8_t *cell_flags = nullptr,
                  bool fuse_tail = false, bool zc = false, const uint32_t *P_dev = nullptr,
                  const double *poses_dev = nullptr);
// key kernels of the pose-sharded search (pcp_score.hip, launch_fan_keys: pcp_fan.hip; used by
// pcp_multi.hip)
// identity: the value of the other ranks' slots (~0 for ncclUint64 MIN, INT64_MAX for a signed
// int64 MIN as torch.distributed reduces it)
void launch_fan_keys(hipStream_t st, const uint32_t *blocked_d, uint32_t lo, uint32_t cnt,
                     uint32_t P, unsigned long long *keys, unsigned long long identity = ~0ull);
// the covered key's mark of a pose some rank scored (k_score_keys; the low 32 bits: the count)
constexpr unsigned long long kScoreWritten = 1ull << 32;
void launch_score_keys(hipStream_t st, const ScoreEnq &o, int lo, int P, unsigned long long *v);
void launch_flags_from_keys(hipStream_t st, const unsigned long long *v, const uint8_t *zbits,
                            int C, int P, uint8_t *flags, int32_t *stats);
void launch_keys_combine(hipStream_t st, unsigned long long *a, const unsigned long long *b,
                         size_t n, bool is_max);
// pcp_score_poses_allreduce's landing: reduced keys, zx120 total, health, flags, stats -> pinned
void launch_score_land(hipStream_t st, const unsigned long long *v, int P, size_t hw,
                       const double *zx_total, const uint8_t *flags, int C, const int32_t *stats,
                       void *pin, size_t fl_off, size_t st_off);
// a device buffer into pinned host memory by a copy kernel (k_copy_pinned; a DMA when the copy
// kernel is off or the pointers are not 16-byte aligned)
int copy_to_pinned_async(pcp_ctx *ctx, void *dst_pinned, const void *src_d, size_t bytes,
                         hipStream_t st);
// the colour-statistics slots (k_cell_flags order) -> pcp_vl_report
void fill_report(const int32_t *st_h, double zx_total, int64_t best_idx, double best,
                 pcp_vl_report *rep);

// pcp_set_excavation_area_async's settlement (pcp_excav.hip): waits for the stream, regrows and
// reruns the neighbour lists on an overflow, sets ctx->n_cells; a no-op with nothing pending
// (stream_synced: the caller has just synchronised ctx->stream after the join)
int area_finish(pcp_ctx *ctx, bool stream_synced = false);
// after a stream synchronisation that followed the pending setup: did its lists overflow?  (the
// count in ctx->area_host is then valid, the cells' normals are not)
bool area_overflowed(const pcp_ctx *ctx);
// the async setup's side stream joined into ctx->stream (a stream wait, no host wait); a no-op
// when nothing is forked
void area_join(pcp_ctx *ctx);
// the area setup over records already device-readable (raw_pre: pcp_excavate_area_async's
// pinned landing; nullptr: staged from area->data as pcp_set_excavation_area does)
int area_setup_from(pcp_ctx *ctx, const pcp_cloud_view *area, double grid_resolution,
                    int32_t vertical_layers, double grid_bbox[6], uint64_t *n_cells, bool defer,
                    const unsigned char *raw_pre);
// pcp_set_terrain over records already device-readable (raw_pre), or staged (nullptr)
int set_terrain_from(pcp_ctx *ctx, const pcp_cloud_view *terrain, const unsigned char *raw_pre);

// the context's RCCL communicator and its events (pcp_comm.hip), by ~pcp_ctx
void comm_release(pcp_ctx *ctx);
// memcpy for host buffers, split over the context's helper threads from 256 KiB on
// (pcp_hostcopy.hip); host_copy_release stops the helpers (~pcp_ctx)
void host_copy(pcp_ctx *ctx, void *dst, const void *src, size_t bytes);
void host_copy_release(pcp_ctx *ctx);

// validate a cloud view
int check_view(pcp_ctx *ctx, const pcp_cloud_view *v, const char *what);

// a small (<= 4 KB) device -> host readback through pinned memory; synchronizes the stream
// (a pageable destination costs a staging copy per call)
int read_small(pcp_ctx *ctx, void *dst, const void *src_d, size_t bytes, hipStream_t st);

// host -> device copy of a caller's (pageable) buffer that does NOT wait for the stream: a
// pageable hipMemcpyAsync returns only once the stream has drained up to it (an implicit
// synchronisation in the middle of a chain).  Up to kUploadPinnedMax bytes are copied on the
// host into a slot of a pinned ring and DMA'd stream-ordered (the slot is reused only after
// its previous DMA completed); larger buffers take the pageable path.  The caller may reuse
// src_h on return either way.
constexpr size_t kUploadPinnedMax = 16u << 20;
int upload_async(pcp_ctx *ctx, void *dst_d, const void *src_h, size_t bytes, hipStream_t st);
// pinned host -> device by a copy kernel on st (no copy-engine hand-off); unaligned pointers
// take hipMemcpyAsync
int copy_pinned_async(pcp_ctx *ctx, void *dst_d, const void *src_pinned, size_t bytes,
                      hipStream_t st);
// several host pieces into one pinned slot at their byte offsets, then ONE DMA of `bytes`
// (the gaps between pieces are don't-care bytes on the device)
struct HostPiece {
    size_t off;
    const void *src;
    size_t bytes;
};
int upload_pieces(pcp_ctx *ctx, void *dst_d, const HostPiece *pc, int k, size_t bytes,
                  hipStream_t st);
// zero-copy staging of message-sized inputs (<= kPinDirectMax bytes): the pieces are copied on
// the host into a slot of the pinned ring and the kernels read them there, over the host link
// -- no DMA, so no copy-engine hand-off in front of the first kernel.  *dev = the slot (a
// device-readable host pointer).  The slot stays held until pin_release records, on st, the
// point after the last kernel that reads it (a call that stages twice without releasing
// drains the stream first).
constexpr size_t kPinDirectMax = 4u << 20;
int pin_stage(pcp_ctx *ctx, const HostPiece *pc, int k, size_t bytes, const void **dev);
void pin_release(pcp_ctx *ctx, hipStream_t st);

// the smallest float d with fl(d * d) >= r2: a point with dz = qz - pz >= d fails FLANN's
// float test (its sum is >= fl(dz^2) >= r2), and so does every lower point of a z-descending
// run -- the walks' early exit as one compare
float exit_dist(float r2);

// fan tables (shared definition with the oracle's orc_fan_tables)
void fan_tables(int32_t n_az, int32_t n_el, double el_min, double el_max, double *ca,
                double *sa, double *ce, double *se);
std::vector<double> step_table(double end);
// the context's device copy of step_table(end), cached by its end (the scoring and the fan share
// it): *K = its length.  A table past PCP_MAX_STEPS is refused, steps_within_bound alone says so
// before anything is launched
int steps_within_bound(pcp_ctx *ctx, double end);
int ensure_steps(pcp_ctx *ctx, double end, int *K);

// The timing entries: warm() once untimed (the phase's first touches), then body() reps times
// between two events on st; *ms = the time per repetition.
template <class Warm, class Body>
int time_reps(pcp_ctx *ctx, const char *what, hipStream_t st, int reps, Warm warm, Body body,
              double *ms) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PCP_HIP(ctx, hipEventCreate(&e0));
    PCP_HIP(ctx, hipEventCreate(&e1));
    int rc = warm();
    hipError_t e = rc ? hipSuccess : hipEventRecord(e0, st);
    for (int r = 0; r < reps && !rc && e == hipSuccess; ++r) rc = body();
    if (!rc && e == hipSuccess) e = hipEventRecord(e1, st);
    if (!rc && e == hipSuccess) e = hipEventSynchronize(e1);
    float t = 0.0f;
    if (!rc && e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(ctx, e, what, __FILE__, __LINE__);
    *ms = (double)t / reps;
    prof_resolve(ctx);
    return PCP_OK;
}

}  // namespace pcp
