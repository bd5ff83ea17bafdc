// pcp_pairs.hip -- the exact best pair of mobile sensors (pcp_place_pair): every pair a < b of
// the admissible poses gets t[a][b] = osum(max(max(base, S[a]), S[b])), the ordered sum of the
// positive combined scores over zx120, the fixed sensors and the two poses, and the first maximum
// wins (include/pcp_abi.h has the definition; DESIGN.md §6h the kernels and their timing).  The
// first-maximum reductions, the ordered total, the fold and the separation test are
// pcp_place_shared.hpp's; k_pair_tiles holds its walk_chunk's text in place.
//
// The scoring (k_score_cells) leaves comb [P][C] and score_z [C] on the device.  Three launches
// follow, ordered by the stream alone (no block ever waits for another):
//   k_pair_prep    base / owner, the admissible mask, the base total, and the clamped rows
//                  M[p][c] = x > 0 ? x : +0.0, x = max(base[c], S[p][c]), so that a pair's term
//                  is max(M[a][c], M[b][c]) (scores are never NaN: eval_cell ends in
//                  fmax(0.0, .)); rows padded to whole tiles and whole chunks with +0.0
//   k_pair_tiles   one block per tile pair of the upper triangle (pcp_pair_tiles.hpp)
//   k_pair_select  the first maxima, the answer's covered counts, cell_score / cell_owner
// The three kernels, their plan and pair_enqueue are in pcp_pair_phase.hpp (pcp_place_triple runs
// the same phase); this file holds the two entries.
#include <cmath>
#include <cstring>

#include "pcp_pair_phase.hpp"

using namespace pcp;

extern "C" int pcp_place_pair(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                              const pcp_vl_params *p, const pcp_pair_params *pp,
                              int64_t best_pair[2], double *pair_total, int32_t *pair_covered,
                              int64_t *best_single, double *single_total,
                              int32_t *single_covered, double *base_total, int32_t *base_covered,
                              double *pair_totals, double *single_totals, double *cell_score,
                              int32_t *cell_owner, int32_t *n_selected) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || !pp || !best_pair || !pair_total || !pair_covered || !best_single ||
        !single_total || !single_covered || !base_total || !base_covered || !n_selected ||
        (n && !poses5))
        return set_err(ctx, PCP_E_INVALID, "pcp_place_pair: null argument");
    PairFixed fx{};
    if (int rc = check_args(ctx, "pcp_place_pair", n, pp, fx)) return rc;
    // the scoring, no flags and no fused tail, as pcp_place_sensors runs it: comb [P][C], score_z
    // [C] and the row sums (row P: zx120) on the device; a step table past PCP_MAX_STEPS is
    // refused in there, before any launch
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o)) return rc;
    hipStream_t st = ctx->stream;
    const int C = o.C, P = o.P;
    auto nothing = [&] {
        best_pair[0] = best_pair[1] = -1;
        *pair_total = -INFINITY;
        *pair_covered = 0;
        *best_single = -1;
        *single_total = -INFINITY;
        *single_covered = 0;
        *n_selected = 0;
    };
    if (!C) {   // no cells: nothing to cover
        if (int rc = stream_done(ctx)) return rc;
        nothing();
        *base_total = 0.0;
        *base_covered = 0;
        return PCP_OK;
    }
    const PairPlan s = make_plan(C, P, pair_totals != nullptr);
    const bool cells_out = cell_score || cell_owner;
    const size_t down = s.dense ? s.bytes
                        : single_totals ? s.adm_off
                        : cells_out ? s.sg_off
                                    : s.cb.score_off;
    PCP_HIP(ctx, ctx->pair_d.ensure(s.bytes + 64));
    PCP_HIP(ctx, ctx->pair_m.ensure(s.m_bytes + 64));
    PCP_HIP(ctx, ctx->pair_host.ensure(down + 64));
    if (int rc = pair_enqueue(ctx, s, o, fx, sep2_of(pp->min_separation))) return rc;
    char *pin = ctx->pair_host.as<char>();
    PCP_HIP(ctx, hipMemcpyAsync(pin, ctx->pair_d.as<char>(), down, hipMemcpyDeviceToHost, st));
    if (int rc = stream_done(ctx)) return rc;
    const PairState *h = reinterpret_cast<const PairState *>(pin);
    nothing();
    best_pair[0] = h->pair[0];
    best_pair[1] = h->pair[1];
    if (h->pair[0] >= 0) {
        *pair_total = h->pair_total;
        *pair_covered = h->pair_cov;
    }
    *best_single = h->single;
    if (h->single >= 0) {
        *single_total = h->single_total;
        *single_covered = h->single_cov;
    }
    *base_total = h->base_total;
    *base_covered = h->base_cov;
    *n_selected = h->n_sel;
    if (pair_totals && P)
        host_copy(ctx, pair_totals, pin + s.tab_off, (size_t)P * P * sizeof(double));
    if (single_totals && P) std::memcpy(single_totals, pin + s.sg_off, (size_t)P * sizeof(double));
    copy_cells(pin, s.cb, C, cell_score, cell_owner);
    return PCP_OK;
}

extern "C" int pcp_place_pair_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                    const double zx[5], const pcp_vl_params *p,
                                    const pcp_pair_params *pp, int reps, double *ms_per_rep) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || !pp || !ms_per_rep || !poses5 || n == 0 || reps <= 0)
        return set_err(ctx, PCP_E_INVALID, "pcp_place_pair_burst: null argument or nothing to time");
    PairFixed fx{};
    if (int rc = check_args(ctx, "pcp_place_pair_burst", n, pp, fx)) return rc;
    *ms_per_rep = 0.0;
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o)) return rc;
    if (!o.C) {
        if (int rc = stream_done(ctx)) return rc;
        return set_err(ctx, PCP_E_INVALID, "pcp_place_pair_burst: no cells, nothing to time");
    }
    const PairPlan s = make_plan(o.C, o.P, false);
    PCP_HIP(ctx, ctx->pair_d.ensure(s.bytes + 64));
    PCP_HIP(ctx, ctx->pair_m.ensure(s.m_bytes + 64));
    const double sep2 = sep2_of(pp->min_separation);
    auto once = [&] { return pair_enqueue(ctx, s, o, fx, sep2); };
    return time_reps(ctx, "pcp_place_pair_burst", ctx->stream, reps, once, once, ms_per_rep);
}
