// Which fan kernel a query launches, on which grid.  Plain host C++ (no HIP
// dependency): fan_enqueue asks fan_pick() once and launches what it answers through its kernel
// tables, and tests/native/fan_pick_selftest.cpp checks the rule stand-alone.
// The production launch is XCD-chunked with NPW poses per wave; the coarse layouts, odd fans,
// odd pose counts, long step tables and the diagnostic modes run the pose-interleaved kernels.
#pragma once

#include <cstdint>

namespace pcp {

constexpr int kStepLds = 256;   // step tables up to this long are read from LDS (fan, cells)
// the fan kernels' MODE template argument
enum class FanMode : int { Plain = 0, Stats = 1, Stamps = 2 };
enum class FanFamily : int {
    Coarse,      // k_raycast_fan over the coarse layouts, poses interleaved
    Fine,        // k_raycast_fan over the fine copy, poses interleaved
    Xcd,         // k_raycast_fan_xcd: the production launch
    PoseMajor,   // k_raycast_fan_pm, 128-thread blocks (PCP_FAN_BATCH=1)
    OccBit,      // k_raycast_fan with the occupancy-bit probe (PCP_FAN_BATCH=2)
};

struct FanPick {
    FanFamily family;
    FanMode mode;     // the kernel's MODE (the diagnostic modes run the interleaved kernels only)
    int FN;           // the kernel's record layout: 0 coarse, 1 / 4 / 8 fine with ftile 0 / 1 / 2
    bool UE;          // uniform rings: the wave's ring index is a scalar
    int NPW;          // poses per wave (Xcd; 1 elsewhere)
    bool full_grid;   // the launch covers every wave of every pose: no culled interval (Skip 4)
    int block;        // threads per workgroup
    bool mounted = false;   // the kernel's mounted form (pcp_fan_dir.hpp): Plain, full grid
};

// Poses per wave of the production launch: the largest of the request, ..., 2, 1 that divides
// the XCD pose chunk P / 8 (a request that is no instantiated width counts as 1).
// bench._fan_npw mirrors this rule; tests/test_fan_pick_host.py compares the two.
inline int fan_npw(int P, int request) {
    int npw = request >= 1 && request <= 32 && (request & (request - 1)) == 0 ? request : 1;
    while (npw > 1 && P % (8 * npw) != 0) npw >>= 1;
    return npw;
}

// fan_batch: PCP_FAN_BATCH (an unknown value is 0); fine / ftile: GridView.frec, .ftile; ue:
// FanArgs.uniform_el (n_az % 64 == 0); K: the step table's length; npw_request: PCP_FAN_NPW;
// burst: pcp_raycast_fan_burst, which times the production rule whatever the variant.
// mounted: pcp_raycast_fan_mounted / pcp_simulate_scan_mounted (Plain only): the production rule
// whatever the variant, always on the full grid -- a tilted ring has no one dz, so no ring
// liveness (Skip 4) holds for it.
inline FanPick fan_pick(FanMode mode, int fan_batch, bool fine, int ftile, bool ue, int P, int K,
                        int npw_request, bool burst, bool mounted = false) {
    const int FN = !fine ? 0 : ftile == 2 ? 8 : ftile != 0 ? 4 : 1;
    // the diagnostic modes write a slot per wave of the pose, and the pose-major grid is 2-D
    const bool full = mode != FanMode::Plain || fan_batch == 1 || mounted;
    const FanPick interleaved{fine ? FanFamily::Fine : FanFamily::Coarse, mode, FN, fine && ue, 1,
                              full, 64, mounted};
    if (mode != FanMode::Plain) return interleaved;
    if (!burst && !mounted) {
        if (fan_batch == 1) return FanPick{FanFamily::PoseMajor, mode, 0, false, 1, true, 128};
        if (fan_batch == 2) return FanPick{FanFamily::OccBit, mode, 0, false, 1, false, 64};
        if (fan_batch == 4) return interleaved;
    }
    // XCD-chunked placement (each XCD's L2 serves neighbouring poses' overlapping fans): 0.61 vs
    // 0.63 ms on C2; several poses per wave over the tiled fine copies only
    if (fine && ue && P % 8 == 0 && K <= kStepLds)
        return FanPick{FanFamily::Xcd, mode, FN, true, ftile != 0 ? fan_npw(P, npw_request) : 1,
                       full, 64, mounted};
    return interleaved;
}

// The launch's grid.  lw: the waves per pose it covers (all under full_grid, else the live
// interval); lw == 0: nothing to launch, {0, 0}.
struct FanGrid { uint32_t x, y; };
inline FanGrid fan_grid(uint32_t lw, uint32_t P, uint32_t rays, const FanPick &k) {
    if (lw == 0) return FanGrid{0u, 0u};
    if (k.family == FanFamily::PoseMajor) return FanGrid{(rays + 127u) / 128u, P};
    return FanGrid{lw * P / (uint32_t)k.NPW, 1u};   // (Xcd: NPW divides P / 8)
}

}  // namespace pcp
