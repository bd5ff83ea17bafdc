// Stand-alone check of pcp_fan_pick.hpp (no GPU, no HIP): fan_pick() and fan_grid() against the
// launch code they replaced.  old_launch() restates that code's if-chains arm by arm -- the
// culling block's full-grid condition, the stats / stamps / lw == 0 / burst / PCP_FAN_BATCH
// branches of fan_enqueue, the seven arms of its interleaved launch and the switch of its
// XCD launcher -- and names the kernel each arm launched with its grid and block.  The new
// rule's answer, formatted the same way, must be the same launch for every combination of
//   mode x fan_batch {0, 1, 2, 3, 4, 7} x layout {coarse (ftile 0, 1, 2), fine tile 0, 1, 2}
//   x uniform rings x P {1..72, 128, 256, 65535} x K {0, 1, 256, 257, 365}
//   x PCP_FAN_NPW {1, 2, 4, 8, 16, 32} x burst,
// each with a culled interval, the full interval and no live wave.
// Then it prints, for tests/test_fan_pick_host.py to compare with bench.py:
//   npw <P> <request> -> <poses per wave>     P = 1..256, every request above and two invalid
//   kernel <ftile> <P> <request> <name>       the production pick over a fine terrain
// Build: c++ -std=c++17 -I pointcloud_processor_amd/csrc tests/native/fan_pick_selftest.cpp
// (add -fsanitize=undefined for a sanitizer run of the host logic).
#include <cstdio>
#include <cstring>
#include <string>

#include "pcp_fan_pick.hpp"

using namespace pcp;

struct Launch {
    std::string kernel;   // demangled, every template argument written out; empty: no launch
    uint32_t gx = 0, gy = 0, block = 0;
    bool full_grid = false;
    bool operator==(const Launch &o) const {
        return kernel == o.kernel && gx == o.gx && gy == o.gy && block == o.block &&
               full_grid == o.full_grid;
    }
};

static std::string fmt(const char *f, int a = 0, int b = 0, int c = 0) {
    char buf[128];
    std::snprintf(buf, sizeof buf, f, a, b, c);
    return buf;
}
static const char *tf(bool b) { return b ? "true" : "false"; }

// ---- the replaced code, restated ----------------------------------------------------------
// template <int MODE, int BS = 64, bool ZB = true, int W = 7, int FN = 0, bool UE = false>
//   k_raycast_fan
// template <int MODE, int BS = 64, bool ZB = true, int W = 8, int FN = 1, bool UE = true,
//           int NPW = 1> k_raycast_fan_xcd
static std::string old_interleaved(int MODE, bool fine, bool tile, bool split, bool ue) {
    if (fine && split && ue) return fmt("k_raycast_fan<%d, 64, true, 8, 8, true>", MODE);
    else if (fine && split) return fmt("k_raycast_fan<%d, 64, true, 8, 8, false>", MODE);
    else if (fine && tile && ue) return fmt("k_raycast_fan<%d, 64, true, 8, 4, true>", MODE);
    else if (fine && tile) return fmt("k_raycast_fan<%d, 64, true, 8, 4, false>", MODE);
    else if (fine && ue) return fmt("k_raycast_fan<%d, 64, true, 8, 1, true>", MODE);
    else if (fine) return fmt("k_raycast_fan<%d, 64, true, 8, 1, false>", MODE);
    else return fmt("k_raycast_fan<%d, 64, true, 7, 0, false>", MODE);
}
static Launch old_xcd(int npw, int ftile, uint32_t lw, uint32_t P) {
    Launch L;
    L.gx = lw * P / (uint32_t)npw;
    L.gy = 1;
    L.block = 64;
    int N;
    switch (npw) {
    case 2: N = 2; break;
    case 4: N = 4; break;
    case 8: N = 8; break;
    case 16: N = 16; break;
    case 32: N = 32; break;
    default: N = 1; break;
    }
    if (ftile == 2) L.kernel = fmt("k_raycast_fan_xcd<0, 64, true, 8, 8, true, %d>", N);
    else L.kernel = fmt("k_raycast_fan_xcd<0, 64, true, 8, 4, true, %d>", N);
    return L;
}
// live_w: the live waves of the call's culled interval; waves: all of a pose's
static Launch old_launch(bool stats, bool stamps, int fan_batch, bool has_frec, int ftile,
                         bool uniform_el, int P, int K, int fan_npw, int burst, uint32_t live_w,
                         uint32_t waves, uint32_t rays) {
    uint32_t lw = waves;
    bool culled = false;
    if (!stats && !stamps && fan_batch != 1) {
        lw = live_w;
        culled = true;
    }
    const uint32_t grid1 = lw * (uint32_t)P;
    const bool fine = has_frec, ue = uniform_el, tile = ftile != 0;
    const bool split = ftile == 2;
    int npw = fan_npw;
    while (npw > 1 && P % (8 * npw) != 0) npw >>= 1;
    Launch L;
    auto interleaved = [&](int MODE) {
        L.kernel = old_interleaved(MODE, fine, tile, split, ue);
        L.gx = grid1;
        L.gy = 1;
        L.block = 64;
    };
    if (stats) {
        interleaved(1);
    } else if (stamps) {
        interleaved(2);
    } else if (lw == 0) {
        // no march
    } else if (burst > 0) {
        if (fine && tile && ue && P % (8 * npw) == 0 && K <= 256)
            L = old_xcd(npw, ftile, lw, (uint32_t)P);
        else if (fine && ue && P % 8 == 0 && K <= 256) {
            L.kernel = "k_raycast_fan_xcd<0, 64, true, 8, 1, true, 1>";
            L.gx = grid1;
            L.gy = 1;
            L.block = 64;
        } else
            interleaved(0);
    } else {
        switch (fan_batch) {
        case 1:
            L.kernel = "k_raycast_fan_pm<128, true>";
            L.gx = (rays + 127) / 128;
            L.gy = (uint32_t)P;
            L.block = 128;
            break;
        case 2:
            L.kernel = "k_raycast_fan<0, 64, false, 7, 0, false>";
            L.gx = grid1;
            L.gy = 1;
            L.block = 64;
            break;
        case 4: interleaved(0); break;
        default:
            if (fine && tile && ue && P % (8 * npw) == 0 && K <= 256)
                L = old_xcd(npw, ftile, lw, (uint32_t)P);
            else if (fine && ue && P % 8 == 0 && K <= 256) {
                L.kernel = "k_raycast_fan_xcd<0, 64, true, 8, 1, true, 1>";
                L.gx = grid1;
                L.gy = 1;
                L.block = 64;
            } else
                interleaved(0);
            break;
        }
    }
    L.full_grid = !culled;
    return L;
}

// ---- the new rule, formatted ---------------------------------------------------------------
static std::string pick_name(const FanPick &k) {
    switch (k.family) {
    case FanFamily::Coarse:
    case FanFamily::Fine:
        return fmt("k_raycast_fan<%d, 64, true, ", (int)k.mode) +
               fmt("%d, %d, ", k.family == FanFamily::Fine ? 8 : 7, k.FN) + tf(k.UE) + ">";
    case FanFamily::Xcd:
        return fmt("k_raycast_fan_xcd<%d, 64, true, 8, ", (int)k.mode) + fmt("%d, ", k.FN) +
               tf(k.UE) + fmt(", %d>", k.NPW);
    case FanFamily::PoseMajor: return fmt("k_raycast_fan_pm<%d, true>", k.block);
    case FanFamily::OccBit:
        return fmt("k_raycast_fan<%d, 64, false, 7, ", (int)k.mode) + fmt("%d, ", k.FN) +
               tf(k.UE) + ">";
    }
    return "?";
}
static Launch new_launch(FanMode mode, int fan_batch, bool fine, int ftile, bool ue, int P, int K,
                         int fan_npw_req, int burst, uint32_t live_w, uint32_t waves,
                         uint32_t rays) {
    const FanPick k = fan_pick(mode, fan_batch, fine, ftile, ue, P, K, fan_npw_req, burst > 0);
    const FanGrid g = fan_grid(k.full_grid ? waves : live_w, (uint32_t)P, rays, k);
    Launch L;
    L.full_grid = k.full_grid;
    if (g.x == 0) return L;   // fan_enqueue launches nothing
    L.kernel = pick_name(k);
    L.gx = g.x;
    L.gy = g.y;
    L.block = (uint32_t)k.block;
    return L;
}

int main() {
    static_assert(kStepLds == 256, "old_launch() restates the bound as a number");
    const int batches[] = {0, 1, 2, 3, 4, 7};
    const int Ks[] = {0, 1, 256, 257, 365};
    const int npws[] = {1, 2, 4, 8, 16, 32};
    int Ps[75];
    for (int i = 0; i < 72; ++i) Ps[i] = i + 1;
    Ps[72] = 128;
    Ps[73] = 256;
    Ps[74] = 65535;
    // 100 x 37 rays: 58 waves, the last one partial; live intervals: some, all, none
    const uint32_t rays = 3700, waves = (rays + 63) / 64;
    const uint32_t lives[] = {5, waves, 0};
    long cases = 0, mismatches = 0, launches = 0;
    for (int mode = 0; mode < 3; ++mode)
        for (int fb : batches)
            for (int layout = 0; layout < 6; ++layout)   // coarse with ftile 0 / 1 / 2, fine 0 / 1 / 2
                for (int ue = 0; ue < 2; ++ue)
                    for (int P : Ps)
                        for (int K : Ks)
                            for (int npw : npws)
                                for (int burst = 0; burst < 2; ++burst) {
                                    const bool fine = layout >= 3;
                                    const int ftile = layout % 3;
                                    ++cases;
                                    for (uint32_t lw : lives) {
                                        const Launch a =
                                            old_launch(mode == 1, mode == 2, fb, fine, ftile, ue != 0,
                                                       P, K, npw, burst * 5, lw, waves, rays);
                                        const Launch b =
                                            new_launch((FanMode)mode, fb, fine, ftile, ue != 0, P, K,
                                                       npw, burst * 5, lw, waves, rays);
                                        if (!a.kernel.empty()) ++launches;
                                        if (a == b) continue;
                                        if (++mismatches <= 20)
                                            std::printf(
                                                "MISMATCH mode %d batch %d fine %d ftile %d ue %d P %d "
                                                "K %d npw %d burst %d lw %u: old %s [%u, %u] x %u "
                                                "full %d, new %s [%u, %u] x %u full %d\n",
                                                mode, fb, (int)fine, ftile, ue, P, K, npw, burst, lw,
                                                a.kernel.c_str(), a.gx, a.gy, a.block,
                                                (int)a.full_grid, b.kernel.c_str(), b.gx, b.gy,
                                                b.block, (int)b.full_grid);
                                    }
                                }
    const int reqs[] = {1, 2, 4, 8, 16, 32, 0, 3};
    for (int P = 1; P <= 256; ++P)
        for (int r : reqs) std::printf("npw %d %d -> %d\n", P, r, fan_npw(P, r));
    for (int ftile = 1; ftile <= 2; ++ftile)
        for (int P : {8, 24, 64, 96, 256})
            for (int r : npws)
                std::printf("kernel %d %d %d %s\n", ftile, P, r,
                            pick_name(fan_pick(FanMode::Plain, 0, true, ftile, true, P, 97, r, false))
                                .c_str());
    std::printf("%ld cases, %ld launches compared, %ld mismatches\n", cases, launches, mismatches);
    if (mismatches) return 1;
    std::printf("ok\n");
    return 0;
}
