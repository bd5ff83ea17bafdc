// Stand-alone check of pcp_fan_clip.hpp (DESIGN.md §5 Skip 3) with the host compiler: the clip
// interval's sample bounds over random and adversarial (box, pose, direction, K) cases, with the
// reciprocal exact and perturbed by +-1 and +-2 ulps (the device's is approximate).  Every
// sample outside [klo, khi] is recomputed in long double from the repeated-addition step table
// and must lie outside the box shrunk by fan_clip_delta, which must stay below the 1 mm query
// margin (beside the part the box's own 1e-6 |coord| inflation carries); a sample on a face
// stays in; e = 1 gives the whole-sample rule bit for bit.  No GPU call.  Prints "ok".
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "pcp_fan_clip.hpp"

using namespace pcp;

namespace {

int fails = 0;
long dropped_checked = 0, kept_total = 0, face_checked = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (++fails < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                                 \
    } while (0)

constexpr double R = 0.056, M = 1e-3;
const float kInvStep = (float)(1.0 / 0.3);
const int kKs[4] = {49, 256, 257, 4096};

std::vector<double> steps;   // s_0 = 0.5, s_(k+1) = s_k + 0.3: the reference's additions

struct Case {
    float fb[6];
    double p[3], d[3];
    int K;
    int face_k;              // a sample built to lie on a face (-1: none): it must be kept
    bool flush;              // denormal direction components reach the rule as zeros
};

// the rule as it was before the slack became a value
void whole_sample_rule(float t0, float t1, int K, int &klo, int &khi) {
    const float kl = ceilf((t0 - 0.5f) * kInvStep) - 1.0f;
    const float kh = floorf(fminf(t1, 1e30f) * kInvStep - 0.5f * kInvStep) + 1.0f;
    klo = (int)fminf(fmaxf(kl, 0.0f), (float)K);
    khi = (int)fminf(fmaxf(kh, -1.0f), (float)(K - 1));
}

float shift_ulps(float v, int n) {
    if (!std::isfinite(v) || v == 0.0f) return v;
    for (; n > 0; --n) v = std::nextafter(v, v > 0 ? INFINITY : -INFINITY);
    for (; n < 0; ++n) v = std::nextafter(v, 0.0f);
    return v;
}

// sample k in long double; true when it lies outside (or on the faces of) the box shrunk by delta
bool outside_shrunk(const Case &c, int k, long double delta) {
    for (int a = 0; a < 3; ++a) {
        const long double q = (long double)c.p[a] + (long double)c.d[a] * (long double)steps[k];
        if (q <= (long double)c.fb[2 * a] + delta || q >= (long double)c.fb[2 * a + 1] - delta)
            return true;
    }
    return false;
}

void check_case(const Case &c) {
    double amax = 0.0;
    for (int a = 0; a < 6; ++a) amax = std::fmax(amax, std::fabs((double)c.fb[a]));
    const double delta = fan_clip_delta(c.K, amax);
    // the bound: its constant part inside the margin m, its growing part inside 1e-6 A beside
    // the rounding of the faces themselves
    CHECK(fan_clip_delta(c.K, 0.0) < M);
    CHECK(delta - fan_clip_delta(c.K, 0.0) + amax / 16777216.0 <= 1e-6 * amax);
    float p[3], df[3];
    for (int a = 0; a < 3; ++a) {
        p[a] = (float)c.p[a];
        df[a] = (float)c.d[a];
        if (c.flush && std::fabs(df[a]) < FLT_MIN) df[a] = std::copysign(0.0f, df[a]);
    }
    for (int s = -2; s <= 2; ++s) {
        float inv[3];
        for (int a = 0; a < 3; ++a) inv[a] = shift_ulps(1.0f / df[a], s);
        // e = 1 against the whole-sample rule, bit for bit
        int kl1, kh1, klr = 0, khr = -1;
        fan_clip(c.fb, p, inv, kInvStep, kClipSlackWhole, c.K, kl1, kh1);
        float t0, t1;
        if (fan_clip_slabs(c.fb, p, inv, t0, t1)) whole_sample_rule(t0, t1, c.K, klr, khr);
        CHECK(kl1 == klr && kh1 == khr);
        int klo, khi;
        fan_clip(c.fb, p, inv, kInvStep, kClipSlack, c.K, klo, khi);
        CHECK(klo >= 0 && klo <= c.K && khi >= -1 && khi <= c.K - 1);
        CHECK(klo >= kl1 && khi <= kh1);             // the small slack only ever drops more
        if (klo <= khi) CHECK(klo <= kl1 + 1 && khi >= kh1 - 1);   // at most the slack sample
        // every dropped sample, of both settings (e = 1 drops a subset: checked through klo, khi
        // of the small slack, and where it alone empties the interval through its own)
        for (int k = 0; k < c.K; ++k) {
            if (klo <= khi && k >= klo && k <= khi) continue;
            ++dropped_checked;
            CHECK(outside_shrunk(c, k, (long double)delta));
        }
        if (klo <= khi) kept_total += khi - klo + 1;
        if (c.face_k >= 0) {
            ++face_checked;
            CHECK(klo <= c.face_k && c.face_k <= khi);
            CHECK(kl1 <= c.face_k && c.face_k <= kh1);
        }
    }
}

struct Gen {
    std::mt19937 rng{20260311u};
    std::uniform_real_distribution<double> U{0.0, 1.0};
    double u(double a, double b) { return a + (b - a) * U(rng); }
    int K() { return U(rng) < 0.12 ? 4096 : kKs[(int)(U(rng) * 3.0)]; }

    // a terrain-like clip box around `at`: the bounding box inflated as GridIndex::view does
    void box(Case &c, const double at[3], double sx, double sy, double sz) {
        const double lo[3] = {at[0] - sx, at[1] - sy, at[2] - sz};
        const double hi[3] = {at[0] + sx, at[1] + sy, at[2] + sz};
        double amax = 0.0;
        for (int a = 0; a < 3; ++a) amax = std::fmax(amax, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
        const double rb = R + M + 1e-6 * amax;
        for (int a = 0; a < 3; ++a) {
            c.fb[2 * a] = (float)(lo[a] - rb);
            c.fb[2 * a + 1] = (float)(hi[a] + rb);
        }
    }
    void unit(double d[3], double el, double az) {
        d[0] = std::cos(el) * std::cos(az);
        d[1] = std::cos(el) * std::sin(az);
        d[2] = std::sin(el);
    }
    void origin(double at[3]) {
        const double far = U(rng);
        const double s = far < 0.5 ? 10.0 : far < 0.8 ? 3000.0 : far < 0.95 ? 2e4 : 1e5;
        for (int a = 0; a < 3; ++a) at[a] = u(-s, s);
    }

    Case random_case() {
        Case c{};
        c.face_k = -1;
        c.K = K();
        double at[3];
        origin(at);
        const double reach = 0.5 + 0.3 * c.K;
        box(c, at, u(1.0, 60.0), u(1.0, 60.0), u(0.05, 3.0));
        unit(c.d, u(-1.5, 1.5), u(-3.2, 3.2));
        const double how = U(rng);
        for (int a = 0; a < 3; ++a) {
            const double w = c.fb[2 * a + 1] - c.fb[2 * a];
            c.p[a] = how < 0.3 ? u(c.fb[2 * a], c.fb[2 * a + 1])                   // inside
                   : how < 0.8 ? u(c.fb[2 * a] - 3.0, c.fb[2 * a + 1] + 3.0)       // near
                               : u(c.fb[2 * a] - 0.4 * reach - w, c.fb[2 * a + 1] + 0.4 * reach + w);
        }
        if (how >= 0.3 && how < 0.8 && U(rng) < 0.7) {   // the benchmark's shape: a metre above
            c.p[2] = c.fb[5] + u(0.0, 2.0);
            if (U(rng) < 0.3) c.p[2] = c.fb[4] - u(0.0, 2.0), c.d[2] = std::fabs(c.d[2]);   // ascending
        }
        return c;
    }

    // the entry (or exit) through face `f` of axis a falls exactly on sample k
    Case on_sample(bool exit) {
        Case c = random_case();
        const int a = (int)(U(rng) * 3.0) % 3;
        const int k = (int)(U(rng) * std::fmin(c.K, 40));
        if (std::fabs(c.d[a]) < 0.05) c.d[a] = c.d[a] < 0 ? -0.3 : 0.3;
        // entry through the low face when d > 0, the high face when d < 0; exit the other way
        const int f = 2 * a + ((c.d[a] > 0) == exit ? 1 : 0);
        c.p[a] = (double)c.fb[f] - c.d[a] * steps[k];
        bool inside = true;
        for (int b = 0; b < 3; ++b) {
            if (b == a) continue;
            const double m = 0.5 * ((double)c.fb[2 * b] + c.fb[2 * b + 1]);
            c.p[b] = m - c.d[b] * steps[k] + u(-0.2, 0.2);   // the crossing lies mid-box on b
            const double q = c.p[b] + c.d[b] * steps[k];
            inside = inside && q > c.fb[2 * b] + 0.1 && q < c.fb[2 * b + 1] - 0.1;
        }
        // (far from the origin the pose's own float rounding, 2^-24 |p| / |d_a| of t, exceeds the
        // slack: there the sample is on the face only to within delta, and may go)
        double pmax = 0.0;
        for (int b = 0; b < 3; ++b) pmax = std::fmax(pmax, std::fabs(c.p[b]));
        c.face_k = inside && pmax < 300.0 ? k : -1;
        return c;
    }

    // a direction component that is 0, -0, denormal or tiny, start inside / outside / on a face
    Case degenerate(int kind, int where) {
        Case c = random_case();
        const int a = (int)(U(rng) * 3.0) % 3;
        static const double tiny[] = {0.0, -0.0, 1e-40, -1e-40, 1e-45, 1e-30, -1e-30, 1e-20, -1e-12, 3e-39};
        c.d[a] = tiny[kind % 10];
        c.flush = kind >= 10;
        const int b = (a + 1) % 3, e = (a + 2) % 3;
        const double n = std::sqrt(c.d[b] * c.d[b] + c.d[e] * c.d[e]);
        if (n > 0) c.d[b] /= n, c.d[e] /= n;
        c.p[a] = where == 0   ? u(c.fb[2 * a] + 0.01, c.fb[2 * a + 1] - 0.01)
                 : where == 1 ? (double)c.fb[2 * a]
                 : where == 2 ? (double)c.fb[2 * a + 1]
                 : where == 3 ? c.fb[2 * a] - u(0.0, 1.0)
                              : c.fb[2 * a + 1] + u(0.0, 1.0);
        return c;
    }

    // a start exactly on a face, any direction
    Case on_face() {
        Case c = random_case();
        const int f = (int)(U(rng) * 6.0) % 6;
        c.p[f / 2] = (double)c.fb[f];
        for (int b = 0; b < 3; ++b)
            if (b != f / 2) c.p[b] = u(c.fb[2 * b], c.fb[2 * b + 1]);
        return c;
    }
};

// a vertical ray over a box whose faces, pose and times are exact in float: the bounds are the
// interval's own first and last sample, nothing more
void exact_vertical() {
    for (int K : kKs)
        for (int k0 = 0; k0 < 8; ++k0) {
            Case c{};
            c.K = K;
            c.face_k = -1;
            const float fb[6] = {-8.0f, 8.0f, -8.0f, 8.0f, -1.875f, 0.125f};
            for (int a = 0; a < 6; ++a) c.fb[a] = fb[a];
            c.d[2] = -1.0;
            c.p[0] = 0.25, c.p[1] = -0.5;
            // entry at t = 0.5 + 0.25 k0, exit 2 later: k0 = 0 and 6 enter on samples 0 and 5
            // (t = 0.5, 2.0), k0 = 4 leaves on sample 10 (t = 3.5)
            c.p[2] = 0.125 + 0.5 + 0.25 * k0;
            check_case(c);
            const float p[3] = {(float)c.p[0], (float)c.p[1], (float)c.p[2]};
            const float inv[3] = {INFINITY, INFINITY, -1.0f};
            int klo, khi;
            fan_clip(c.fb, p, inv, kInvStep, kClipSlack, K, klo, khi);
            const double t0 = 0.5 + 0.25 * k0, t1 = t0 + 2.0;
            int want_lo = 0, want_hi = -1;
            for (int k = 0; k < K; ++k)
                if (steps[k] >= t0 - 1e-9 && steps[k] <= t1 + 1e-9) {
                    if (want_hi < 0) want_lo = k;
                    want_hi = k;
                }
            CHECK(klo == want_lo && khi == want_hi);
        }
}

}  // namespace

int main() {
    steps.push_back(0.5);
    while (steps.size() < 4096) steps.push_back(steps.back() + 0.3);
    for (size_t k = 0; k < steps.size(); ++k) CHECK(std::fabs(steps[k] - (0.5 + 0.3 * (double)k)) < 5e-10);
    CHECK(kClipSlack * 0.3 > 10.0 * (4.1 * 1229.0 / 16777216.0 + 5e-10));   // (1) of the header
    CHECK(kClipSlackWhole == 1.0f && kClipSlack > 0.0f && kClipSlack < 1.0f);

    Gen g;
    for (int i = 0; i < 2500; ++i) check_case(g.random_case());
    for (int i = 0; i < 600; ++i) check_case(g.on_sample(false));
    for (int i = 0; i < 600; ++i) check_case(g.on_sample(true));
    for (int kind = 0; kind < 20; ++kind)
        for (int where = 0; where < 5; ++where)
            for (int i = 0; i < 4; ++i) check_case(g.degenerate(kind, where));
    for (int i = 0; i < 300; ++i) check_case(g.on_face());
    exact_vertical();
    // every K with the box kilometres away and the pose a metre above it
    for (int K : kKs)
        for (int i = 0; i < 40; ++i) {
            Case c = g.random_case();
            c.K = K;
            const double at[3] = {3000.0, -3000.0, 3000.0};
            g.box(c, at, 40.0, 40.0, 0.2);
            c.p[0] = at[0] + g.u(-30, 30), c.p[1] = at[1] + g.u(-30, 30);
            c.p[2] = c.fb[5] + g.u(0.5, 1.5);
            g.unit(c.d, g.u(-1.5, 0.05), g.u(-3.2, 3.2));
            check_case(c);
        }
    CHECK(dropped_checked > 1000000 && kept_total > 100000 && face_checked > 2000);
    std::printf("dropped samples checked %ld, kept %ld, face samples %ld\n", dropped_checked,
                kept_total, face_checked);
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
