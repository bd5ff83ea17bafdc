/* devmath_host.c -- pcp_crmath.h and pcp_libm.h as a small shared object of array entry points:
 * the host (gcc) build of the two headers, element by element, for tests/test_crmath_exact.py
 * (against the exact reference tests/cr_ref.py) and tests/test_device_math_gpu.py (the device
 * build of the same text against this one).  Build: gcc -O2 -ffp-contract=off -shared -fPIC. */
#include <stdint.h>

#include "pcp_crmath.h"
#include "pcp_libm.h"

void dm_score_sin_part(const double *d, const double *r0, int64_t n, double *out, int32_t *phase) {
    for (int64_t i = 0; i < n; ++i) {
        int ph = 0;
        out[i] = pcp_score_sin_part(d[i], r0[i], &ph);
        phase[i] = ph;
    }
}

void dm_acos_fix(const double *d, const double *r0, int64_t n, double *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = pcp_cr_acos_fix(d[i], r0[i]);
}

void dm_cr_sin(const double *a, int64_t n, double *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = pcp_cr_sin(a[i]);
}

void dm_atan2_fix(const double *y, const double *x, const double *r0, int64_t n, double *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = pcp_cr_atan2_fix(y[i], x[i], r0[i]);
}

void dm_atan2f(const float *y, const float *x, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = pcp_atan2f(y[i], x[i]);
}

void dm_sinf(const float *a, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = pcp_sinf(a[i]);
}

void dm_cosf(const float *a, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = pcp_cosf(a[i]);
}

void dm_divf(const float *a, const float *b, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = pcp_lm_div(a[i], b[i]);
}

void dm_sqrtf(const float *a, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = pcp_lm_sqrt(a[i]);
}
