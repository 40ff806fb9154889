// The reproducible-dropout entry points of libdsp_frontend.so (include/dsp_frontend.h: dsp_rng_advance, dsp_dropout_apply,
// dsp_dropout_apply_key, dsp_dropout_multipliers): argument checks and the launches of kernels_dropout.h.  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_dropout.h"

namespace {

const int64_t kMaxElems = (int64_t)1 << 34;                      // element_index / 4 is one 32-bit counter word

// p in [0, 1) -> the keep threshold and the scale of a kept element, both formed in double.
int keep_rule(const char* who, double p, uint32_t* thr, float* scale) {
    if (!(p >= 0.0 && p < 1.0)) return dsp_fail(DSP_EINVAL, "%s: p %g must be in [0, 1)", who, p);
    *thr = (uint32_t)std::llrint((1.0 - p) * 16777216.0);
    *scale = (float)(1.0 / (1.0 - p));
    return DSP_OK;
}

int check_state(const char* who, const char* name, const void* d_state) {
    if (!d_state) return dsp_fail(DSP_EINVAL, "%s: NULL %s", who, name);
    if (!aligned(d_state, 8)) return dsp_fail(DSP_EINVAL, "%s: %s must be 8-byte aligned", who, name);
    return DSP_OK;
}

int check_site(const char* who, int32_t site, int32_t count) {
    if (site < 0 || site > 0x7fffffff - count) return dsp_fail(DSP_EINVAL, "%s: site %d must be in [0, 2^31 - %d)", who, site, count);
    return DSP_OK;
}

int apply(const char* who, const char* state_name, const float* d_x, float* d_y, int64_t n, double p, int32_t site, const int64_t* d_state,
          int64_t* d_key_out, void* stream) {
    if (!d_x || !d_y) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = check_state(who, state_name, d_state)) return rc;
    if (d_key_out && !aligned(d_key_out, 8)) return dsp_fail(DSP_EINVAL, "%s: d_key_out must be 8-byte aligned", who);
    if (!aligned(d_x, 4) || !aligned(d_y, 4)) return dsp_fail(DSP_EINVAL, "%s: every tensor must be 4-byte aligned", who);
    if (n < 0) return dsp_fail(DSP_EINVAL, "%s: n %lld must be >= 0", who, (long long)n);
    if (n >= kMaxElems) return dsp_fail(DSP_EINVAL, "%s: n %lld must be below 2^34", who, (long long)n);
    uint32_t thr;
    float scale;
    if (int rc = keep_rule(who, p, &thr, &scale)) return rc;
    if (int rc = check_site(who, site, 1)) return rc;
    const Range rx = range_of(d_x, n * 4), ry = range_of(d_y, n * 4), rs = range_of(d_state, 16);
    if (d_x != d_y && overlap(rx, ry)) return dsp_fail(DSP_EINVAL, "%s: d_x and d_y overlap in part (d_y == d_x is served)", who);
    if (overlap(ry, rs)) return dsp_fail(DSP_EINVAL, "%s: d_y overlaps %s", who, state_name);
    if (d_key_out) {
        const Range rk = range_of(d_key_out, 16);
        if (overlap(rk, rx) || overlap(rk, ry) || overlap(rk, rs)) return dsp_fail(DSP_EINVAL, "%s: d_key_out overlaps another argument", who);
    }
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    const int grid = grid_for((n + 3) / 4, DROPOUT_THREADS);
    const long long* st = reinterpret_cast<const long long*>(d_state);
    long long* key = reinterpret_cast<long long*>(d_key_out);
    if (aligned(d_x, 16) && aligned(d_y, 16))
        dropout_apply_kernel<true><<<grid, DROPOUT_THREADS, 0, (hipStream_t)stream>>>(d_x, d_y, (long long)n, thr, scale, (uint32_t)site, st, key);
    else
        dropout_apply_kernel<false><<<grid, DROPOUT_THREADS, 0, (hipStream_t)stream>>>(d_x, d_y, (long long)n, thr, scale, (uint32_t)site, st, key);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_rng_advance(int64_t* d_state, void* stream) {
    const char* who = "dsp_rng_advance";
    if (int rc = check_state(who, "d_state", d_state)) return rc;
    if (int rc = dsp_refuse_dry_run(who)) return rc;
    rng_advance_kernel<<<1, 1, 0, (hipStream_t)stream>>>(reinterpret_cast<long long*>(d_state));
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_dropout_apply(const float* d_x, float* d_y, int64_t n, double p, int32_t site, const int64_t* d_state, int64_t* d_key_out, void* stream) {
    return apply("dsp_dropout_apply", "d_state", d_x, d_y, n, p, site, d_state, d_key_out, stream);
}

int dsp_dropout_apply_key(const float* d_g, float* d_dx, int64_t n, double p, int32_t site, const int64_t* d_key, void* stream) {
    return apply("dsp_dropout_apply_key", "d_key", d_g, d_dx, n, p, site, d_key, nullptr, stream);
}

int dsp_dropout_multipliers(float* d_m, int32_t L, int32_t T, int32_t B, int32_t C, double p, int32_t site_base, const int64_t* d_state,
                            const int32_t* d_rows, void* stream) {
    const char* who = "dsp_dropout_multipliers";
    if (!d_m) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = check_state(who, "d_state", d_state)) return rc;
    if (!aligned(d_m, 4) || (d_rows && !aligned(d_rows, 4))) return dsp_fail(DSP_EINVAL, "%s: d_m and d_rows must be 4-byte aligned", who);
    if (L < 1 || L > 64) return dsp_fail(DSP_EINVAL, "%s: L %d must be in [1, 64]", who, L);
    if (T < 1 || B < 1 || C < 1) return dsp_fail(DSP_EINVAL, "%s: T %d, B %d, C %d must be >= 1", who, T, B, C);
    const int64_t row = (int64_t)B * C;                          // below 2^62
    if (row >= kMaxElems || row > (kMaxElems - 1) / T)
        return dsp_fail(DSP_EINVAL, "%s: T B C = %d x %d x %d must be below 2^34", who, T, B, C);
    const int64_t per_layer = row * T;
    uint32_t thr;
    float scale;
    if (int rc = keep_rule(who, p, &thr, &scale)) return rc;
    if (int rc = check_site(who, site_base, L)) return rc;
    const Range rm = range_of(d_m, per_layer * L * 4);
    if (overlap(rm, range_of(d_state, 16))) return dsp_fail(DSP_EINVAL, "%s: d_m overlaps d_state", who);
    if (overlap(rm, range_of(d_rows, 4))) return dsp_fail(DSP_EINVAL, "%s: d_m overlaps d_rows", who);
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    const dim3 grid((unsigned)grid_for((per_layer + 3) / 4, DROPOUT_THREADS), (unsigned)L);
    const long long* st = reinterpret_cast<const long long*>(d_state);
    if (aligned(d_m, 16) && (per_layer & 3) == 0)
        dropout_multipliers_kernel<true><<<grid, DROPOUT_THREADS, 0, (hipStream_t)stream>>>(d_m, T, per_layer, row, thr, scale, (uint32_t)site_base, st, d_rows);
    else
        dropout_multipliers_kernel<false><<<grid, DROPOUT_THREADS, 0, (hipStream_t)stream>>>(d_m, T, per_layer, row, thr, scale, (uint32_t)site_base, st, d_rows);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // extern "C"
