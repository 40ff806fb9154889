// The row-bounded products of libdsp_frontend.so (include/dsp_frontend.h: dsp_rows_wgrad_scratch_bytes, dsp_rows_wgrad,
// dsp_rows_product): argument checks and the launches of kernels_wgrad.h.  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_wgrad.h"
#include "rows_host.h"

namespace {

int64_t scratch_floats(int32_t T, int32_t B, int32_t m, int32_t n) { return wgrad_scratch_floats(T, B, m, n); }

}  // namespace

extern "C" {

int dsp_rows_wgrad_scratch_bytes(int32_t T, int32_t B, int32_t m, int32_t n, int64_t* out_bytes) {
    const char* who = "dsp_rows_wgrad_scratch_bytes";
    if (!out_bytes) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = check_sizes(who, T, B)) return rc;
    if (m < 1 || m > WGRAD_MAX_DIM) return dsp_fail(DSP_EINVAL, "%s: m %d must be in [1, %d]", who, m, WGRAD_MAX_DIM);
    if (n < 1 || n > WGRAD_MAX_DIM) return dsp_fail(DSP_EINVAL, "%s: n %d must be in [1, %d]", who, n, WGRAD_MAX_DIM);
    *out_bytes = scratch_floats(T, B, m, n) * 4;
    return DSP_OK;
}

int dsp_rows_wgrad(const dsp_rows_operand* a, const dsp_rows_operand* x, int32_t shift, const float* d_x_init, int64_t init_stride_b,
                   const float* d_scale, int32_t T, int32_t B, const int32_t* d_rows, float* d_c, float* d_colsum, void* d_scratch,
                   int64_t scratch_bytes, void* stream) {
    const char* who = "dsp_rows_wgrad";
    if (int rc = check_sizes(who, T, B)) return rc;
    RowsOp A, X;
    Range ra, rx;
    if (int rc = check_operand(who, "a", a, T, B, &A, &ra)) return rc;
    if (int rc = check_operand(who, "x", x, T, B, &X, &rx)) return rc;
    if (shift < -1 || shift > 1) return dsp_fail(DSP_EINVAL, "%s: shift %d must be -1, 0 or 1", who, shift);
    if (!d_c) return dsp_fail(DSP_EINVAL, "%s: NULL output d_c", who);
    if (!d_scratch) return dsp_fail(DSP_EINVAL, "%s: NULL scratch", who);
    if (!aligned(d_c, 4) || (d_colsum && !aligned(d_colsum, 4)) || (d_scale && !aligned(d_scale, 4)) || (d_x_init && !aligned(d_x_init, 4)) ||
        (d_rows && !aligned(d_rows, 4)))
        return dsp_fail(DSP_EINVAL, "%s: every pointer must be 4-byte aligned", who);
    if (!aligned(d_scratch, 16)) return dsp_fail(DSP_EINVAL, "%s: scratch must be 16-byte aligned", who);
    const int32_t m = A.cols, n = X.cols;
    const int64_t need = scratch_floats(T, B, m, n) * 4;
    if (scratch_bytes < need)
        return dsp_fail(DSP_EINVAL, "%s: scratch of %lld bytes is short of the %lld dsp_rows_wgrad_scratch_bytes asks for", who,
                        (long long)scratch_bytes, (long long)need);
    Range ri{0, 0};
    if (d_x_init) {
        if (shift != -1) return dsp_fail(DSP_EINVAL, "%s: an initial row needs shift -1 (got %d)", who, shift);
        if (init_stride_b < n || init_stride_b > ((int64_t)1 << 40) / B)
            return dsp_fail(DSP_EINVAL, "%s: init_stride_b %lld must be in [%d, 2^40 / B]", who, (long long)init_stride_b, n);
        ri = range_of(d_x_init, ((int64_t)(B - 1) * init_stride_b + n) * 4);
        if (!(aligned(d_x_init, 16) && (init_stride_b & 3) == 0)) X.vec = 0;
    }
    const Range rs = range_of(d_scale, (int64_t)T * B * 4);
    // outputs and scratch against everything that is read, and against each other
    const Range outs[3] = {range_of(d_c, (int64_t)m * n * 4), range_of(d_colsum, m * 4), range_of(d_scratch, need)};
    const char* out_names[3] = {"d_c", "d_colsum", "scratch"};
    const Range ins[5] = {ra, rx, ri, rs, range_of(d_rows, 4)};
    const char* in_names[5] = {"operand a", "operand x", "the initial row", "the scale", "d_rows"};
    if (int rc = check_overlaps(who, outs, out_names, 3, ins, in_names, 5)) return rc;
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    hipStream_t st = (hipStream_t)stream;
    const int steps = wgrad_chunk_steps(B);
    const int chunks = (T + steps - 1) / steps;
    const int tiles_m = (m + WGRAD_TILE - 1) / WGRAD_TILE, tiles_n = (n + WGRAD_TILE - 1) / WGRAD_TILE;
    float* part = static_cast<float*>(d_scratch);
    float* cpart = part + (int64_t)chunks * tiles_m * tiles_n * (WGRAD_TILE * WGRAD_TILE);
    rows_wgrad_kernel<<<dim3(tiles_m * tiles_n, chunks), WGRAD_THREADS, 0, st>>>(A, X, shift, d_x_init, init_stride_b, d_scale, T, B, d_rows,
                                                                                 tiles_n, part, d_colsum ? cpart : nullptr);
    HIP_TRY(hipGetLastError());
    const int64_t elems = (int64_t)m * n + (d_colsum ? m : 0);
    rows_wgrad_reduce_kernel<<<dim3((unsigned)((elems + 255) / 256)), 256, 0, st>>>(part, cpart, m, n, tiles_m, tiles_n, T, B, d_rows, d_c,
                                                                                    d_colsum);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_rows_product(const dsp_rows_operand* a0, const float* d_w0, const dsp_rows_operand* a1, const float* d_w1, int32_t n, int32_t T,
                     int32_t B, const int32_t* d_rows, float* d_y, void* stream) {
    const char* who = "dsp_rows_product";
    if (int rc = check_sizes(who, T, B)) return rc;
    if (n < 1 || n > WGRAD_MAX_DIM) return dsp_fail(DSP_EINVAL, "%s: n %d must be in [1, %d]", who, n, WGRAD_MAX_DIM);
    RowsTerm P[2] = {};
    Range ra[2] = {}, rw[2] = {};
    const dsp_rows_operand* ops[2] = {a0, a1};
    const float* ws[2] = {d_w0, d_w1};
    const char* names[2] = {"a0", "a1"};
    if ((a1 == nullptr) != (d_w1 == nullptr)) return dsp_fail(DSP_EINVAL, "%s: a1 and d_w1 are given together or not at all", who);
    const int nterms = a1 ? 2 : 1;
    for (int p = 0; p < nterms; ++p) {
        if (int rc = check_operand(who, names[p], ops[p], T, B, &P[p].a, &ra[p])) return rc;
        if (!ws[p]) return dsp_fail(DSP_EINVAL, "%s: NULL matrix d_w%d", who, p);
        if (!aligned(ws[p], 4)) return dsp_fail(DSP_EINVAL, "%s: every pointer must be 4-byte aligned", who);
        P[p].w = ws[p];
        P[p].wvec = aligned(ws[p], 16) && (n & 3) == 0;
        rw[p] = range_of(ws[p], (int64_t)P[p].a.cols * n * 4);
    }
    if (!d_y) return dsp_fail(DSP_EINVAL, "%s: NULL output d_y", who);
    if (!aligned(d_y, 4) || (d_rows && !aligned(d_rows, 4))) return dsp_fail(DSP_EINVAL, "%s: every pointer must be 4-byte aligned", who);
    const Range ry = range_of(d_y, (int64_t)T * B * n * 4);
    for (int p = 0; p < nterms; ++p) {
        if (overlap(ry, ra[p])) return dsp_fail(DSP_EINVAL, "%s: d_y overlaps operand %s", who, names[p]);
        if (overlap(ry, rw[p])) return dsp_fail(DSP_EINVAL, "%s: d_y overlaps d_w%d", who, p);
    }
    if (overlap(ry, range_of(d_rows, 4))) return dsp_fail(DSP_EINVAL, "%s: d_y overlaps d_rows", who);
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    const int64_t total = (int64_t)T * B;
    const dim3 grid((unsigned)((total + WGRAD_TILE - 1) / WGRAD_TILE), (n + WGRAD_TILE - 1) / WGRAD_TILE);
    const int yvec = aligned(d_y, 16) && (n & 3) == 0;
    rows_product_kernel<<<grid, WGRAD_THREADS, 0, (hipStream_t)stream>>>(P[0], P[1], nterms, n, T, B, d_rows, d_y, yvec);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // extern "C"
