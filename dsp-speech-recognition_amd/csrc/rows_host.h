// The argument checks shared by the row-bounded entry points (csrc/dsp_wgrad.hip, csrc/dsp_reduce.hip): sizes and one
// operand view.  Host only.
#pragma once

#include <stdint.h>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_wgrad.h"

namespace {

int check_sizes(const char* who, int32_t T, int32_t B) {
    if (T < 1) return dsp_fail(DSP_EINVAL, "%s: T %d must be >= 1", who, T);
    if (B < 1) return dsp_fail(DSP_EINVAL, "%s: B %d must be >= 1", who, B);
    if ((int64_t)T * B > 0x7fffffff) return dsp_fail(DSP_EINVAL, "%s: T B = %lld must be below 2^31", who, (long long)T * B);
    if ((T + wgrad_chunk_steps(B) - 1) / wgrad_chunk_steps(B) > 65535)
        return dsp_fail(DSP_EINVAL, "%s: T %d gives more than 65535 chunks of %d time steps", who, T, wgrad_chunk_steps(B));
    return DSP_OK;
}

// One operand view: pointer, strides, columns; -> the kernel's form and the bytes it may read.
int check_operand(const char* who, const char* name, const dsp_rows_operand* op, int32_t T, int32_t B, RowsOp* out, Range* span) {
    if (!op) return dsp_fail(DSP_EINVAL, "%s: NULL operand %s", who, name);
    if (!op->d_ptr) return dsp_fail(DSP_EINVAL, "%s: NULL pointer in operand %s", who, name);
    if (!aligned(op->d_ptr, 4)) return dsp_fail(DSP_EINVAL, "%s: operand %s must be 4-byte aligned", who, name);
    if (op->cols < 1 || op->cols > WGRAD_MAX_DIM)
        return dsp_fail(DSP_EINVAL, "%s: operand %s: cols %d must be in [1, %d]", who, name, op->cols, WGRAD_MAX_DIM);
    if (op->stride_t < 0 || op->stride_b < 0)
        return dsp_fail(DSP_EINVAL, "%s: operand %s: strides (%lld, %lld) must not be negative", who, name, (long long)op->stride_t,
                        (long long)op->stride_b);
    if (op->reserved != 0) return dsp_fail(DSP_EINVAL, "%s: operand %s: reserved must be 0", who, name);
    const int64_t lim = (int64_t)1 << 40;                                   // floats: far above any buffer, far below an int64 overflow
    if (op->stride_t > lim / T || op->stride_b > lim / B)
        return dsp_fail(DSP_EINVAL, "%s: operand %s: strides (%lld, %lld) too large for T %d, B %d", who, name, (long long)op->stride_t,
                        (long long)op->stride_b, T, B);
    out->p = op->d_ptr;
    out->st = op->stride_t;
    out->sb = op->stride_b;
    out->cols = op->cols;
    out->vec = aligned(op->d_ptr, 16) && (op->stride_t & 3) == 0 && (op->stride_b & 3) == 0;
    *span = range_of(op->d_ptr, ((int64_t)(T - 1) * op->stride_t + (int64_t)(B - 1) * op->stride_b + op->cols) * 4);
    return DSP_OK;
}

}  // namespace
