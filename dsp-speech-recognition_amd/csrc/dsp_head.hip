// The head entry points of libdsp_frontend.so (include/dsp_frontend.h: dsp_head_lengths_batch, dsp_head_pool_batch,
// dsp_head_pool_train_batch, dsp_head_pool_backward_batch): argument checks and the launches of kernels_head.h.  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_head.h"

namespace {

// The checks the three pooling calls share: sizes, the two column ranges of the [B, ld] matrix, dry run.
int head_pool_check(const char* who, int32_t T, int32_t B, int32_t H, int64_t ld, const char* ld_name, const char* verb, int32_t col_avg,
                    int32_t col_max) {
    if (T < 1) return dsp_fail(DSP_EINVAL, "%s: T %d must be >= 1", who, T);
    if (B < 1) return dsp_fail(DSP_EINVAL, "%s: B %d must be >= 1", who, B);
    if (H < 1 || H > 65535 * 64) return dsp_fail(DSP_EINVAL, "%s: H %d must be in [1, %d]", who, H, 65535 * 64);
    if (col_max < 0) return dsp_fail(DSP_EINVAL, "%s: col_max %d is negative", who, col_max);
    if (col_avg >= 0 && col_avg < (int64_t)col_max + H && col_max < (int64_t)col_avg + H)
        return dsp_fail(DSP_EINVAL, "%s: the columns of the average (%d) and of the maximum (%d) overlap", who, col_avg, col_max);
    const int64_t last = (int64_t)(col_avg > col_max ? col_avg : col_max) + H;
    if (ld < last) return dsp_fail(DSP_EINVAL, "%s: %s %lld is below the %lld columns %s", who, ld_name, (long long)ld, (long long)last, verb);
    if (int rc = dsp_refuse_dry_run(who)) return rc;
    return DSP_OK;
}

// dsp_head_pool_batch (d_arg NULL) and dsp_head_pool_train_batch: the same kernel, with or without the row of the maximum.
int head_pool(const char* who, const float* d_y, int32_t T, int32_t B, int32_t H, const int32_t* d_len, const int32_t* d_rows, float* d_feat,
              int64_t ld_feat, int32_t col_avg, int32_t col_max, int32_t* d_arg, void* stream) {
    if (!d_y || !d_len || !d_feat) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = head_pool_check(who, T, B, H, ld_feat, "ld_feat", "written", col_avg, col_max)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(64 * HEAD_POOL_WAVES);
    // 16-byte loads where every row of every column group is aligned: H a multiple of 4 and y itself aligned
    const bool wide = (H & 3) == 0 && (reinterpret_cast<uintptr_t>(d_y) & 15) == 0;
    const dim3 grid(B, wide ? (H / 4 + 63) / 64 : (H + 63) / 64);
    if (wide && d_arg) head_pool_kernel<4, true><<<grid, block, 0, st>>>(d_y, T, B, H, d_len, d_rows, d_feat, ld_feat, col_avg, col_max, d_arg);
    else if (wide) head_pool_kernel<4><<<grid, block, 0, st>>>(d_y, T, B, H, d_len, d_rows, d_feat, ld_feat, col_avg, col_max);
    else if (d_arg) head_pool_kernel<1, true><<<grid, block, 0, st>>>(d_y, T, B, H, d_len, d_rows, d_feat, ld_feat, col_avg, col_max, d_arg);
    else head_pool_kernel<1><<<grid, block, 0, st>>>(d_y, T, B, H, d_len, d_rows, d_feat, ld_feat, col_avg, col_max);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_head_lengths_batch(const int32_t* d_len0, int32_t B, int32_t T, int32_t hir, int32_t* d_len0c, int32_t* d_len1, int32_t* d_info,
                           void* stream) {
    const char* who = "dsp_head_lengths_batch";
    if (!d_len0 || !d_len0c || !d_len1 || !d_info) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (B < 1 || B > HEAD_MAX_B) return dsp_fail(DSP_EINVAL, "%s: B %d must be in [1, %d]", who, B, HEAD_MAX_B);
    if (T < 1) return dsp_fail(DSP_EINVAL, "%s: T %d must be >= 1", who, T);
    if (hir < 1) return dsp_fail(DSP_EINVAL, "%s: hir %d must be >= 1", who, hir);
    if (int rc = dsp_refuse_dry_run(who)) return rc;
    head_lengths_kernel<<<1, HEAD_LEN_THREADS, 0, (hipStream_t)stream>>>(d_len0, B, T, hir, d_len0c, d_len1, d_info);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_head_pool_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const int32_t* d_len, const int32_t* d_rows, float* d_feat,
                        int64_t ld_feat, int32_t col_avg, int32_t col_max, void* stream) {
    return head_pool("dsp_head_pool_batch", d_y, T, B, H, d_len, d_rows, d_feat, ld_feat, col_avg, col_max, nullptr, stream);
}

int dsp_head_pool_train_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const int32_t* d_len, const int32_t* d_rows, float* d_feat,
                              int64_t ld_feat, int32_t col_avg, int32_t col_max, int32_t* d_arg, void* stream) {
    const char* who = "dsp_head_pool_train_batch";
    if (!d_arg) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    return head_pool(who, d_y, T, B, H, d_len, d_rows, d_feat, ld_feat, col_avg, col_max, d_arg, stream);
}

int dsp_head_pool_backward_batch(const float* d_gfeat, int64_t ld_g, int32_t col_avg, int32_t col_max, const int32_t* d_len,
                                 const int32_t* d_arg, int32_t T, int32_t B, int32_t H, float* d_gy, void* stream) {
    const char* who = "dsp_head_pool_backward_batch";
    if (!d_gfeat || !d_len || !d_arg || !d_gy) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = head_pool_check(who, T, B, H, ld_g, "ld_g", "read", col_avg, col_max)) return rc;
    hipStream_t st = (hipStream_t)stream;
    // 16-byte stores where every row of every column group is aligned: H a multiple of 4 and gy itself aligned
    if ((H & 3) == 0 && (reinterpret_cast<uintptr_t>(d_gy) & 15) == 0)
        head_pool_bwd_kernel<4><<<dim3(B, (H / 4 + 63) / 64), 64 * HEAD_POOL_WAVES, 0, st>>>(d_gfeat, ld_g, col_avg, col_max, d_len, d_arg, T, B, H, d_gy);
    else
        head_pool_bwd_kernel<1><<<dim3(B, (H + 63) / 64), 64 * HEAD_POOL_WAVES, 0, st>>>(d_gfeat, ld_g, col_avg, col_max, d_len, d_arg, T, B, H, d_gy);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // extern "C"
