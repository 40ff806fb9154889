// The scoring entry points of libdsp_frontend.so (include/dsp_frontend.h: dsp_metrics_bytes, dsp_metrics_reset,
// dsp_xent_metrics_batch): argument checks and the launches of kernels_loss.h.  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_loss.h"

namespace {

int check_sizes(const char* who, int32_t n_classes, int32_t wrong_capacity) {
    if (n_classes < 2 || n_classes > XENT_MAX_CLASSES)
        return dsp_fail(DSP_EINVAL, "%s: n_classes %d must be in [2, %d]", who, n_classes, XENT_MAX_CLASSES);
    if (wrong_capacity < 0 || wrong_capacity > XENT_MAX_WRONG)
        return dsp_fail(DSP_EINVAL, "%s: wrong_capacity %d must be in [0, %d]", who, wrong_capacity, XENT_MAX_WRONG);
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_metrics_bytes(int32_t n_classes, int32_t wrong_capacity, int64_t* out_bytes) {
    const char* who = "dsp_metrics_bytes";
    if (!out_bytes) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    *out_bytes = 0;
    if (int rc = check_sizes(who, n_classes, wrong_capacity)) return rc;
    *out_bytes = xent_state_bytes(n_classes, wrong_capacity);
    return DSP_OK;
}

int dsp_metrics_reset(void* d_state, int32_t n_classes, int32_t wrong_capacity, void* stream) {
    const char* who = "dsp_metrics_reset";
    if (!d_state) return dsp_fail(DSP_EINVAL, "%s: NULL d_state", who);
    if (!aligned(d_state, 8)) return dsp_fail(DSP_EINVAL, "%s: d_state must be 8-byte aligned", who);
    if (int rc = check_sizes(who, n_classes, wrong_capacity)) return rc;
    if (int rc = dsp_refuse_dry_run(who)) return rc;
    const long long n_words = xent_state_bytes(n_classes, wrong_capacity) / 4;
    xent_reset_kernel<<<grid_for(n_words, 256), 256, 0, (hipStream_t)stream>>>(static_cast<int32_t*>(d_state), n_words);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_xent_metrics_batch(const float* d_logits, int64_t ld_logits, int32_t n_utt, int32_t n_classes, const int64_t* d_labels,
                           const int32_t* d_pred_in, const float* d_grad_out, float* d_nll, float* d_loss, int32_t* d_pred,
                           float* d_prob, float* d_dlogits, int64_t ld_dlogits, void* d_state, int32_t wrong_capacity, void* stream) {
    const char* who = "dsp_xent_metrics_batch";
    if (!d_logits || !d_labels) return dsp_fail(DSP_EINVAL, "%s: NULL logits / labels", who);
    if (n_utt < 1 || n_utt > XENT_MAX_UTT) return dsp_fail(DSP_EINVAL, "%s: n_utt %d must be in [1, %d]", who, n_utt, XENT_MAX_UTT);
    if (int rc = check_sizes(who, n_classes, d_state ? wrong_capacity : 0)) return rc;
    if (ld_logits < n_classes || ld_logits > ((int64_t)1 << 40))
        return dsp_fail(DSP_EINVAL, "%s: ld_logits %lld is below n_classes %d (or above 2^40)", who, (long long)ld_logits, n_classes);
    if (d_dlogits && (ld_dlogits < n_classes || ld_dlogits > ((int64_t)1 << 40)))
        return dsp_fail(DSP_EINVAL, "%s: ld_dlogits %lld is below n_classes %d (or above 2^40)", who, (long long)ld_dlogits, n_classes);
    if (!d_nll && !d_loss && !d_pred && !d_prob && !d_dlogits && !d_state)
        return dsp_fail(DSP_EINVAL, "%s: nothing to write (every output and d_state are NULL)", who);
    if (!aligned(d_logits, 4) || !aligned(d_pred_in, 4) || !aligned(d_grad_out, 4) || !aligned(d_nll, 4) || !aligned(d_loss, 4) ||
        !aligned(d_pred, 4) || !aligned(d_prob, 4) || !aligned(d_dlogits, 4))
        return dsp_fail(DSP_EINVAL, "%s: every fp32 / int32 tensor must be 4-byte aligned", who);
    if (!aligned(d_labels, 8)) return dsp_fail(DSP_EINVAL, "%s: d_labels must be 8-byte aligned", who);
    if (!aligned(d_state, 8)) return dsp_fail(DSP_EINVAL, "%s: d_state must be 8-byte aligned", who);

    // the outputs must lie apart from each other and from every input (inputs may share memory)
    const int64_t n = n_utt, C = n_classes;
    Ranges rg;
    rg.add("d_logits", d_logits, ((n - 1) * ld_logits + C) * 4, false);
    rg.add("d_labels", d_labels, n * 8, false);
    rg.add("d_pred_in", d_pred_in, n * 4, false);
    rg.add("d_grad_out", d_grad_out, 4, false);
    rg.add("d_nll", d_nll, n * 4, true);
    rg.add("d_loss", d_loss, 4, true);
    rg.add("d_pred", d_pred, n * 4, true);
    rg.add("d_prob", d_prob, n * C * 4, true);
    rg.add("d_dlogits", d_dlogits, ((n - 1) * ld_dlogits + C) * 4, true);
    rg.add("d_state", d_state, xent_state_bytes(n_classes, wrong_capacity), true);
    if (int rc = rg.check(who)) return rc;
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    XentParams P = {};
    P.logits = d_logits; P.ld_logits = ld_logits;
    P.n_utt = n_utt; P.C = n_classes;
    P.labels = d_labels; P.pred_in = d_pred_in; P.grad_out = d_grad_out;
    P.nll = d_nll; P.loss = d_loss; P.pred = d_pred; P.prob = d_prob;
    P.dlogits = d_dlogits; P.ld_dlogits = ld_dlogits;
    P.state = static_cast<long long*>(d_state); P.wrong_cap = d_state ? wrong_capacity : 0;
    hipStream_t st = (hipStream_t)stream;
    if (d_nll || d_pred || d_prob || d_dlogits) {
        const int blocks = (n_utt + XENT_ROWS_PER_BLOCK - 1) / XENT_ROWS_PER_BLOCK;
        xent_rows_kernel<<<blocks, 64 * XENT_ROWS_PER_BLOCK, 0, st>>>(P);
        HIP_TRY(hipGetLastError());
    }
    if (d_loss || d_state) {
        xent_reduce_kernel<<<1, XENT_REDUCE_THREADS, 0, st>>>(P);
        HIP_TRY(hipGetLastError());
    }
    return DSP_OK;
}

}  // extern "C"
