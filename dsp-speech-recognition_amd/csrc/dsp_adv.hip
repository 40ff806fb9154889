// The speaker-discriminator entry points of libdsp_frontend.so (include/dsp_frontend.h: dsp_adv_disc_work_bytes,
// dsp_adv_disc_forward, dsp_adv_disc_train): argument checks and the launches of kernels_adv.h, with the loss through the
// scoring kernels of kernels_loss.h and the parameter gradients through the row-reduction kernels of kernels_wgrad.h (T = 1).
// gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include <math.h>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_adv.h"
#include "kernels_loss.h"
#include "kernels_wgrad.h"

namespace {

int check_sizes(const char* who, int32_t B, int32_t F, int32_t H, int32_t S) {
    if (B < 1 || B > ADV_MAX_B) return dsp_fail(DSP_EINVAL, "%s: B %d must be in [1, %d]", who, B, ADV_MAX_B);
    if (F < 1 || F > ADV_MAX_F) return dsp_fail(DSP_EINVAL, "%s: F %d must be in [1, %d]", who, F, ADV_MAX_F);
    if (H < 1 || H > ADV_MAX_H) return dsp_fail(DSP_EINVAL, "%s: H %d must be in [1, %d]", who, H, ADV_MAX_H);
    if (S < 2 || S > ADV_MAX_S) return dsp_fail(DSP_EINVAL, "%s: S %d must be in [2, %d]", who, S, ADV_MAX_S);
    return DSP_OK;
}

int check_stride(const char* who, const char* name, int64_t ld, int32_t cols) {
    if (ld < cols || ld > ((int64_t)1 << 40))
        return dsp_fail(DSP_EINVAL, "%s: %s %lld is below the %d columns (or above 2^40)", who, name, (long long)ld, cols);
    return DSP_OK;
}

int64_t round16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// The workspace of dsp_adv_disc_train: | z [B, S] | dpre [B, H] | wgrad scratch | a matrix nobody asked for |
struct Work {
    int64_t z, dpre, scratch, scratch_bytes, spare, total;
};

Work work_layout(int32_t B, int32_t F, int32_t H, int32_t S) {
    Work w;
    w.z = 0;
    w.dpre = w.z + round16((int64_t)B * S * 4);
    w.scratch = w.dpre + round16((int64_t)B * H * 4);
    const int64_t s2 = wgrad_scratch_floats(1, B, S, H) * 4, s1 = wgrad_scratch_floats(1, B, H, F) * 4;
    w.scratch_bytes = s1 > s2 ? s1 : s2;
    w.spare = w.scratch + round16(w.scratch_bytes);
    w.total = w.spare + round16((int64_t)H * (F > S ? F : S) * 4);
    return w;
}

AdvParams forward_params(const float* d_feat, int64_t ld_feat, int32_t B, int32_t F, int32_t H, int32_t S, const float* d_W1,
                         const float* d_b1, const float* d_W2, const float* d_b2, float* d_a, float* z, int64_t ld_z) {
    AdvParams P = {};
    P.feat = d_feat; P.ld_feat = ld_feat;
    P.W1 = d_W1; P.b1 = d_b1; P.W2 = d_W2; P.b2 = d_b2;
    P.B = B; P.F = F; P.H = H; P.S = S;
    P.a = d_a; P.z = z; P.ld_z = ld_z;
    P.feat_vec = aligned(d_feat, 16) && (ld_feat & 3) == 0;
    P.w1_vec = aligned(d_W1, 16) && (F & 3) == 0;
    P.w2_vec = aligned(d_W2, 16) && (H & 3) == 0;
    return P;
}

// The checks both entry points share: sizes, the mandatory inputs, their alignment, the strides; the inputs' ranges go to `rg`.
int check_inputs(const char* who, const float* d_feat, int64_t ld_feat, int32_t B, int32_t F, int32_t H, int32_t S, const float* d_W1,
                 const float* d_b1, const float* d_W2, const float* d_b2, Ranges* rg) {
    if (int rc = check_sizes(who, B, F, H, S)) return rc;
    if (!d_feat || !d_W1 || !d_b1 || !d_W2 || !d_b2) return dsp_fail(DSP_EINVAL, "%s: NULL feat / W1 / b1 / W2 / b2", who);
    if (int rc = check_stride(who, "ld_feat", ld_feat, F)) return rc;
    if (!aligned(d_feat, 4) || !aligned(d_W1, 4) || !aligned(d_b1, 4) || !aligned(d_W2, 4) || !aligned(d_b2, 4))
        return dsp_fail(DSP_EINVAL, "%s: every fp32 tensor must be 4-byte aligned", who);
    rg->add("d_feat", d_feat, ((int64_t)(B - 1) * ld_feat + F) * 4, false);
    rg->add("d_W1", d_W1, (int64_t)H * F * 4, false);
    rg->add("d_b1", d_b1, (int64_t)H * 4, false);
    rg->add("d_W2", d_W2, (int64_t)S * H * 4, false);
    rg->add("d_b2", d_b2, (int64_t)S * 4, false);
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_adv_disc_work_bytes(int32_t B, int32_t F, int32_t H, int32_t S, int64_t* out_bytes) {
    const char* who = "dsp_adv_disc_work_bytes";
    if (!out_bytes) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    *out_bytes = 0;
    if (int rc = check_sizes(who, B, F, H, S)) return rc;
    *out_bytes = work_layout(B, F, H, S).total;
    return DSP_OK;
}

int dsp_adv_disc_forward(const float* d_feat, int64_t ld_feat, int32_t B, int32_t F, int32_t H, int32_t S, const float* d_W1,
                         const float* d_b1, const float* d_W2, const float* d_b2, float* d_a, float* d_logits2, int64_t ld_logits2,
                         void* stream) {
    const char* who = "dsp_adv_disc_forward";
    Ranges rg;
    if (int rc = check_inputs(who, d_feat, ld_feat, B, F, H, S, d_W1, d_b1, d_W2, d_b2, &rg)) return rc;
    if (!d_logits2) return dsp_fail(DSP_EINVAL, "%s: NULL output d_logits2", who);
    if (int rc = check_stride(who, "ld_logits2", ld_logits2, S)) return rc;
    if (!aligned(d_a, 4) || !aligned(d_logits2, 4)) return dsp_fail(DSP_EINVAL, "%s: every fp32 tensor must be 4-byte aligned", who);
    rg.add("d_a", d_a, (int64_t)B * H * 4, true);
    rg.add("d_logits2", d_logits2, ((int64_t)(B - 1) * ld_logits2 + S) * 4, true);
    if (int rc = rg.check(who)) return rc;
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    const AdvParams P = forward_params(d_feat, ld_feat, B, F, H, S, d_W1, d_b1, d_W2, d_b2, d_a, d_logits2, ld_logits2);
    adv_disc_fwd_kernel<<<(B + ADV_ROWS - 1) / ADV_ROWS, ADV_THREADS, 0, (hipStream_t)stream>>>(P);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_adv_disc_train(const float* d_feat, int64_t ld_feat, int32_t B, int32_t F, int32_t H, int32_t S, const float* d_W1,
                       const float* d_b1, const float* d_W2, const float* d_b2, const int64_t* d_speakers, const float* d_grad_out,
                       double gamma, const float* d_gamma, float* d_a, float* d_logits2, int64_t ld_logits2, float* d_loss2, float* d_dz,
                       float* d_dfeat, int64_t ld_dfeat, float* d_dW1, float* d_db1, float* d_dW2, float* d_db2, void* d_state,
                       int32_t wrong_capacity, void* d_work, int64_t work_bytes, void* stream) {
    const char* who = "dsp_adv_disc_train";
    Ranges rg;
    if (int rc = check_inputs(who, d_feat, ld_feat, B, F, H, S, d_W1, d_b1, d_W2, d_b2, &rg)) return rc;
    if (!d_speakers) return dsp_fail(DSP_EINVAL, "%s: NULL d_speakers", who);
    if (!d_a || !d_loss2 || !d_dz) return dsp_fail(DSP_EINVAL, "%s: NULL output d_a / d_loss2 / d_dz", who);
    if (!d_work) return dsp_fail(DSP_EINVAL, "%s: NULL workspace", who);
    if (!(fabs(gamma) <= 1e30)) return dsp_fail(DSP_EINVAL, "%s: gamma %g must be finite (|gamma| <= 1e30)", who, gamma);
    if (d_logits2)
        if (int rc = check_stride(who, "ld_logits2", ld_logits2, S)) return rc;
    if (d_dfeat)
        if (int rc = check_stride(who, "ld_dfeat", ld_dfeat, F)) return rc;
    const int32_t cap = d_state ? wrong_capacity : 0;
    if (cap < 0 || cap > XENT_MAX_WRONG)
        return dsp_fail(DSP_EINVAL, "%s: wrong_capacity %d must be in [0, %d]", who, cap, XENT_MAX_WRONG);
    if (!aligned(d_grad_out, 4) || !aligned(d_gamma, 4) || !aligned(d_a, 4) || !aligned(d_logits2, 4) || !aligned(d_loss2, 4) ||
        !aligned(d_dz, 4) || !aligned(d_dfeat, 4) || !aligned(d_dW1, 4) || !aligned(d_db1, 4) || !aligned(d_dW2, 4) || !aligned(d_db2, 4))
        return dsp_fail(DSP_EINVAL, "%s: every fp32 tensor must be 4-byte aligned", who);
    if (!aligned(d_speakers, 8)) return dsp_fail(DSP_EINVAL, "%s: d_speakers must be 8-byte aligned", who);
    if (!aligned(d_state, 8)) return dsp_fail(DSP_EINVAL, "%s: d_state must be 8-byte aligned", who);
    if (!aligned(d_work, 16)) return dsp_fail(DSP_EINVAL, "%s: the workspace must be 16-byte aligned", who);
    const Work w = work_layout(B, F, H, S);
    if (work_bytes < w.total)
        return dsp_fail(DSP_EINVAL, "%s: workspace of %lld bytes is short of the %lld dsp_adv_disc_work_bytes asks for", who,
                        (long long)work_bytes, (long long)w.total);

    rg.add("d_speakers", d_speakers, (int64_t)B * 8, false);
    rg.add("d_grad_out", d_grad_out, 4, false);
    rg.add("d_gamma", d_gamma, 4, false);
    rg.add("d_a", d_a, (int64_t)B * H * 4, true);
    rg.add("d_logits2", d_logits2, ((int64_t)(B - 1) * ld_logits2 + S) * 4, true);
    rg.add("d_loss2", d_loss2, 4, true);
    rg.add("d_dz", d_dz, (int64_t)B * S * 4, true);
    rg.add("d_dfeat", d_dfeat, ((int64_t)(B - 1) * ld_dfeat + F) * 4, true);
    rg.add("d_dW1", d_dW1, (int64_t)H * F * 4, true);
    rg.add("d_db1", d_db1, (int64_t)H * 4, true);
    rg.add("d_dW2", d_dW2, (int64_t)S * H * 4, true);
    rg.add("d_db2", d_db2, (int64_t)S * 4, true);
    rg.add("d_state", d_state, xent_state_bytes(S, cap), true);
    rg.add("the workspace", d_work, w.total, true);
    if (int rc = rg.check(who)) return rc;
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(d_work);
    float* z = d_logits2 ? d_logits2 : reinterpret_cast<float*>(base + w.z);
    const int64_t ld_z = d_logits2 ? ld_logits2 : S;
    float* dpre = reinterpret_cast<float*>(base + w.dpre);
    float* spare = reinterpret_cast<float*>(base + w.spare);
    const int blocks = (B + ADV_ROWS - 1) / ADV_ROWS;

    // 1. the forward
    AdvParams P = forward_params(d_feat, ld_feat, B, F, H, S, d_W1, d_b1, d_W2, d_b2, d_a, z, ld_z);
    adv_disc_fwd_kernel<<<blocks, ADV_THREADS, 0, st>>>(P);
    HIP_TRY(hipGetLastError());

    // 2. the loss, dz = (softmax - onehot) grad_out / n_scored and the metrics: the two scoring launches
    XentParams X = {};
    X.logits = z; X.ld_logits = ld_z;
    X.n_utt = B; X.C = S;
    X.labels = d_speakers; X.grad_out = d_grad_out;
    X.loss = d_loss2;
    X.dlogits = d_dz; X.ld_dlogits = S;
    X.state = static_cast<long long*>(d_state); X.wrong_cap = cap;
    xent_rows_kernel<<<(B + XENT_ROWS_PER_BLOCK - 1) / XENT_ROWS_PER_BLOCK, 64 * XENT_ROWS_PER_BLOCK, 0, st>>>(X);
    HIP_TRY(hipGetLastError());
    xent_reduce_kernel<<<1, XENT_REDUCE_THREADS, 0, st>>>(X);
    HIP_TRY(hipGetLastError());

    // 3. the backward over row tiles: dpre, and dfeat where asked for
    const bool want1 = d_dW1 || d_db1;
    if (d_dfeat || want1) {
        P.dz = d_dz; P.dpre = dpre;
        P.dfeat = d_dfeat; P.ld_dfeat = ld_dfeat;
        P.d_gamma = d_gamma; P.gamma = (float)gamma;
        P.dz_vec = aligned(d_dz, 16) && (S & 3) == 0;
        adv_disc_bwd_kernel<<<blocks, ADV_THREADS, 0, st>>>(P);
        HIP_TRY(hipGetLastError());
    }

    // 4. the parameter gradients: C[m, n] = sum_b A[b, m] X[b, n] with its column sum, T = 1
    auto wgrad = [&](const float* A, int64_t lda, int m, const float* Xp, int64_t ldx, int n, float* C, float* csum) -> int {
        RowsOp a = {A, 0, lda, m, (int32_t)(aligned(A, 16) && (lda & 3) == 0)};
        RowsOp x = {Xp, 0, ldx, n, (int32_t)(aligned(Xp, 16) && (ldx & 3) == 0)};
        const int tiles_m = (m + WGRAD_TILE - 1) / WGRAD_TILE, tiles_n = (n + WGRAD_TILE - 1) / WGRAD_TILE;
        float* part = reinterpret_cast<float*>(base + w.scratch);
        float* cpart = part + (int64_t)tiles_m * tiles_n * (WGRAD_TILE * WGRAD_TILE);       // one chunk: T = 1
        rows_wgrad_kernel<<<dim3(tiles_m * tiles_n, 1), WGRAD_THREADS, 0, st>>>(a, x, 0, nullptr, 0, nullptr, 1, B, nullptr, tiles_n, part,
                                                                              csum ? cpart : nullptr);
        HIP_TRY(hipGetLastError());
        const int64_t elems = (int64_t)m * n + (csum ? m : 0);
        rows_wgrad_reduce_kernel<<<dim3((unsigned)((elems + 255) / 256)), 256, 0, st>>>(part, cpart, m, n, tiles_m, tiles_n, 1, B, nullptr,
                                                                                        C ? C : spare, csum);
        HIP_TRY(hipGetLastError());
        return DSP_OK;
    };
    if (d_dW2 || d_db2)
        if (int rc = wgrad(d_dz, S, S, d_a, H, H, d_dW2, d_db2)) return rc;
    if (want1)
        if (int rc = wgrad(dpre, H, H, d_feat, ld_feat, F, d_dW1, d_db1)) return rc;
    return DSP_OK;
}

}  // extern "C"
