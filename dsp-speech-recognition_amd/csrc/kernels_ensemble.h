// The last step of the reference's ensemble (ensemble.py:44-67) on the device: the pre-emphasised, endpoint-trimmed copy of
// the clips the pitch features are taken from (pitch_model.py:55-57), the RBF support-vector machine on those features
// (pitch_model.py:59-61: RobustScaler.transform + SVC.predict, written out from their public attributes) and the confidence
// gate that lets it overrule the classifier (ensemble.py:49-53, behind model.py:156-157).  Everything is fp64 except the
// logits and the probabilities, which are fp32 as torch holds them.  gfx950 only (wave64).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dsp_common.h"
#include "softmax_row.h"

#define SVM_MAX_FEATURES 16
#define SVM_MAX_SV 65536
#define ENS_MAX_RULES 4
#define ENS_ROWS_PER_BLOCK 4      // one wave per row / clip, 256 threads

// One fitted model as the kernels see it: pointers into the handle's single table allocation.
struct SvmView {
    const double* center;   // [SVM_MAX_FEATURES]  RobustScaler.center_ (zeros without centering)
    const double* scale;    // [SVM_MAX_FEATURES]  RobustScaler.scale_ (ones without scaling)
    const double* dual;     // [n_pad]             SVC.dual_coef_[0], zeros behind n_sv
    const double* sv_t;     // [F][n_pad]          SVC.support_vectors_ transposed, zeros behind n_sv
    int32_t F, n_pad;       // n_pad = n_sv rounded up to whole waves
    int32_t class0, class1;
    double gamma, intercept;
};

struct EnsRule {
    int32_t label_a, label_b;
    double threshold;
    SvmView svm;
};

struct EnsParams {
    const float* logits;
    int64_t ld_logits;
    int32_t n_utt, C, n_rules;
    EnsRule rules[ENS_MAX_RULES];
    const double* feat;
    int64_t ld_feat;
    const int32_t* valid;
    int64_t ld_valid;
    int32_t* pred;
    float* prob;
    int32_t* used;
    double* decision;
};

// dec(x) = sum_i dual_i exp(-gamma |(x - center) / scale - sv_i|^2) + intercept for the row at `x`, by one whole wave:
// every lane scales the row (a true division, as RobustScaler.transform), lanes stride over the support vectors -- the
// padded ones carry dual = 0 and add an exact zero, so there is no tail branch --, each lane adds its terms in ascending
// order and the butterfly adds the lanes.  Products and sums are spelled as fma / single operations, so the value does not
// depend on what the compiler may contract around the call: the stand-alone kernel and the gate return the same bits.
__device__ __forceinline__ double svm_decision_wave(const SvmView& m, const double* __restrict__ x, int lane) {
    double z[SVM_MAX_FEATURES];
#pragma unroll
    for (int f = 0; f < SVM_MAX_FEATURES; ++f) z[f] = f < m.F ? (x[f] - m.center[f]) / m.scale[f] : 0.0;
    const double neg_gamma = -m.gamma;
    double acc = 0.0;
    for (int i = lane; i < m.n_pad; i += 64) {
        double d2 = 0.0;
#pragma unroll
        for (int f = 0; f < SVM_MAX_FEATURES; ++f)
            if (f < m.F) {
                const double d = z[f] - m.sv_t[(int64_t)f * m.n_pad + i];
                d2 = fma(d, d, d2);
            }
        acc = fma(m.dual[i], exp(neg_gamma * d2), acc);
    }
    return ens_wave_sum(acc) + m.intercept;
}

// pitch_model.py:59-61 for n_rows rows of features: one wave per row.
__global__ __launch_bounds__(64 * ENS_ROWS_PER_BLOCK) void svm_rbf_kernel(SvmView m, const double* __restrict__ feat, int64_t ld_feat,
                                                                         int32_t n_rows, double* __restrict__ decision,
                                                                         int32_t* __restrict__ label) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * ENS_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= n_rows) return;                       // a whole wave leaves; nothing below synchronises the workgroup
    const double dec = svm_decision_wave(m, feat + row * ld_feat, lane);
    if (lane == 0) {
        if (decision != nullptr) decision[row] = dec;
        if (label != nullptr) label[row] = dec > 0.0 ? m.class1 : m.class0;
    }
}

// model.py:156-157 and ensemble.py:49-53 for a batch: one wave per clip, lane c < C holds logit c.
//   prob = softmax(logits) in fp64 (max subtracted), rounded to fp32          F.softmax(out, dim=1)
//   pred = the lowest index among the largest logits                           torch.max(out, 1)
//   the rule whose label pair holds pred fires when (double)prob[pred] < threshold (the reference compares the fp32
//   probability as a Python float); its SVM then decides from the clip's pitch features, if they are valid.
// The branch into the SVM is wave-uniform: a wave is one clip.
__global__ __launch_bounds__(64 * ENS_ROWS_PER_BLOCK) void ensemble_decide_kernel(EnsParams P) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * ENS_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= P.n_utt) return;
    const bool mine = lane < P.C;
    const float lf = mine ? P.logits[b * P.ld_logits + lane] : -INFINITY;
    const RowSoftmax sm = row_softmax_wave(lf, mine);          // softmax_row.h: shared with the loss kernels, bit for bit
    const int pred = sm.pred;
    const float p = sm.p;
    if (P.prob != nullptr && mine) P.prob[b * P.C + lane] = p;
    const double p_pred = (double)__shfl(p, pred, 64);
    int fired = -1;
#pragma unroll
    for (int r = 0; r < ENS_MAX_RULES; ++r)
        if (r < P.n_rules && fired < 0 && (pred == P.rules[r].label_a || pred == P.rules[r].label_b) &&
            p_pred < P.rules[r].threshold)
            fired = r;
    int32_t out = pred, used = 0;
    double dec = 0.0;
    if (fired >= 0) {
        const bool ok = P.valid == nullptr || P.valid[b * P.ld_valid] != 0;
        if (ok) {
            SvmView m = P.rules[0].svm;
#pragma unroll
            for (int r = 1; r < ENS_MAX_RULES; ++r)
                if (fired == r) m = P.rules[r].svm;
            dec = svm_decision_wave(m, P.feat + b * P.ld_feat, lane);
            out = dec > 0.0 ? m.class1 : m.class0;
            used = fired + 1;
        } else {
            used = -(fired + 1);
        }
    }
    if (lane == 0) {
        P.pred[b] = out;
        P.used[b] = used;
        if (P.decision != nullptr) P.decision[b] = dec;
    }
}

// pitch_model.py:55-57 for a ragged batch: sig = preemphasis(sig, coeff) over the WHOLE clip, then sig[l:r] -- the first
// kept sample uses x[l - 1], and y[0] = x[0] only where l = 0 (preprocess.py:19).  fp64 with the product and the
// difference rounded separately, as NumPy's `signal[1:] - coeff * signal[:-1]` rounds them (the build contracts a * b + c
// otherwise), then one rounding to fp32.  One workgroup per utterance, the tables of dsp_trim_scale_batch; the segment is
// clipped to the clip as numpy slicing does.
template <int DTYPE>
__global__ __launch_bounds__(256) void trim_preemph_kernel(const void* __restrict__ wave, const int64_t* __restrict__ src_off,
                                                           const int64_t* __restrict__ seg, const int64_t* __restrict__ dst_off,
                                                           double coeff, float* __restrict__ out) {
    const int b = blockIdx.x;
    const int64_t base = src_off[b], len = src_off[b + 1] - base;
    int64_t l = seg[2 * b], r = seg[2 * b + 1];
    if (l < 0) l = 0;
    if (r > len) r = len;
    float* dst = out + dst_off[b];
    for (int64_t i = l + threadIdx.x; i < r; i += 256) {
        const double x = (double)dsp_load_sample<DTYPE>(wave, base + i);
        double y = x;
        if (i > 0) {
            double prod = coeff * (double)dsp_load_sample<DTYPE>(wave, base + i - 1);
            // the rounded product, opaque to the compiler: with -ffp-contract=fast the backend fuses a product into the
            // difference behind it whatever the source says (__dmul_rn / __dsub_rn and a contract(off) pragma included)
            asm volatile("" : "+v"(prod));
            y = x - prod;
        }
        dst[i - l] = (float)y;
    }
}
