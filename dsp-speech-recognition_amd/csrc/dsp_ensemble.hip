// The ensemble entry points of libdsp_frontend.so (include/dsp_frontend.h: dsp_svm_*, dsp_ensemble_decide_batch,
// dsp_trim_preemph_batch): argument checks, the table handle of a fitted SVM and the launches of kernels_ensemble.h.
// gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_ensemble.h"

// One fitted scaler + RBF SVM (include/dsp_frontend.h: dsp_svm); immutable after dsp_svm_create.
struct dsp_svm {
    int32_t F, n_sv, n_pad, class0, class1;
    double gamma, intercept;
    double* d_tables;      // one allocation: center [16] | scale [16] | dual [n_pad] | support vectors [F][n_pad]
    int device;            // -1 for a dry-run handle
    int dry_run;           // tables in HOST memory (dsp_debug_host_dry_run): the handle can be destroyed, nothing else
};

namespace {

SvmView svm_view(const dsp_svm* h) {
    SvmView m;
    m.center = h->d_tables;
    m.scale = h->d_tables + SVM_MAX_FEATURES;
    m.dual = h->d_tables + 2 * SVM_MAX_FEATURES;
    m.sv_t = m.dual + h->n_pad;
    m.F = h->F;
    m.n_pad = h->n_pad;
    m.class0 = h->class0;
    m.class1 = h->class1;
    m.gamma = h->gamma;
    m.intercept = h->intercept;
    return m;
}

// A handle a launch may use: not a dry-run one, and of the current device.
int svm_check_usable(const char* who, const dsp_svm* h) {
    if (h->dry_run) return dsp_fail(DSP_EINVAL, "%s: the SVM handle was created under dsp_debug_host_dry_run: launches are refused", who);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != h->device) return dsp_fail(DSP_EINVAL, "%s: the SVM handle belongs to device %d, current device is %d", who, h->device, dev);
    return DSP_OK;
}

inline int ens_blocks(int32_t n) { return (n + ENS_ROWS_PER_BLOCK - 1) / ENS_ROWS_PER_BLOCK; }

}  // namespace

extern "C" {

int dsp_svm_create(const dsp_svm_desc* d, dsp_svm** out) {
    if (!d || !out) return dsp_fail(DSP_EINVAL, "dsp_svm_create: NULL argument");
    *out = nullptr;
    if (d->n_features < 1 || d->n_features > SVM_MAX_FEATURES)
        return dsp_fail(DSP_EINVAL, "dsp_svm_create: n_features %d must be in [1, %d]", d->n_features, SVM_MAX_FEATURES);
    if (d->n_sv < 1 || d->n_sv > SVM_MAX_SV) return dsp_fail(DSP_EINVAL, "dsp_svm_create: n_sv %d must be in [1, %d]", d->n_sv, SVM_MAX_SV);
    if (!std::isfinite(d->gamma) || d->gamma <= 0.0) return dsp_fail(DSP_EINVAL, "dsp_svm_create: gamma must be finite and positive");
    if (!std::isfinite(d->intercept)) return dsp_fail(DSP_EINVAL, "dsp_svm_create: the intercept is not finite");
    if (!d->h_sv || !d->h_dual) return dsp_fail(DSP_EINVAL, "dsp_svm_create: NULL support vectors / dual coefficients");
    const int32_t F = d->n_features, n = d->n_sv, n_pad = (n + 63) / 64 * 64;
    for (int f = 0; f < F; ++f) {
        if (d->h_scale && (!std::isfinite(d->h_scale[f]) || d->h_scale[f] == 0.0))
            return dsp_fail(DSP_EINVAL, "dsp_svm_create: scale[%d] must be finite and not zero", f);
        if (d->h_center && !std::isfinite(d->h_center[f])) return dsp_fail(DSP_EINVAL, "dsp_svm_create: center[%d] is not finite", f);
    }
    for (int64_t i = 0; i < (int64_t)n * F; ++i)
        if (!std::isfinite(d->h_sv[i])) return dsp_fail(DSP_EINVAL, "dsp_svm_create: a support vector is not finite");
    for (int32_t i = 0; i < n; ++i)
        if (!std::isfinite(d->h_dual[i])) return dsp_fail(DSP_EINVAL, "dsp_svm_create: a dual coefficient is not finite");
    std::vector<double> t((size_t)2 * SVM_MAX_FEATURES + (size_t)n_pad * (1 + F), 0.0);
    double* center = t.data();
    double* scale = center + SVM_MAX_FEATURES;
    double* dual = scale + SVM_MAX_FEATURES;
    double* sv_t = dual + n_pad;
    for (int f = 0; f < SVM_MAX_FEATURES; ++f) {
        center[f] = (f < F && d->h_center) ? d->h_center[f] : 0.0;
        scale[f] = (f < F && d->h_scale) ? d->h_scale[f] : 1.0;
    }
    for (int32_t i = 0; i < n; ++i) {
        dual[i] = d->h_dual[i];
        for (int f = 0; f < F; ++f) sv_t[(size_t)f * n_pad + i] = d->h_sv[(size_t)i * F + f];
    }
    int dev = -1;
    if (!g_host_dry_run) HIP_TRY(hipGetDevice(&dev));
    void* tables = nullptr;
    const hipError_t e = dsp_table_alloc_copy(&tables, t.data(), t.size() * sizeof(double));
    if (e != hipSuccess) return dsp_fail(DSP_EHIP, "dsp_svm_create: %s", hipGetErrorString(e));
    dsp_svm* h = new dsp_svm();
    h->F = F; h->n_sv = n; h->n_pad = n_pad;
    h->class0 = d->class0; h->class1 = d->class1;
    h->gamma = d->gamma; h->intercept = d->intercept;
    h->d_tables = static_cast<double*>(tables);
    h->dry_run = g_host_dry_run ? 1 : 0;
    h->device = dev;
    *out = h;
    return DSP_OK;
}

int dsp_svm_destroy(dsp_svm* h) {
    if (!h) return DSP_OK;
    dsp_table_free(h->d_tables, h->dry_run);
    delete h;
    return DSP_OK;
}

int dsp_svm_decision_batch(const dsp_svm* h, const double* d_feat, int64_t ld_feat, int32_t n_rows, double* d_decision,
                           int32_t* d_label, void* stream) {
    const char* who = "dsp_svm_decision_batch";
    if (!h || !d_feat) return dsp_fail(DSP_EINVAL, "%s: NULL handle / features", who);
    if (n_rows < 1) return dsp_fail(DSP_EINVAL, "%s: n_rows %d must be >= 1", who, n_rows);
    if (ld_feat < h->F) return dsp_fail(DSP_EINVAL, "%s: ld_feat %lld is below the %d features of the model", who, (long long)ld_feat, h->F);
    if (!d_decision && !d_label) return dsp_fail(DSP_EINVAL, "%s: nothing to write (both outputs are NULL)", who);
    if (int rc = svm_check_usable(who, h)) return rc;
    svm_rbf_kernel<<<ens_blocks(n_rows), 64 * ENS_ROWS_PER_BLOCK, 0, (hipStream_t)stream>>>(svm_view(h), d_feat, ld_feat, n_rows, d_decision, d_label);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_ensemble_decide_batch(const float* d_logits, int64_t ld_logits, int32_t n_utt, int32_t n_classes,
                              const dsp_ensemble_rule* rules, int32_t n_rules, const double* d_feat, int64_t ld_feat,
                              const int32_t* d_valid, int64_t ld_valid, int32_t* d_pred, float* d_prob, int32_t* d_used,
                              double* d_decision, void* stream) {
    const char* who = "dsp_ensemble_decide_batch";
    if (!d_logits || !d_pred || !d_used) return dsp_fail(DSP_EINVAL, "%s: NULL logits / d_pred / d_used", who);
    if (n_utt < 1) return dsp_fail(DSP_EINVAL, "%s: n_utt %d must be >= 1", who, n_utt);
    if (n_classes < 2 || n_classes > 64) return dsp_fail(DSP_EINVAL, "%s: n_classes %d must be in [2, 64]", who, n_classes);
    if (ld_logits < n_classes) return dsp_fail(DSP_EINVAL, "%s: ld_logits %lld is below n_classes %d", who, (long long)ld_logits, n_classes);
    if (n_rules < 0 || n_rules > ENS_MAX_RULES) return dsp_fail(DSP_EINVAL, "%s: n_rules %d must be in [0, %d]", who, n_rules, ENS_MAX_RULES);
    if (n_rules > 0 && !rules) return dsp_fail(DSP_EINVAL, "%s: NULL rules", who);
    for (int r = 0; r < n_rules; ++r) {
        const dsp_ensemble_rule& q = rules[r];
        if (!q.svm) return dsp_fail(DSP_EINVAL, "%s: rule %d has a NULL SVM handle", who, r);
        if (q.label_a < 0 || q.label_a >= n_classes || q.label_b < 0 || q.label_b >= n_classes)
            return dsp_fail(DSP_EINVAL, "%s: rule %d names a label outside [0, %d)", who, r, n_classes);
        if (std::isnan(q.threshold)) return dsp_fail(DSP_EINVAL, "%s: rule %d has a NaN threshold", who, r);
        if (q.svm->F != rules[0].svm->F)
            return dsp_fail(DSP_EINVAL, "%s: rule %d's SVM takes %d features, rule 0's takes %d", who, r, q.svm->F, rules[0].svm->F);
        for (int k = 0; k < r; ++k)
            if (q.label_a == rules[k].label_a || q.label_a == rules[k].label_b || q.label_b == rules[k].label_a || q.label_b == rules[k].label_b)
                return dsp_fail(DSP_EINVAL, "%s: the label sets of rules %d and %d overlap", who, k, r);
    }
    if (n_rules > 0) {
        if (!d_feat) return dsp_fail(DSP_EINVAL, "%s: NULL features with %d rules", who, n_rules);
        if (ld_feat < rules[0].svm->F)
            return dsp_fail(DSP_EINVAL, "%s: ld_feat %lld is below the %d features of the models", who, (long long)ld_feat, rules[0].svm->F);
        if (d_valid && ld_valid < 1) return dsp_fail(DSP_EINVAL, "%s: ld_valid %lld must be >= 1", who, (long long)ld_valid);
    }
    for (int r = 0; r < n_rules; ++r)
        if (int rc = svm_check_usable(who, rules[r].svm)) return rc;
    EnsParams P = {};
    P.logits = d_logits; P.ld_logits = ld_logits;
    P.n_utt = n_utt; P.C = n_classes; P.n_rules = n_rules;
    for (int r = 0; r < n_rules; ++r) {
        P.rules[r].label_a = rules[r].label_a;
        P.rules[r].label_b = rules[r].label_b;
        P.rules[r].threshold = rules[r].threshold;
        P.rules[r].svm = svm_view(rules[r].svm);
    }
    P.feat = d_feat; P.ld_feat = ld_feat;
    P.valid = n_rules > 0 ? d_valid : nullptr; P.ld_valid = ld_valid;
    P.pred = d_pred; P.prob = d_prob; P.used = d_used; P.decision = d_decision;
    ensemble_decide_kernel<<<ens_blocks(n_utt), 64 * ENS_ROWS_PER_BLOCK, 0, (hipStream_t)stream>>>(P);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_trim_preemph_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets, const int64_t* d_segments,
                           const int64_t* d_dst_offsets, int32_t n_utt, double coeff, float* d_out, void* stream) {
    const char* who = "dsp_trim_preemph_batch";
    if (!d_wave || !d_sample_offsets || !d_segments || !d_dst_offsets || !d_out) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (n_utt < 1) return dsp_fail(DSP_EINVAL, "%s: n_utt %d must be >= 1", who, n_utt);
    if (wave_dtype != DSP_WAVE_I16 && wave_dtype != DSP_WAVE_F32) return dsp_fail(DSP_EINVAL, "%s: unsupported wave_dtype %d", who, wave_dtype);
    if (!std::isfinite(coeff)) return dsp_fail(DSP_EINVAL, "%s: the coefficient is not finite", who);
    hipStream_t st = (hipStream_t)stream;
    if (wave_dtype == DSP_WAVE_I16)
        trim_preemph_kernel<DSP_WAVE_I16><<<n_utt, 256, 0, st>>>(d_wave, d_sample_offsets, d_segments, d_dst_offsets, coeff, d_out);
    else
        trim_preemph_kernel<DSP_WAVE_F32><<<n_utt, 256, 0, st>>>(d_wave, d_sample_offsets, d_segments, d_dst_offsets, coeff, d_out);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // extern "C"
