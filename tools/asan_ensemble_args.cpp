// Stand-alone host check of the ensemble entry points (include/dsp_frontend.h: dsp_svm_create, dsp_svm_destroy,
// dsp_svm_decision_batch, dsp_ensemble_decide_batch, dsp_trim_preemph_batch; csrc/dsp_ensemble.hip).  Under
// dsp_debug_host_dry_run(1) create builds its transposed, padded tables in host memory, so the table builder runs here, and
// every argument error is DSP_EINVAL with a message before any device call: the program needs no GPU.
// `make -C dsp-speech-recognition_amd/csrc asan-ensemble` builds it with AddressSanitizer + UBSan against the sanitized build
// of the library and runs it; it needs no preloaded runtime.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "asan_args.h"
#include "dsp_frontend.h"

int main() {
    dsp_debug_host_dry_run(1);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    // exact-size arrays: a read past either end of a table is a report
    const int sizes[][2] = {{1, 1}, {5, 63}, {5, 64}, {5, 65}, {16, 257}, {3, 65536}};
    std::vector<dsp_svm*> made;
    for (const auto& s : sizes) {
        const int F = s[0], n = s[1];
        std::vector<double> sv((size_t)n * F), dual(n), scale(F), center(F);
        for (size_t i = 0; i < sv.size(); ++i) sv[i] = 0.001 * (double)(i % 977);
        for (int i = 0; i < n; ++i) dual[i] = (i & 1) ? -0.5 : 0.5;
        for (int f = 0; f < F; ++f) { scale[f] = 1.0 + f; center[f] = 0.1 * f; }
        dsp_svm_desc d = {F, n, 0, 1, 0.25, -0.125, center.data(), scale.data(), sv.data(), dual.data()};
        dsp_svm* h = nullptr;
        EXPECT_OK(dsp_svm_create(&d, &h));
        if (h) made.push_back(h);
        d.h_center = nullptr;
        d.h_scale = nullptr;
        h = nullptr;
        EXPECT_OK(dsp_svm_create(&d, &h));
        EXPECT_OK(dsp_svm_destroy(h));
    }
    EXPECT_OK(dsp_svm_destroy(nullptr));

    double sv[10] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0}, dual[2] = {0.5, -0.5}, scale[5] = {1, 2, 3, 4, 5}, center[5] = {0, 0, 0, 0, 0};
    const dsp_svm_desc good = {5, 2, 0, 1, 0.5, 0.25, center, scale, sv, dual};
    dsp_svm* h = nullptr;
    dsp_svm_desc d = good;
    EXPECT(dsp_svm_create(nullptr, &h), "NULL");
    EXPECT(dsp_svm_create(&d, nullptr), "NULL");
    d = good; d.n_features = 0; EXPECT(dsp_svm_create(&d, &h), "n_features");
    d = good; d.n_features = 17; EXPECT(dsp_svm_create(&d, &h), "n_features");
    d = good; d.n_sv = 0; EXPECT(dsp_svm_create(&d, &h), "n_sv");
    d = good; d.n_sv = 65537; EXPECT(dsp_svm_create(&d, &h), "n_sv");
    d = good; d.gamma = 0.0; EXPECT(dsp_svm_create(&d, &h), "gamma");
    d = good; d.gamma = -1.0; EXPECT(dsp_svm_create(&d, &h), "gamma");
    d = good; d.gamma = inf; EXPECT(dsp_svm_create(&d, &h), "gamma");
    d = good; d.gamma = nan; EXPECT(dsp_svm_create(&d, &h), "gamma");
    d = good; d.intercept = nan; EXPECT(dsp_svm_create(&d, &h), "intercept");
    d = good; d.h_sv = nullptr; EXPECT(dsp_svm_create(&d, &h), "NULL");
    d = good; d.h_dual = nullptr; EXPECT(dsp_svm_create(&d, &h), "NULL");
    scale[3] = 0.0; EXPECT(dsp_svm_create(&good, &h), "scale[3]");
    scale[3] = inf; EXPECT(dsp_svm_create(&good, &h), "scale[3]");
    scale[3] = 4.0;
    center[1] = nan; EXPECT(dsp_svm_create(&good, &h), "center[1]");
    center[1] = 0.0;
    sv[7] = inf; EXPECT(dsp_svm_create(&good, &h), "support vector");
    sv[7] = 0.8;
    dual[1] = nan; EXPECT(dsp_svm_create(&good, &h), "dual");
    dual[1] = -0.5;
    if (h != nullptr) { std::printf("a failed create left a handle behind\n"); ++g_bad; }

    dsp_svm *a = nullptr, *b = nullptr, *c3 = nullptr;
    EXPECT_OK(dsp_svm_create(&good, &a));
    EXPECT_OK(dsp_svm_create(&good, &b));
    d = good; d.n_features = 3;
    EXPECT_OK(dsp_svm_create(&d, &c3));

    alignas(16) static double feat[64];              // pointers that are only checked, never followed
    alignas(16) static float logits[64];
    alignas(16) static int32_t ints[64];
    static int64_t offs[8];
    EXPECT(dsp_svm_decision_batch(nullptr, feat, 5, 1, feat, ints, nullptr), "NULL");
    EXPECT(dsp_svm_decision_batch(a, nullptr, 5, 1, feat, ints, nullptr), "NULL");
    EXPECT(dsp_svm_decision_batch(a, feat, 5, 0, feat, ints, nullptr), "n_rows");
    EXPECT(dsp_svm_decision_batch(a, feat, 4, 1, feat, ints, nullptr), "ld_feat");
    EXPECT(dsp_svm_decision_batch(a, feat, 5, 1, nullptr, nullptr, nullptr), "nothing to write");
    EXPECT(dsp_svm_decision_batch(a, feat, 5, 1, feat, ints, nullptr), "dry_run");

    dsp_ensemble_rule r2[2] = {{0, 1, 0.8, a}, {6, 7, 0.7, b}};
    EXPECT(dsp_ensemble_decide_batch(nullptr, 20, 1, 20, r2, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "NULL");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, feat, 5, nullptr, 0, nullptr, logits, ints, feat, nullptr), "NULL");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, feat, 5, nullptr, 0, ints, logits, nullptr, feat, nullptr), "NULL");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 0, 20, r2, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "n_utt");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 1, r2, 0, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "n_classes");
    EXPECT(dsp_ensemble_decide_batch(logits, 65, 1, 65, r2, 0, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "n_classes");
    EXPECT(dsp_ensemble_decide_batch(logits, 19, 1, 20, r2, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "ld_logits");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 5, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "n_rules");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, -1, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "n_rules");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, nullptr, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "NULL rules");
    EXPECT(dsp_ensemble_decide_batch(logits, 7, 1, 7, r2, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "label");
    r2[1].svm = nullptr;
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "NULL SVM");
    r2[1].svm = c3;
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "features");
    r2[1].svm = b;
    r2[1].label_a = 1;
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "overlap");
    r2[1].label_a = 6;
    r2[0].threshold = nan;
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "threshold");
    r2[0].threshold = 0.8;
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, nullptr, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "NULL features");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, feat, 4, nullptr, 0, ints, logits, ints, feat, nullptr), "ld_feat");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, feat, 5, ints, 0, ints, logits, ints, feat, nullptr), "ld_valid");
    EXPECT(dsp_ensemble_decide_batch(logits, 20, 1, 20, r2, 2, feat, 5, nullptr, 0, ints, logits, ints, feat, nullptr), "dry_run");

    EXPECT(dsp_trim_preemph_batch(nullptr, DSP_WAVE_I16, offs, offs, offs, 1, 0.97, logits, nullptr), "NULL");
    EXPECT(dsp_trim_preemph_batch(logits, DSP_WAVE_F32, nullptr, offs, offs, 1, 0.97, logits, nullptr), "NULL");
    EXPECT(dsp_trim_preemph_batch(logits, DSP_WAVE_F32, offs, nullptr, offs, 1, 0.97, logits, nullptr), "NULL");
    EXPECT(dsp_trim_preemph_batch(logits, DSP_WAVE_F32, offs, offs, nullptr, 1, 0.97, logits, nullptr), "NULL");
    EXPECT(dsp_trim_preemph_batch(logits, DSP_WAVE_F32, offs, offs, offs, 1, 0.97, nullptr, nullptr), "NULL");
    EXPECT(dsp_trim_preemph_batch(logits, DSP_WAVE_F32, offs, offs, offs, 0, 0.97, logits, nullptr), "n_utt");
    EXPECT(dsp_trim_preemph_batch(logits, 7, offs, offs, offs, 1, 0.97, logits, nullptr), "wave_dtype");
    EXPECT(dsp_trim_preemph_batch(logits, DSP_WAVE_F32, offs, offs, offs, 1, nan, logits, nullptr), "coefficient");

    EXPECT_OK(dsp_svm_destroy(a));
    EXPECT_OK(dsp_svm_destroy(b));
    EXPECT_OK(dsp_svm_destroy(c3));
    for (dsp_svm* m : made) EXPECT_OK(dsp_svm_destroy(m));
    dsp_debug_host_dry_run(0);
    return finish("asan_ensemble_args");
}
