// Stand-alone host check of the fitting entry points (include/dsp_frontend.h: dsp_robust_scale_fit_batch, dsp_var_all,
// dsp_svm_fit_workspace_bytes, dsp_svm_fit_batch; csrc/dsp_svmfit.hip).  Every NULL, range, alignment, overlap and workspace
// error is DSP_EINVAL with a message before any device call, and under dsp_debug_host_dry_run(1) what passed every check is
// refused instead of launched: the program needs no GPU.  `make -C dsp-speech-recognition_amd/csrc asan-svmfit` builds it
// with AddressSanitizer + UBSan against the sanitized build of the library and runs it; it needs no preloaded runtime.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "asan_args.h"
#include "dsp_frontend.h"

int main() {
    dsp_debug_host_dry_run(1);
    const char* refused = "dry_run: launches are refused";
    // never reached by a kernel: every call below returns before a launch.  n = 8 rows of F = 3 features with ld = 4 and
    // P = 2 problems throughout: the workspace is 256 bytes of scaled rows and 2 x 8 row numbers.
    alignas(16) static double X[8 * 4], center[16], scale[16], out_scale[16], out_center[16], var[2], C[2], gamma[2], coef[2 * 8], rho[2];
    alignas(16) static int32_t valid[8 * 9], info[16];
    alignas(16) static int8_t Y[2 * 8], mask[8];
    alignas(16) static char work[256 + 64 + 16];
    const int64_t wb = 256 + 64;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    char* const X1 = reinterpret_cast<char*>(X) + 4;
    int64_t n = 0;

    // ---- dsp_robust_scale_fit_batch
    EXPECT(dsp_robust_scale_fit_batch(nullptr, 4, 8, 3, nullptr, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), "NULL matrix d_X");
    EXPECT(dsp_robust_scale_fit_batch(reinterpret_cast<double*>(X1), 4, 8, 3, nullptr, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), "d_X must be 8-byte aligned");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 0, nullptr, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), "F 0 must be in [1, 16]");
    EXPECT(dsp_robust_scale_fit_batch(X, 17, 8, 17, nullptr, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), "F 17 must be in [1, 16]");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 0, 3, nullptr, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), "n 0 must be in [1, 8192]");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8193, 3, nullptr, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), "n 8193 must be in [1, 8192]");
    EXPECT(dsp_robust_scale_fit_batch(X, 2, 8, 3, nullptr, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), "ld 2 must be in");
    EXPECT(dsp_robust_scale_fit_batch(X, INT64_MAX, 8, 3, nullptr, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), "must be in [F = 3, 2^32]");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, valid, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), "ld_valid 0 must be in");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, reinterpret_cast<int32_t*>(reinterpret_cast<char*>(valid) + 2), 9, 25, 75, 0, out_scale, nullptr, info, nullptr), "d_valid must be 4-byte aligned");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, -1, 75, 0, out_scale, nullptr, info, nullptr), "the quantile pair");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 75, 25, 0, out_scale, nullptr, info, nullptr), "the quantile pair");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 25, 100.5, 0, out_scale, nullptr, info, nullptr), "the quantile pair");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, nan, 75, 0, out_scale, nullptr, info, nullptr), "the quantile pair");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 25, 75, 0, nullptr, nullptr, info, nullptr), "NULL output d_scale / d_info");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 25, 75, 0, out_scale, nullptr, nullptr, nullptr), "NULL output d_scale / d_info");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 25, 75, 1, out_scale, nullptr, info, nullptr), "NULL output d_center with centering");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 25, 75, 0, reinterpret_cast<double*>(reinterpret_cast<char*>(out_scale) + 4), nullptr, info, nullptr), "aligned to their element size");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 25, 75, 0, X + 30, nullptr, info, nullptr), "d_scale overlaps d_X");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, valid, 9, 25, 75, 0, out_scale, nullptr, valid + 63, nullptr), "d_info overlaps d_valid");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 25, 75, 1, out_scale, out_scale + 2, info, nullptr), "d_scale overlaps d_center");
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 25, 75, 0, out_scale, nullptr, info, nullptr), refused);
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, valid + 8, 9, 0, 100, 1, out_scale, out_center, info, nullptr), refused);
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 50, 50, 0, out_scale, out_scale, info, nullptr), refused);      // d_center unused without centering
    EXPECT(dsp_robust_scale_fit_batch(X, 4, 8, 3, nullptr, 0, 25, 75, 0, X + 31, nullptr, info, nullptr), refused);           // right behind the last row's features

    // ---- dsp_var_all
    EXPECT(dsp_var_all(nullptr, 4, 8, 3, nullptr, nullptr, nullptr, var, nullptr), "NULL matrix d_X");
    EXPECT(dsp_var_all(X, 4, 8, 3, nullptr, nullptr, nullptr, nullptr, nullptr), "NULL output d_out");
    EXPECT(dsp_var_all(X, 4, 0, 3, nullptr, nullptr, nullptr, var, nullptr), "n 0 must be in [1, 8192]");
    EXPECT(dsp_var_all(X, 4, 8, 17, nullptr, nullptr, nullptr, var, nullptr), "F 17 must be in [1, 16]");
    EXPECT(dsp_var_all(X, 1, 8, 3, nullptr, nullptr, nullptr, var, nullptr), "ld 1 must be in");
    EXPECT(dsp_var_all(X, 4, 8, 3, reinterpret_cast<double*>(reinterpret_cast<char*>(center) + 4), nullptr, nullptr, var, nullptr), "must be 8-byte aligned");
    EXPECT(dsp_var_all(X, 4, 8, 3, nullptr, nullptr, nullptr, X + 3, nullptr), "d_out overlaps d_X");
    EXPECT(dsp_var_all(X, 4, 8, 3, center, nullptr, nullptr, center + 1, nullptr), "d_out overlaps d_center");
    EXPECT(dsp_var_all(X, 4, 8, 3, nullptr, scale, nullptr, scale + 2, nullptr), "d_out overlaps d_scale");
    EXPECT(dsp_var_all(X, 4, 8, 3, nullptr, nullptr, reinterpret_cast<int8_t*>(var), var, nullptr), "d_out overlaps d_mask");
    EXPECT(dsp_var_all(X, 4, 8, 3, nullptr, nullptr, nullptr, var, nullptr), refused);
    EXPECT(dsp_var_all(X, 4, 8, 3, center, scale, mask, var, nullptr), refused);

    // ---- dsp_svm_fit_workspace_bytes
    if (dsp_svm_fit_workspace_bytes(8, 3, 2, &n) != DSP_OK || n != wb) { std::printf("workspace bytes %lld, expected %lld\n", (long long)n, (long long)wb); ++g_bad; }
    if (dsp_svm_fit_workspace_bytes(8192, 16, 65535, &n) != DSP_OK || n != (int64_t)8192 * 16 * 8 + (int64_t)65535 * 8192 * 4) { std::printf("workspace bytes %lld\n", (long long)n); ++g_bad; }
    EXPECT(dsp_svm_fit_workspace_bytes(8, 3, 2, nullptr), "NULL argument");
    EXPECT(dsp_svm_fit_workspace_bytes(1, 3, 2, &n), "n 1 must be in [2, 8192]");
    EXPECT(dsp_svm_fit_workspace_bytes(8193, 3, 2, &n), "n 8193 must be in [2, 8192]");
    EXPECT(dsp_svm_fit_workspace_bytes(8, 0, 2, &n), "F 0 must be in [1, 16]");
    EXPECT(dsp_svm_fit_workspace_bytes(8, 17, 2, &n), "F 17 must be in [1, 16]");
    EXPECT(dsp_svm_fit_workspace_bytes(8, 3, 0, &n), "P 0 must be in [1, 65535]");
    EXPECT(dsp_svm_fit_workspace_bytes(8, 3, 65536, &n), "P 65536 must be in [1, 65535]");

    // ---- dsp_svm_fit_batch
#define FIT(X_, ld_, n_, F_, ce_, sc_, Y_, ldy_, P_, C_, g_, tol_, it_, coef_, ldc_, rho_, info_, w_, wb_) \
    dsp_svm_fit_batch(X_, ld_, n_, F_, ce_, sc_, Y_, ldy_, P_, C_, g_, tol_, it_, coef_, ldc_, rho_, info_, w_, wb_, nullptr)
    EXPECT(FIT(X, 4, 1, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "n 1 must be in [2, 8192]");
    EXPECT(FIT(X, 4, 8, 17, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "F 17 must be in [1, 16]");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 0, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "P 0 must be in [1, 65535]");
    EXPECT(FIT(nullptr, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "NULL matrix d_X");
    EXPECT(FIT(X, 2, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "ld 2 must be in");
    EXPECT(FIT(X, 4, 8, 3, center, scale, nullptr, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "NULL labels d_Y / d_C / d_gamma");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, nullptr, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "NULL labels d_Y / d_C / d_gamma");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, nullptr, 1e-3, 100, coef, 8, rho, info, work, wb), "NULL labels d_Y / d_C / d_gamma");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 7, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "ld_y 7 must be in");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 0.0, 100, coef, 8, rho, info, work, wb), "tol must be finite and positive");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, nan, 100, coef, 8, rho, info, work, wb), "tol must be finite and positive");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, inf, 100, coef, 8, rho, info, work, wb), "tol must be finite and positive");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 0, coef, 8, rho, info, work, wb), "max_iter 0 must be in [1, 10000000]");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 10000001, coef, 8, rho, info, work, wb), "max_iter 10000001 must be in");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, nullptr, 8, rho, info, work, wb), "NULL output d_coef / d_rho / d_info");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, nullptr, info, work, wb), "NULL output d_coef / d_rho / d_info");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, nullptr, work, wb), "NULL output d_coef / d_rho / d_info");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 7, rho, info, work, wb), "ld_coef 7 must be in");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, nullptr, wb), "NULL workspace");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work + 8, wb), "the workspace must be 16-byte aligned");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, reinterpret_cast<double*>(reinterpret_cast<char*>(C) + 4), gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "aligned to its element size");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb - 1), "is short of");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, 0), "is short of");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, X + 16, 8, rho, info, work, wb), "d_coef overlaps d_X");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, C + 1, info, work, wb), "d_rho overlaps d_C");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, gamma, info, work, wb), "d_rho overlaps d_gamma");
    EXPECT(FIT(X, 4, 8, 3, center, scale, reinterpret_cast<int8_t*>(info), 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), "d_info overlaps d_Y");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, center + 2, info, work, wb), "d_rho overlaps d_center");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, scale + 1, info, work, wb), "d_rho overlaps d_scale");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, coef + 15, info, work, wb), "d_coef overlaps d_rho");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, reinterpret_cast<int32_t*>(work + 256), work, wb), "d_info overlaps the workspace");
    EXPECT(FIT(X, 4, 8, 3, center, scale, Y, 8, 2, C, gamma, 1e-3, 100, coef, 8, rho, info, work, wb), refused);
    EXPECT(FIT(X, 4, 8, 3, nullptr, nullptr, Y, 8, 1, C, gamma, 1e-6, 10000000, coef, 8, rho, info, work, wb + 16), refused);
    EXPECT(FIT(X, 3, 8, 3, nullptr, scale, Y, 8, 2, C, gamma, 1e-3, 1, coef, 8, rho, info, work, wb), refused);
#undef FIT

    dsp_debug_host_dry_run(0);
    return finish("asan_svmfit_args");
}
