// The fitting entry points of libdsp_frontend.so (include/dsp_frontend.h: dsp_robust_scale_fit_batch, dsp_var_all,
// dsp_svm_fit_workspace_bytes, dsp_svm_fit_batch): argument checks and the launches of kernels_svmfit.h.  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_svmfit.h"

namespace {

int check_matrix(const char* who, const double* d_X, int64_t ld, int32_t n, int32_t n_min, int32_t F) {
    if (!d_X) return dsp_fail(DSP_EINVAL, "%s: NULL matrix d_X", who);
    if (!aligned(d_X, 8)) return dsp_fail(DSP_EINVAL, "%s: d_X must be 8-byte aligned", who);
    if (F < 1 || F > SVMFIT_MAX_FEATURES) return dsp_fail(DSP_EINVAL, "%s: F %d must be in [1, %d]", who, F, SVMFIT_MAX_FEATURES);
    if (n < n_min || n > SVMFIT_MAX_ROWS) return dsp_fail(DSP_EINVAL, "%s: n %d must be in [%d, %d]", who, n, n_min, SVMFIT_MAX_ROWS);
    if (ld < F || ld > ((int64_t)1 << 32)) return dsp_fail(DSP_EINVAL, "%s: ld %lld must be in [F = %d, 2^32]", who, (long long)ld, F);
    return DSP_OK;
}

int64_t matrix_bytes(int64_t ld, int32_t n, int32_t F) { return ((int64_t)(n - 1) * ld + F) * 8; }

int64_t fit_xs_bytes(int32_t n, int32_t F) { return ((int64_t)n * F * 8 + 255) / 256 * 256; }

int64_t fit_work_bytes(int32_t n, int32_t F, int32_t P) { return fit_xs_bytes(n, F) + (int64_t)P * n * 4; }

int check_fit_sizes(const char* who, int32_t n, int32_t F, int32_t P) {
    if (F < 1 || F > SVMFIT_MAX_FEATURES) return dsp_fail(DSP_EINVAL, "%s: F %d must be in [1, %d]", who, F, SVMFIT_MAX_FEATURES);
    if (n < 2 || n > SVMFIT_MAX_ROWS) return dsp_fail(DSP_EINVAL, "%s: n %d must be in [2, %d]", who, n, SVMFIT_MAX_ROWS);
    if (P < 1 || P > SVMFIT_MAX_PROBLEMS) return dsp_fail(DSP_EINVAL, "%s: P %d must be in [1, %d]", who, P, SVMFIT_MAX_PROBLEMS);
    return DSP_OK;
}

template <int RPT, int THREADS>
int launch_fit(const SvmFitParams& prm, int32_t P, hipStream_t st) {
    static size_t granted[DSP_MAX_DEVICES] = {};
    const size_t lds = svmfit_lds_bytes(prm.n);
    if (lds > 48 * 1024 && dsp_ensure_dynamic_lds(reinterpret_cast<const void*>(&svm_fit_kernel<RPT, THREADS>), lds, granted) != 0)
        return dsp_fail(DSP_EHIP, "dsp_svm_fit_batch: cannot raise the dynamic LDS limit to %zu bytes", lds);
    svm_fit_kernel<RPT, THREADS><<<P, THREADS, lds, st>>>(prm);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_robust_scale_fit_batch(const double* d_X, int64_t ld, int32_t n, int32_t F, const int32_t* d_valid, int64_t ld_valid,
                               double q_lo, double q_hi, int32_t with_centering, double* d_scale, double* d_center, int32_t* d_info,
                               void* stream) {
    const char* who = "dsp_robust_scale_fit_batch";
    if (int rc = check_matrix(who, d_X, ld, n, 1, F)) return rc;
    if (d_valid && (ld_valid < 1 || ld_valid > ((int64_t)1 << 32)))
        return dsp_fail(DSP_EINVAL, "%s: ld_valid %lld must be in [1, 2^32]", who, (long long)ld_valid);
    if (d_valid && !aligned(d_valid, 4)) return dsp_fail(DSP_EINVAL, "%s: d_valid must be 4-byte aligned", who);
    if (!(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 100.0))
        return dsp_fail(DSP_EINVAL, "%s: the quantile pair (%g, %g) must satisfy 0 <= lo <= hi <= 100", who, q_lo, q_hi);
    if (!d_scale || !d_info) return dsp_fail(DSP_EINVAL, "%s: NULL output d_scale / d_info", who);
    if (with_centering && !d_center) return dsp_fail(DSP_EINVAL, "%s: NULL output d_center with centering", who);
    if (!aligned(d_scale, 8) || (d_center && !aligned(d_center, 8)) || !aligned(d_info, 4))
        return dsp_fail(DSP_EINVAL, "%s: the outputs must be aligned to their element size", who);
    const Range outs[3] = {range_of(d_scale, F * 8), range_of(with_centering ? d_center : nullptr, F * 8), range_of(d_info, 8)};
    const char* out_names[3] = {"d_scale", "d_center", "d_info"};
    const Range ins[2] = {range_of(d_X, matrix_bytes(ld, n, F)), range_of(d_valid, d_valid ? ((int64_t)(n - 1) * ld_valid + 1) * 4 : 0)};
    const char* in_names[2] = {"d_X", "d_valid"};
    if (int rc = check_overlaps(who, outs, out_names, 3, ins, in_names, 2)) return rc;
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    int32_t npad = 2;
    while (npad < n) npad <<= 1;
    const int threads = npad >= 2048 ? 1024 : (npad >= 512 ? 256 : 64);
    static size_t granted[DSP_MAX_DEVICES] = {};
    const size_t lds = (size_t)npad * 8;
    if (lds > 48 * 1024 && dsp_ensure_dynamic_lds(reinterpret_cast<const void*>(&robust_scale_fit_kernel), lds, granted) != 0)
        return dsp_fail(DSP_EHIP, "%s: cannot raise the dynamic LDS limit to %zu bytes", who, lds);
    robust_scale_fit_kernel<<<F, threads, lds, (hipStream_t)stream>>>(d_X, ld, n, F, d_valid, d_valid ? ld_valid : 0, q_lo, q_hi,
                                                                      with_centering ? 1 : 0, npad, d_scale, d_center, d_info);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_var_all(const double* d_X, int64_t ld, int32_t n, int32_t F, const double* d_center, const double* d_scale,
                const int8_t* d_mask, double* d_out, void* stream) {
    const char* who = "dsp_var_all";
    if (int rc = check_matrix(who, d_X, ld, n, 1, F)) return rc;
    if (!d_out) return dsp_fail(DSP_EINVAL, "%s: NULL output d_out", who);
    if (!aligned(d_out, 8) || (d_center && !aligned(d_center, 8)) || (d_scale && !aligned(d_scale, 8)))
        return dsp_fail(DSP_EINVAL, "%s: every fp64 pointer must be 8-byte aligned", who);
    const Range outs[1] = {range_of(d_out, 16)};
    const char* out_names[1] = {"d_out"};
    const Range ins[4] = {range_of(d_X, matrix_bytes(ld, n, F)), range_of(d_center, F * 8), range_of(d_scale, F * 8), range_of(d_mask, n)};
    const char* in_names[4] = {"d_X", "d_center", "d_scale", "d_mask"};
    if (int rc = check_overlaps(who, outs, out_names, 1, ins, in_names, 4)) return rc;
    if (int rc = dsp_refuse_dry_run(who)) return rc;
    svmfit_var_all_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(d_X, ld, n, F, d_center, d_scale, d_mask, d_out);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_svm_fit_workspace_bytes(int32_t n, int32_t F, int32_t P, int64_t* out_bytes) {
    const char* who = "dsp_svm_fit_workspace_bytes";
    if (!out_bytes) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = check_fit_sizes(who, n, F, P)) return rc;
    *out_bytes = fit_work_bytes(n, F, P);
    return DSP_OK;
}

int dsp_svm_fit_batch(const double* d_X, int64_t ld, int32_t n, int32_t F, const double* d_center, const double* d_scale,
                      const int8_t* d_Y, int64_t ld_y, int32_t P, const double* d_C, const double* d_gamma, double tol,
                      int32_t max_iter, double* d_coef, int64_t ld_coef, double* d_rho, int32_t* d_info, void* d_work,
                      int64_t work_bytes, void* stream) {
    const char* who = "dsp_svm_fit_batch";
    if (int rc = check_fit_sizes(who, n, F, P)) return rc;
    if (int rc = check_matrix(who, d_X, ld, n, 2, F)) return rc;
    if (!d_Y || !d_C || !d_gamma) return dsp_fail(DSP_EINVAL, "%s: NULL labels d_Y / d_C / d_gamma", who);
    if (ld_y < n || ld_y > ((int64_t)1 << 32)) return dsp_fail(DSP_EINVAL, "%s: ld_y %lld must be in [n = %d, 2^32]", who, (long long)ld_y, n);
    if (!(std::isfinite(tol) && tol > 0.0)) return dsp_fail(DSP_EINVAL, "%s: tol must be finite and positive", who);
    if (max_iter < 1 || max_iter > 10000000) return dsp_fail(DSP_EINVAL, "%s: max_iter %d must be in [1, 10000000]", who, max_iter);
    if (!d_coef || !d_rho || !d_info) return dsp_fail(DSP_EINVAL, "%s: NULL output d_coef / d_rho / d_info", who);
    if (ld_coef < n || ld_coef > ((int64_t)1 << 32))
        return dsp_fail(DSP_EINVAL, "%s: ld_coef %lld must be in [n = %d, 2^32]", who, (long long)ld_coef, n);
    if (!d_work) return dsp_fail(DSP_EINVAL, "%s: NULL workspace", who);
    if (!aligned(d_work, 16)) return dsp_fail(DSP_EINVAL, "%s: the workspace must be 16-byte aligned", who);
    if (!aligned(d_C, 8) || !aligned(d_gamma, 8) || !aligned(d_coef, 8) || !aligned(d_rho, 8) || !aligned(d_info, 4) ||
        (d_center && !aligned(d_center, 8)) || (d_scale && !aligned(d_scale, 8)))
        return dsp_fail(DSP_EINVAL, "%s: every pointer must be aligned to its element size", who);
    const int64_t need = fit_work_bytes(n, F, P);
    if (work_bytes < need)
        return dsp_fail(DSP_EINVAL, "%s: workspace of %lld bytes is short of the %lld dsp_svm_fit_workspace_bytes asks for", who,
                        (long long)work_bytes, (long long)need);
    const Range outs[4] = {range_of(d_coef, ((int64_t)(P - 1) * ld_coef + n) * 8), range_of(d_rho, (int64_t)P * 8),
                           range_of(d_info, (int64_t)P * 20), range_of(d_work, need)};
    const char* out_names[4] = {"d_coef", "d_rho", "d_info", "the workspace"};
    const Range ins[6] = {range_of(d_X, matrix_bytes(ld, n, F)), range_of(d_Y, (int64_t)(P - 1) * ld_y + n), range_of(d_C, (int64_t)P * 8),
                          range_of(d_gamma, (int64_t)P * 8), range_of(d_center, F * 8), range_of(d_scale, F * 8)};
    const char* in_names[6] = {"d_X", "d_Y", "d_C", "d_gamma", "d_center", "d_scale"};
    if (int rc = check_overlaps(who, outs, out_names, 4, ins, in_names, 6)) return rc;
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    hipStream_t st = (hipStream_t)stream;
    double* xs = static_cast<double*>(d_work);
    svmfit_scale_rows_kernel<<<(n * F + 255) / 256, 256, 0, st>>>(d_X, ld, n, F, d_center, d_scale, xs);
    HIP_TRY(hipGetLastError());
    SvmFitParams prm;
    prm.xs = xs;
    prm.Y = d_Y; prm.ld_y = ld_y;
    prm.C = d_C; prm.gamma = d_gamma;
    prm.tol = tol; prm.max_iter = max_iter; prm.n = n; prm.F = F;
    prm.idx = reinterpret_cast<int32_t*>(static_cast<char*>(d_work) + fit_xs_bytes(n, F));
    prm.coef = d_coef; prm.ld_coef = ld_coef; prm.rho = d_rho; prm.info = d_info;
    // the workgroup by the row count, the upper bound of a problem's active count (which only the device knows):
    // rows per thread x threads >= n
    if (n <= 64) return launch_fit<1, 64>(prm, P, st);
    if (n <= 128) return launch_fit<1, 128>(prm, P, st);
    if (n <= 512) return launch_fit<2, 256>(prm, P, st);
    if (n <= 2048) return launch_fit<4, 512>(prm, P, st);
    return launch_fit<8, 1024>(prm, P, st);
}

}  // extern "C"
