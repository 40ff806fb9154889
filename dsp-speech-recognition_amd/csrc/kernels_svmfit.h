// Fitting the pitch model on the device (pitch_model.py:48-50: scaler.fit, scaler.transform, clf.fit): the quantile scaler
// (RobustScaler.fit as NumPy's nanpercentile / nanmedian compute it), the variance behind SVC's gamma='scale', and the
// two-class C-SVC dual by sequential minimal optimisation (libsvm's Solver without shrinking and without a kernel cache),
// one workgroup per problem, many problems per launch.  Everything is fp64.  No atomics, no memset, no communication between
// workgroups: every reduction is a fixed tree whose result does not depend on the workgroup size, so a run is reproducible
// bit for bit.  gfx950 only (wave64).
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "dsp_common.h"

#define SVMFIT_MAX_FEATURES 16
#define SVMFIT_MAX_ROWS 8192
#define SVMFIT_MAX_PROBLEMS 65535
#define SVMFIT_MAX_WAVES 16
#define SVMFIT_TAU 1e-12           // libsvm's TAU: the curvature of a pair of identical rows

// status words of d_info
#define SVMFIT_OK 0
#define SVMFIT_MAX_ITER 1
#define SVMFIT_NONFINITE 2
#define SVMFIT_ONE_CLASS 3
#define SVMFIT_BAD_HYPER 4         // C or gamma of the problem is not finite and positive (they live on the device)
#define SCALEFIT_NO_ROWS 1         // the scaler: no valid row

// A rounded intermediate the backend cannot fuse into the operation behind it (the build contracts a * b + c otherwise).
__device__ __forceinline__ double svmfit_rounded(double v) {
    asm volatile("" : "+v"(v));
    return v;
}

// Sums of three counters over the workgroup (integer: the order does not matter).  Two barriers.
__device__ __forceinline__ void svmfit_block_sum3(int& a, int& b, int& c, int* scratch /* [3 * SVMFIT_MAX_WAVES] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    __syncthreads();                                   // the scratch may still be read from a call before
    if (lane == 0) {
        scratch[3 * wave] = a;
        scratch[3 * wave + 1] = b;
        scratch[3 * wave + 2] = c;
    }
    __syncthreads();
    a = b = c = 0;
    for (int w = 0; w < nw; ++w) {
        a += scratch[3 * w];
        b += scratch[3 * w + 1];
        c += scratch[3 * w + 2];
    }
}

// ---- RobustScaler.fit ------------------------------------------------------------------------------------------------

// np.percentile(sorted[0:m], q) with method='linear' as NumPy 2.x rounds it: the virtual index (m q + (1 - q)) - 1 with
// q = percent / 100, and the two-sided lerp  a + (b - a) t  for t < 0.5,  b - (b - a)(1 - t)  otherwise.
__device__ __forceinline__ double svmfit_percentile(const double* sorted, int m, double percent) {
    const double q = percent / 100.0;
    const double vi = (svmfit_rounded((double)m * q) + (1.0 - q)) - 1.0;
    if (vi >= (double)(m - 1)) return sorted[m - 1];
    if (vi < 0.0) return sorted[0];
    const double fl = floor(vi);
    const int k = (int)fl;
    const double a = sorted[k], b = sorted[k + 1], t = vi - fl, d = b - a;
    if (t >= 0.5) return b - svmfit_rounded(d * (1.0 - t));
    return a + svmfit_rounded(d * t);
}

// One workgroup per feature: the valid rows' values of column blockIdx.x sorted in LDS (a bitonic network over npad, a
// power of two; the tail is +inf), then the two percentiles and, when centring, the median ((a + b) / 2 of the two middle
// values, as nanmedian takes it).  Every workgroup looks at every feature of the valid rows, so all of them agree on the
// status without talking to each other: with a non-finite value in a valid row nothing but d_info is written.
__global__ __launch_bounds__(1024) void robust_scale_fit_kernel(const double* __restrict__ X, int64_t ld, int32_t n, int32_t F,
                                                                const int32_t* __restrict__ valid, int64_t ld_valid, double q_lo,
                                                                double q_hi, int32_t centering, int32_t npad,
                                                                double* __restrict__ scale, double* __restrict__ center,
                                                                int32_t* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double rs_sorted[];
    __shared__ int rs_scratch[3 * SVMFIT_MAX_WAVES];
    const int f = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    int cnt = 0, bad = 0, unused = 0;
    for (int r = tid; r < npad; r += T) {
        double v = INFINITY;
        if (r < n && (valid == nullptr || valid[(int64_t)r * ld_valid] != 0)) {
            const double* row = X + (int64_t)r * ld;
            for (int k = 0; k < F; ++k)
                if (!isfinite(row[k])) bad = 1;
            v = row[f];
            if (!isfinite(v)) v = INFINITY;
            ++cnt;
        }
        rs_sorted[r] = v;
    }
    svmfit_block_sum3(cnt, bad, unused, rs_scratch);
    const int status = bad ? SVMFIT_NONFINITE : (cnt < 1 ? SCALEFIT_NO_ROWS : SVMFIT_OK);
    if (f == 0 && tid == 0) {
        info[0] = cnt;
        info[1] = status;
    }
    if (status != SVMFIT_OK) return;                      // the whole workgroup, and every workgroup
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = tid; i < npad; i += T) {
                const int p = i ^ j;
                if (p > i) {
                    const double a = rs_sorted[i], b = rs_sorted[p];
                    if ((a > b) == ((i & k) == 0)) {
                        rs_sorted[i] = b;
                        rs_sorted[p] = a;
                    }
                }
            }
        }
    __syncthreads();
    if (tid == 0) {
        double s = svmfit_percentile(rs_sorted, cnt, q_hi) - svmfit_percentile(rs_sorted, cnt, q_lo);
        if (s < 10.0 * DBL_EPSILON) s = 1.0;               // sklearn's _handle_zeros_in_scale
        scale[f] = s;
        if (centering) center[f] = (rs_sorted[(cnt - 1) >> 1] + rs_sorted[cnt >> 1]) / 2.0;
    }
}

// ---- the scaled matrix and its variance ------------------------------------------------------------------------------

// xs[r, f] = (X[r, f] - center[f]) / scale[f]: a true division, as RobustScaler.transform and svm_decision_wave.
__global__ __launch_bounds__(256) void svmfit_scale_rows_kernel(const double* __restrict__ X, int64_t ld, int32_t n, int32_t F,
                                                                const double* __restrict__ center, const double* __restrict__ scale,
                                                                double* __restrict__ xs) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * F) return;
    const int r = e / F, f = e - r * F;
    const double c = center ? center[f] : 0.0, s = scale ? scale[f] : 1.0;
    xs[e] = (X[(int64_t)r * ld + f] - c) / s;
}

// Sum of one double per thread over the workgroup: the butterfly in each wave, then the waves in index order.
__device__ __forceinline__ double svmfit_block_sum(double v, double* scratch /* [SVMFIT_MAX_WAVES] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += scratch[w];
    return s;
}

// np.var of every entry of the scaled rows the mask keeps (NULL: all), two passes: out[0] = mean((v - mean(v))^2),
// out[1] = the number of entries.  One workgroup of 1024 threads, a fixed order.
__global__ __launch_bounds__(1024) void svmfit_var_all_kernel(const double* __restrict__ X, int64_t ld, int32_t n, int32_t F,
                                                              const double* __restrict__ center, const double* __restrict__ scale,
                                                              const int8_t* __restrict__ mask, double* __restrict__ out) {
    __shared__ double va_scratch[SVMFIT_MAX_WAVES];
    __shared__ int va_iscratch[3 * SVMFIT_MAX_WAVES];
    const int tid = threadIdx.x, total = n * F;
    int cnt = 0, u0 = 0, u1 = 0;
    double s = 0.0;
    for (int e = tid; e < total; e += 1024) {
        const int r = e / F, f = e - r * F;
        if (mask == nullptr || mask[r] != 0) {
            s += (X[(int64_t)r * ld + f] - (center ? center[f] : 0.0)) / (scale ? scale[f] : 1.0);
            ++cnt;
        }
    }
    svmfit_block_sum3(cnt, u0, u1, va_iscratch);
    const double mean = svmfit_block_sum(s, va_scratch) / (double)cnt;
    double q = 0.0;
    for (int e = tid; e < total; e += 1024) {
        const int r = e / F, f = e - r * F;
        if (mask == nullptr || mask[r] != 0) {
            const double d = (X[(int64_t)r * ld + f] - (center ? center[f] : 0.0)) / (scale ? scale[f] : 1.0) - mean;
            q = fma(d, d, q);
        }
    }
    q = svmfit_block_sum(q, va_scratch);
    if (tid == 0) {
        out[0] = q / (double)cnt;
        out[1] = (double)cnt;
    }
}

// ---- the solver ------------------------------------------------------------------------------------------------------

struct SvmFitParams {
    const double* xs;          // [n, F] the scaled rows (workspace)
    const int8_t* Y;           // [P, ld_y]  -1 / 0 / +1; 0 = the row is not in the problem
    int64_t ld_y;
    const double* C;           // [P]
    const double* gamma;       // [P]
    double tol;
    int32_t max_iter, n, F;
    int32_t* idx;              // [P, n] the rows of each problem, ascending (workspace)
    double* coef;              // [P, ld_coef]
    int64_t ld_coef;
    double* rho;               // [P]
    int32_t* info;             // [P, 5]  n_iter, status, n_sv, n_bounded, n_active
};

// exp(-gamma |a - b|^2) from the sum of squared differences, spelled as fma / single operations: the same bits wherever
// it is inlined.
__device__ __forceinline__ double svmfit_rbf(const double* __restrict__ a, const double* __restrict__ b, int F, double neg_gamma) {
    double d2 = 0.0;
#pragma unroll 4
    for (int f = 0; f < F; ++f) {
        const double d = a[f] - b[f];
        d2 = fma(d, d, d2);
    }
    return exp(neg_gamma * d2);
}

struct SvmFitPick {            // what a wave hands to the workgroup after an arg-reduction
    double v, alpha, g, other;
    int idx, pad;
};

// Bytes of dynamic LDS: alpha [cap] | G [cap] | y [cap] (int8), cap = n rounded up to 16.
__host__ __device__ inline size_t svmfit_lds_bytes(int32_t n) { return (size_t)((n + 15) / 16 * 16) * 17; }

// One workgroup per problem; thread `tid` owns the positions tid + k blockDim.x, k < RPT, of the problem's row list.  alpha,
// G and the labels stay in LDS, row i of the kernel matrix in registers (RPT values per thread), row j is used as it is made.
// Per iteration two barriers: the winner of each arg-reduction travels with its alpha and G (read by the leader of the wave
// that owns it, so nobody reads a value another wave is about to write), and every thread repeats the two-variable update on
// those values; the owners store the result.  Ties go to the lowest position whatever the workgroup size, sums that reach an
// output are taken over a fixed 64-lane partition: the bits do not depend on blockDim.x.
// THREADS is the workgroup size of the launch: each instantiation is compiled for its own, so only the 1024-thread one is
// held to 128 registers.
template <int RPT, int THREADS>
__global__ __launch_bounds__(THREADS) void svm_fit_kernel(SvmFitParams P) {
    extern __shared__ __attribute__((aligned(16))) double fit_smem[];
    __shared__ SvmFitPick s_a[SVMFIT_MAX_WAVES], s_b[SVMFIT_MAX_WAVES];
    __shared__ int s_cnt[3 * SVMFIT_MAX_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;
    const int n = P.n, F = P.F, cap = (n + 15) / 16 * 16;
    double* const alpha = fit_smem;
    double* const G = alpha + cap;
    int8_t* const ys = reinterpret_cast<int8_t*>(G + cap);
    const int8_t* const Yp = P.Y + (int64_t)p * P.ld_y;
    int32_t* const idx = P.idx + (int64_t)p * n;
    const double* const xs = P.xs;

    // the ascending list of the problem's rows; from here on everything is a position in it
    int base = 0, n_pos = 0, n_neg = 0, bad = 0;
    for (int r0 = 0; r0 < n; r0 += T) {
        const int r = r0 + tid;
        const int yv = r < n ? (int)Yp[r] : 0;
        const unsigned long long act = __ballot(yv != 0);
        if (lane == 0) s_cnt[wave] = __popcll(act);
        __syncthreads();
        int off = base, tot = 0;
        for (int w = 0; w < nw; ++w) {
            const int c = s_cnt[w];
            off += w < wave ? c : 0;
            tot += c;
        }
        if (yv != 0) {
            const int t = off + __popcll(act & ((1ull << lane) - 1ull));
            idx[t] = r;
            ys[t] = yv > 0 ? 1 : -1;
            alpha[t] = 0.0;
            G[t] = -1.0;
            if (yv > 0) ++n_pos; else ++n_neg;
            for (int f = 0; f < F; ++f)
                if (!isfinite(xs[(int64_t)r * F + f])) bad = 1;
        }
        base += tot;
        __syncthreads();
    }
    const int na = base;
    svmfit_block_sum3(n_pos, n_neg, bad, s_cnt);          // (its barriers also publish idx, ys, alpha, G)
    const double C = P.C[p], gamma = P.gamma[p], tol = P.tol;
    int status = SVMFIT_MAX_ITER;
    // (non-finite rows first: a gamma derived from them, 1 / (F var), is not finite either, and the rows are the cause)
    if (bad) status = SVMFIT_NONFINITE;
    else if (!(isfinite(C) && C > 0.0 && isfinite(gamma) && gamma > 0.0)) status = SVMFIT_BAD_HYPER;
    else if (n_pos < 1 || n_neg < 1) status = SVMFIT_ONE_CLASS;
    if (status != SVMFIT_MAX_ITER) {                      // workgroup-uniform; nothing but the info is written
        if (tid == 0) {
            int32_t* o = P.info + (int64_t)p * 5;
            o[0] = 0; o[1] = status; o[2] = 0; o[3] = 0; o[4] = na;
        }
        return;
    }
    const double neg_gamma = -gamma;
    const double* xrow[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int t = tid + k * T;
        xrow[k] = xs + (int64_t)(t < na ? idx[t] : 0) * F;
    }

    int iter = 0;
    while (iter < P.max_iter) {
        // 1. i = arg max of -y G over I_up (lowest position among equals), M = min of -y G over I_low
        double vmax = -INFINITY, vmin = INFINITY;
        int imax = -1;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int t = tid + k * T;
            if (t < na) {
                const double a = alpha[t], g = G[t];
                const bool pos = ys[t] > 0;
                const double v = pos ? -g : g;
                const bool up = pos ? a < C : a > 0.0, low = pos ? a > 0.0 : a < C;
                if (up && v > vmax) { vmax = v; imax = t; }
                if (low && v < vmin) vmin = v;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(vmax, o, 64);
            const int oi = __shfl_xor(imax, o, 64);
            if (ov > vmax || (ov == vmax && (unsigned)oi < (unsigned)imax)) { vmax = ov; imax = oi; }
            vmin = fmin(vmin, __shfl_xor(vmin, o, 64));
        }
        if (lane == 0) {
            s_a[wave].v = vmax;
            s_a[wave].idx = imax;
            s_a[wave].alpha = imax >= 0 ? alpha[imax] : 0.0;
            s_a[wave].other = vmin;
        }
        __syncthreads();
        double m = s_a[0].v, M = s_a[0].other, a_i = s_a[0].alpha;
        int i = s_a[0].idx;
        for (int w = 1; w < nw; ++w) {
            const double ov = s_a[w].v;
            const int oi = s_a[w].idx;
            if (ov > m || (ov == m && (unsigned)oi < (unsigned)i)) { m = ov; i = oi; a_i = s_a[w].alpha; }
            M = fmin(M, s_a[w].other);
        }
        if (i < 0 || m - M < tol) { status = SVMFIT_OK; break; }
        const int y_i = ys[i];
        const double g_i = y_i > 0 ? -m : m;
        const double* const xi = xs + (int64_t)idx[i] * F;

        // 2. row i of the kernel matrix, 3. j = arg min of -b^2 / a over I_low with b = m + y_t G_t > 0
        double Ki[RPT];
        double best = INFINITY;
        int jmin = -1;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int t = tid + k * T;
            Ki[k] = 0.0;
            if (t < na) {
                Ki[k] = svmfit_rbf(xi, xrow[k], F, neg_gamma);
                const double a = alpha[t], g = G[t];
                const bool pos = ys[t] > 0;
                const bool low = pos ? a > 0.0 : a < C;
                const double b = m - (pos ? -g : g);
                if (low && b > 0.0) {
                    double q = 2.0 - 2.0 * Ki[k];             // Q_ii + Q_tt - 2 y_i y_t Q_it (2 K is exact: one rounding)
                    if (q <= 0.0) q = SVMFIT_TAU;
                    const double obj = -(b * b) / q;
                    if (obj < best) { best = obj; jmin = t; }
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(jmin, o, 64);
            if (ov < best || (ov == best && (unsigned)oi < (unsigned)jmin)) { best = ov; jmin = oi; }
        }
        if (lane == 0) {
            s_b[wave].v = best;
            s_b[wave].idx = jmin;
            s_b[wave].alpha = jmin >= 0 ? alpha[jmin] : 0.0;
            s_b[wave].g = jmin >= 0 ? G[jmin] : 0.0;
        }
        __syncthreads();
        double bj = s_b[0].v, a_j = s_b[0].alpha, g_j = s_b[0].g;
        int j = s_b[0].idx;
        for (int w = 1; w < nw; ++w) {
            const double ov = s_b[w].v;
            const int oi = s_b[w].idx;
            if (ov < bj || (ov == bj && (unsigned)oi < (unsigned)j)) { bj = ov; j = oi; a_j = s_b[w].alpha; g_j = s_b[w].g; }
        }
        if (j < 0) { status = SVMFIT_OK; break; }
        const int y_j = ys[j];
        const double* const xj = xs + (int64_t)idx[j] * F;

        // 5. libsvm's two-variable update (C_i = C_j = C, Q_ii = Q_jj = 1), by every thread on the same values
        double quad = 2.0 - 2.0 * svmfit_rbf(xi, xj, F, neg_gamma);
        if (quad <= 0.0) quad = SVMFIT_TAU;
        double n_i = a_i, n_j = a_j;
        if (y_i != y_j) {
            const double delta = (-g_i - g_j) / quad, diff = a_i - a_j;
            n_i += delta;
            n_j += delta;
            if (diff > 0.0) {
                if (n_j < 0.0) { n_j = 0.0; n_i = diff; }
            } else {
                if (n_i < 0.0) { n_i = 0.0; n_j = -diff; }
            }
            if (diff > 0.0) {                                   // C_i - C_j = 0
                if (n_i > C) { n_i = C; n_j = C - diff; }
            } else {
                if (n_j > C) { n_j = C; n_i = C + diff; }
            }
        } else {
            const double delta = (g_i - g_j) / quad, sum = a_i + a_j;
            n_i -= delta;
            n_j += delta;
            if (sum > C) {
                if (n_i > C) { n_i = C; n_j = sum - C; }
            } else {
                if (n_j < 0.0) { n_j = 0.0; n_i = sum; }
            }
            if (sum > C) {
                if (n_j > C) { n_j = C; n_i = sum - C; }
            } else {
                if (n_i < 0.0) { n_i = 0.0; n_j = sum; }
            }
        }
        const double d_i = n_i - a_i, d_j = n_j - a_j;

        // 4. + 6. row j as it is made: G += Q_i d_i + Q_j d_j
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int t = tid + k * T;
            if (t < na) {
                const int y_t = ys[t];
                const double kj = svmfit_rbf(xj, xrow[k], F, neg_gamma);
                const double q_i = y_i == y_t ? Ki[k] : -Ki[k], q_j = y_j == y_t ? kj : -kj;
                G[t] = fma(q_j, d_j, fma(q_i, d_i, G[t]));
                if (t == i) alpha[t] = n_i;
                if (t == j) alpha[t] = n_j;
            }
        }
        ++iter;
    }
    __syncthreads();

    // libsvm's calculate_rho and the counts, by wave 0 over the fixed partition lane, lane + 64, ...
    if (wave == 0) {
        double ub = INFINITY, lb = -INFINITY, sum_free = 0.0;
        int n_free = 0, n_sv = 0, n_bounded = 0;
        for (int t = lane; t < na; t += 64) {
            const double a = alpha[t];
            const bool pos = ys[t] > 0;
            const double yg = pos ? G[t] : -G[t];
            if (a > 0.0) ++n_sv;
            if (a >= C) {
                ++n_bounded;
                if (pos) lb = fmax(lb, yg); else ub = fmin(ub, yg);
            } else if (a <= 0.0) {
                if (pos) ub = fmin(ub, yg); else lb = fmax(lb, yg);
            } else {
                ++n_free;
                sum_free += yg;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ub = fmin(ub, __shfl_xor(ub, o, 64));
            lb = fmax(lb, __shfl_xor(lb, o, 64));
            sum_free += __shfl_xor(sum_free, o, 64);
            n_free += __shfl_xor(n_free, o, 64);
            n_sv += __shfl_xor(n_sv, o, 64);
            n_bounded += __shfl_xor(n_bounded, o, 64);
        }
        if (lane == 0) {
            P.rho[p] = n_free > 0 ? sum_free / (double)n_free : (ub + lb) / 2.0;
            int32_t* o = P.info + (int64_t)p * 5;
            o[0] = iter; o[1] = status; o[2] = n_sv; o[3] = n_bounded; o[4] = na;
        }
    }
    double* const coef = P.coef + (int64_t)p * P.ld_coef;
    for (int r = tid; r < n; r += T)
        if (Yp[r] == 0) coef[r] = 0.0;
    for (int t = tid; t < na; t += T) {
        const double a = alpha[t];
        coef[idx[t]] = a > 0.0 ? (ys[t] > 0 ? a : -a) : 0.0;
    }
}
