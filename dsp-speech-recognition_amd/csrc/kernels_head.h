// The pieces between the encoders and the output layer of the classifier heads (rnn_clf.py:29-31, 52, 68-72, 107-115, 146)
// that need max(len0), with every length read from device memory: the row counts of a batch (head_lengths_kernel) and the
// average | max pooling over the padded rows (head_pool_kernel).  gfx950 / ROCm only.  No grid barrier, no flag, no atomic:
// the lengths kernel is ONE workgroup, the pooling combines the partial results of its waves in LDS in a fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rnn_common.h"

constexpr int HEAD_LEN_THREADS = 256;          // the one workgroup of head_lengths_kernel
constexpr int HEAD_POOL_WAVES = 4;             // the time axis of a column is split over this many waves
constexpr int HEAD_MAX_B = 65535;

// len0c[b] = clamp(len0[b], 1, T), len1[b] = ceil(len0c[b] / hir), info = (max len0c, ceil(max / hir), number of clamped
// entries, 0).  One workgroup: thread i takes b = i, i + 256, ..; integers, so the order of the reduction does not matter.
// len0c may be len0 itself (every entry is read and written by one thread).
__global__ __launch_bounds__(HEAD_LEN_THREADS) void head_lengths_kernel(const int32_t* len0, int B, int T, int hir, int32_t* len0c,
                                                                        int32_t* __restrict__ len1, int32_t* __restrict__ info) {
    __shared__ int32_t s_max[HEAD_LEN_THREADS / 64], s_bad[HEAD_LEN_THREADS / 64];
    const int tid = threadIdx.x;
    int mx = 1, bad = 0;
    for (int b = tid; b < B; b += HEAD_LEN_THREADS) {
        const int32_t v = len0[b];
        const int32_t c = min(max(v, 1), T);
        bad += (c != v) ? 1 : 0;
        mx = max(mx, c);
        len0c[b] = c;
        len1[b] = (c + hir - 1) / hir;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        mx = max(mx, __shfl_xor(mx, o, 64));
        bad += __shfl_xor(bad, o, 64);
    }
    if ((tid & 63) == 0) { s_max[tid >> 6] = mx; s_bad[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < HEAD_LEN_THREADS / 64; ++w) { mx = max(mx, s_max[w]); bad += s_bad[w]; }
        info[0] = mx;
        info[1] = (mx + hir - 1) / hir;
        info[2] = bad;
        info[3] = 0;
    }
}

// torch.max's rule: a NaN wins and stays.
__device__ __forceinline__ float head_max(float m, float v) { return (v > m || v != v) ? v : m; }

// Whether row `av` with value v replaces row `am` with value m as the row of the maximum: none yet (am < 0), a first NaN, a
// larger value, or the same value (or another NaN) at a smaller row.  av < 0 (a wave without rows) never replaces.
__device__ __forceinline__ bool head_arg_takes(float m, int am, float v, int av) {
    if (av < 0) return false;
    if (am < 0) return true;
    if (m != m) return v != v && av < am;
    return v != v || v > m || (v == m && av < am);
}

// y [T, B, H] -> feat[b, col_avg + h] = (sum_{t < len} y[t, b, h]) / len and feat[b, col_max + h] = max_{t < len} y[t, b, h],
// against 0 where len < rows (the zero rows pad_packed_sequence leaves behind a shorter utterance; they are not read).
// len = clamp(d_len[b], 1, T), rows = min(*d_rows, T) or T.  Workgroup (b, chunk): HEAD_POOL_WAVES waves, lane l of each
// owns the V adjacent columns h = (64 chunk + l) V .. + V - 1 (V = 4: one 16-byte load per row), wave w takes the rows
// t = w, w + HEAD_POOL_WAVES, ..; the partial sums and maxima meet in LDS and wave 0 combines them in the order w = 0, 1, ..
// ARG (dsp_head_pool_train_batch): arg[b, h] = the smallest t < len whose value the max column returned (the first NaN row if
// there is one), -1 where the padding's 0.0f won.  The sums and maxima are those of the plain instantiation, bit for bit.
template <int V, bool ARG = false>
__global__ __launch_bounds__(64 * HEAD_POOL_WAVES) void head_pool_kernel(const float* __restrict__ y, int T, int B, int H,
                                                                         const int32_t* __restrict__ d_len, const int32_t* __restrict__ d_rows,
                                                                         float* __restrict__ feat, int64_t ld_feat, int col_avg, int col_max,
                                                                         int32_t* __restrict__ arg = nullptr) {
    __shared__ float s_sum[HEAD_POOL_WAVES][64 * V], s_max[HEAD_POOL_WAVES][64 * V];
    __shared__ int32_t s_arg[ARG ? HEAD_POOL_WAVES : 1][64 * V];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x;
    const int h0 = (blockIdx.y * 64 + lane) * V;
    const int len = min(max(d_len[b], 1), T);
    const int rows = d_rows ? min(d_rows[0], T) : T;
    float sum[V], mx[V];
    int am[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { sum[e] = 0.f; mx[e] = -INFINITY; am[e] = -1; }
    if (h0 < H) {                                            // (V = 4: H is a multiple of 4, so h0 + 3 < H as well)
        const float* col = y + (int64_t)b * H + h0;
        const int64_t step = (int64_t)B * H;
#pragma unroll 4
        for (int t = w; t < len; t += HEAD_POOL_WAVES) {
            if constexpr (V == 4) {
                const hm_f32x4 v = *(const hm_gf4*)(col + t * step);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (ARG) am[e] = head_arg_takes(mx[e], am[e], v[e], t) ? t : am[e];
                    sum[e] += v[e]; mx[e] = head_max(mx[e], v[e]);
                }
            } else {
                const float v = col[t * step];
                if constexpr (ARG) am[0] = head_arg_takes(mx[0], am[0], v, t) ? t : am[0];
                sum[0] += v; mx[0] = head_max(mx[0], v);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        s_sum[w][lane * V + e] = sum[e]; s_max[w][lane * V + e] = mx[e];
        if constexpr (ARG) s_arg[w][lane * V + e] = am[e];
    }
    __syncthreads();
    if (w != 0 || h0 >= H) return;
    const float n = (float)len;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        float s = sum[e], m = mx[e];
        int a = am[e];
#pragma unroll
        for (int k = 1; k < HEAD_POOL_WAVES; ++k) {
            if constexpr (ARG) a = head_arg_takes(m, a, s_max[k][lane * V + e], s_arg[k][lane * V + e]) ? s_arg[k][lane * V + e] : a;
            s += s_sum[k][lane * V + e]; m = head_max(m, s_max[k][lane * V + e]);
        }
        if (len < rows) {
            if constexpr (ARG) a = (0.f > m) ? -1 : a;          // the padding wins only where it is LARGER: a tie goes to the active row
            m = head_max(m, 0.f);
        }
        float* row = feat + (int64_t)b * ld_feat;
        if (col_avg >= 0) row[col_avg + h0 + e] = s / n;
        row[col_max + h0 + e] = m;
        if constexpr (ARG) arg[(int64_t)b * H + h0 + e] = a;
    }
}

// The backward of head_pool_kernel, one streaming pass that writes every element of gy [T, B, H] once:
//   gy[t, b, h] = t < len ? (col_avg >= 0 ? g[b, col_avg + h] / (float)len : 0) + (arg[b, h] == t ? g[b, col_max + h] : 0) : 0
// (the gradient of a padding win, arg = -1, is dropped: those rows are constants of the encoders).  The mapping is the
// forward's: workgroup (b, chunk), lane l owns the V adjacent columns h = (64 chunk + l) V .., wave w writes the rows
// t = w, w + HEAD_POOL_WAVES, .. (V = 4: one 16-byte store per row).  The quotient is formed once per (b, h).
template <int V>
__global__ __launch_bounds__(64 * HEAD_POOL_WAVES) void head_pool_bwd_kernel(const float* __restrict__ g, int64_t ld_g, int col_avg, int col_max,
                                                                             const int32_t* __restrict__ d_len, const int32_t* __restrict__ arg,
                                                                             int T, int B, int H, float* __restrict__ gy) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x;
    const int h0 = (blockIdx.y * 64 + lane) * V;
    if (h0 >= H) return;                                     // (V = 4: H is a multiple of 4, so h0 + 3 < H as well)
    const int len = min(max(d_len[b], 1), T);
    const float n = (float)len;
    const float* row = g + (int64_t)b * ld_g;
    float q[V], gm[V];
    int a[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        q[e] = col_avg >= 0 ? row[col_avg + h0 + e] / n : 0.f;
        gm[e] = row[col_max + h0 + e];
        a[e] = arg[(int64_t)b * H + h0 + e];
    }
    float* col = gy + (int64_t)b * H + h0;
    const int64_t step = (int64_t)B * H;
#pragma unroll 4
    for (int t = w; t < T; t += HEAD_POOL_WAVES) {
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = t < len ? q[e] + (a[e] == t ? gm[e] : 0.f) : 0.f;
        if constexpr (V == 4) *(hm_gf4*)(col + t * step) = hm_f32x4{o[0], o[1], o[2], o[3]};
        else col[t * step] = o[0];
    }
}
