// The attention blocks of the classifiers, forward (the gradients: kernels_attn_bwd.h), fp32, on v_mfma_f32_16x16x4_f32:
//   * the Transformer encoder block in front of rnn_clf.Transformer (transformer.py:16-140, layers.py:125-143) as three launches
//     -- projection, batch-softmax statistics, output -- none of which holds a [B, T, T] tensor;
//   * layers.SelfAttn (layers.py:78-95), the pooling of rnn_clf.HRNN_Att, as one launch.
//
// The block's algebra.  With x_b [T, d] the rows of utterance b, n_head = 1 and temper = sqrt(d):
//   s[b,t,u] = tanh(x_b[t] W_q) . (x_b[u] W_k) / temper  =  q'[b,t] . x_b[u],    q'[b,t] = (tanh(x_b[t] W_q) W_k^T) / temper
//   o[b,t]   = sum_u a[b,t,u] (x_b[u] W_v)               =  (sum_u a[b,t,u] x_b[u]) W_v
// so keys and values are never stored: the score product and the weighted sum both run over the d <= 64 columns of x itself
// (d_k, d_v are 100 in the shipped head).  The workspace holds x and q' as zero-padded [B, TP, DP] copies (TP = T rounded up
// to 16 rows, DP = d rounded up to 16 columns: every operand is an aligned float4 and no launch needs a bounds test on a load)
// and the two [TP, TP] statistics  smax[t,u] = max_b s[b,t,u],  ssum[t,u] = sum_b exp(s[b,t,u] - smax[t,u]).
//
// Operand layout of one 16x16x4 product step e of k-group g (shared with rnn_common.h): lane l supplies A[l & 15][k] and
// B[k][l & 15] with k = 16 g + 4 (l >> 4) + e, i.e. one float4 per lane and k-group from a row-major operand, and receives
// D[4 (l >> 4) + r][l & 15], r = 0..3.  The score tile is computed TRANSPOSED (D[u][t]): its registers are then exactly the
// B operand (k = u, n = t) of the weighted sum, computed transposed as well, and no shuffle or LDS trip lies between them.
//
// Every reduction runs in a fixed order (b ascending per wave, waves combined in order; u ascending), without atomics: the
// same arguments give the same bits.  Every loop is bounded by an argument; no workgroup waits on another one.
#pragma once

#include <math.h>

#include "dsp_common.h"
#include "rnn_common.h"

#define AT_MAX_D 64           // d_model
#define AT_MAX_DKV 128        // d_k, d_v
#define AT_MAX_INNER 256      // d_inner
#define AT_MAX_T 1024
#define AT_MAX_H 256          // pooling width
#define AT_SA (AT_MAX_D + 4)          // LDS row strides: + 4 floats, so that the 16 rows of a float4 column do not share banks
#define AT_SB (AT_MAX_INNER + 4)
#define AT_SK (AT_MAX_DKV + 4)
#define AT_STAT_WAVES 8       // waves of a statistics workgroup: each takes a contiguous range of b

static inline int32_t at_pad16(int32_t v) { return (v + 15) & ~15; }

// Packed parameters of one encoder block.  Matrices are [K][N] products stored as float4 [ng][nt][64] (k-group, N tile, lane),
// zero beyond K and N; vectors are padded with zeros to whole tiles.
struct AttnWeights {
    const float4* wq;      // [d][d_k]       x -> q
    const float4* wkt;     // [d_k][d]       tanh(q) -> q' (in front of the temperature)
    const float4* wv;      // [d][d_v]       sum_u a x_u -> o
    const float4* wpt;     // [d_v][d]       proj.weight^T
    const float4* w1t;     // [d][d_inner]   pos_ffn.w_1.weight^T
    const float4* w2t;     // [d_inner][d]   pos_ffn.w_2.weight^T
    const float *ln1a, *ln1b, *pb, *b1, *b2, *ln2a, *ln2b;
    int32_t d, ngd, ngk, ngv, ngi;      // d_model and the 16-groups of d, d_k, d_v, d_inner
    float eps, inv_temper;
};

struct AttnParams {
    AttnWeights w;
    int32_t T, TP, B;
    const float* x;        // [T, B, d]
    float* y;              // [T, B, d]
    float* xp;             // workspace: [B, TP, DP]
    float* qp;             //            [B, TP, DP]
    float* smax;           //            [TP, TP]
    float* ssum;           //            [TP, TP]
    float* msave;          // training: [B, TP, DP], the weighted sums M in front of W_v (kernels_attn_bwd.h); NULL otherwise
};

__device__ __forceinline__ hm_f32x4 at_mfma4(hm_f32x4 acc, const hm_f32x4 a, const hm_f32x4 b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// out[16 rows][16 nt] = in[16 rows][16 ng] x packed [ng][nt]: the wave's 16 rows, row-major in LDS (stride a multiple of 4
// floats), through one dense layer.  Four N tiles share one read of the LDS operand; behind the last tile the index is clamped
// (a product computed twice, nothing read past the matrix).  epi(tile, acc) receives D[4 (l >> 4) + r][16 tile + (l & 15)].
template <class Epi>
__device__ __forceinline__ void at_dense(const float* in, int stride, const float4* __restrict__ wp, int ng, int nt, int lane, Epi&& epi) {
    const hm_lf4* a4 = (const hm_lf4*)(in + (lane & 15) * stride + 4 * (lane >> 4));
    const hm_gf4* w4 = (const hm_gf4*)wp + lane;
    for (int t0 = 0; t0 < nt; t0 += 4) {
        hm_f32x4 acc[4];
        int ti[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { acc[i] = hm_f32x4{0.f, 0.f, 0.f, 0.f}; ti[i] = min(t0 + i, nt - 1); }
        for (int g = 0; g < ng; ++g) {
            const hm_f32x4 a = a4[4 * g];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = at_mfma4(acc[i], a, w4[(size_t)(g * nt + ti[i]) * 64]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (t0 + i < nt) epi(t0 + i, acc[i]);
    }
}

// layers.LayerNormalization over the d columns of the wave's 16 rows in LDS: four lanes per row, unbiased sigma, eps added to it.
__device__ __forceinline__ void at_layer_norm(float* buf, int stride, int d, const float* __restrict__ a2, const float* __restrict__ b2,
                                              float eps, int lane) {
    float* row = buf + (lane >> 2) * stride;
    const int q = lane & 3;
    float s = 0.f;
    for (int j = q; j < d; j += 4) s += row[j];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    const float mu = s / (float)d;
    float v = 0.f;
    for (int j = q; j < d; j += 4) { const float c = row[j] - mu; v += c * c; }
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    const float sigma = sqrtf(v / (float)(d - 1));          // d = 1: 0 / 0, not a number, as torch.std gives
    const float inv = 1.0f / (sigma + eps);
    for (int j = q; j < d; j += 4) row[j] = (row[j] - mu) * inv * a2[j] + b2[j];
}

// Launch 1: one wave per (utterance, 16 rows).  Writes the padded copy of x and q' = tanh(x W_q) W_k^T / temper.
__global__ __launch_bounds__(64) void attn_proj_kernel(const AttnParams P) {
    __shared__ __attribute__((aligned(16))) float xs[16 * AT_SA];
    __shared__ __attribute__((aligned(16))) float tq[16 * AT_SK];
    const AttnWeights& W = P.w;
    const int lane = threadIdx.x, tiles = P.TP >> 4;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) << 4;
    const int d = W.d, DP = W.ngd << 4;
    float* xp = P.xp + ((int64_t)b * P.TP + t0) * DP;
    float* qp = P.qp + ((int64_t)b * P.TP + t0) * DP;
    for (int idx = lane; idx < 16 * DP; idx += 64) {
        const int r = idx / DP, j = idx - r * DP, t = t0 + r;
        const float v = (t < P.T && j < d) ? P.x[((int64_t)t * P.B + b) * d + j] : 0.f;
        xs[r * AT_SA + j] = v;
        xp[idx] = v;
    }
    __syncthreads();
    const int r0 = 4 * (lane >> 4), c0 = lane & 15;
    at_dense(xs, AT_SA, W.wq, W.ngd, W.ngk, lane, [&](int t, const hm_f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) tq[(r0 + r) * AT_SK + 16 * t + c0] = tanhf(acc[r]);
    });
    __syncthreads();
    at_dense(tq, AT_SK, W.wkt, W.ngk, W.ngd, lane, [&](int t, const hm_f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) qp[(r0 + r) * DP + 16 * t + c0] = acc[r] * W.inv_temper;
    });
}

// The transposed 16 x 16 score tile of utterance b: D[u][t] = x_b[u0 + .] . q'[b, t0 + .].  xrow / qrow: the lane's float4
// column (l >> 4) of row u0 + (l & 15) of xp and of row t0 + (l & 15) of qp.
__device__ __forceinline__ hm_f32x4 at_scores(const hm_gf4* xrow, const hm_gf4* qrow, int ngd) {
    hm_f32x4 acc = hm_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < ngd; ++g) acc = at_mfma4(acc, xrow[4 * g], qrow[4 * g]);
    return acc;
}

// Launch 2: a workgroup per (u tile, t tile); wave w walks its range of b in ascending order with a running maximum and a
// rescaled sum, then wave 0 combines the eight partial results in order.
__global__ __launch_bounds__(AT_STAT_WAVES * 64) void attn_stats_kernel(const AttnParams P) {
    __shared__ float sm[AT_STAT_WAVES][4][64], sz[AT_STAT_WAVES][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.x << 4, t0 = blockIdx.y << 4;
    const int ngd = P.w.ngd, DP = ngd << 4;
    const int chunk = (P.B + AT_STAT_WAVES - 1) / AT_STAT_WAVES;
    const int b_lo = w * chunk, b_hi = min(P.B, b_lo + chunk);
    const int64_t per_b = (int64_t)P.TP * DP;
    const int64_t xoff = (int64_t)(u0 + (lane & 15)) * DP + 4 * (lane >> 4), qoff = (int64_t)(t0 + (lane & 15)) * DP + 4 * (lane >> 4);
    float m[4], z[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; z[r] = 0.f; }
    for (int b = b_lo; b < b_hi; ++b) {
        const hm_f32x4 s = at_scores((const hm_gf4*)(P.xp + b * per_b + xoff), (const hm_gf4*)(P.qp + b * per_b + qoff), ngd);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float mn = fmaxf(m[r], s[r]);
            z[r] = z[r] * expf(m[r] - mn) + expf(s[r] - mn);       // (the first b: 0 * exp(-inf) + 1)
            m[r] = mn;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { sm[w][r][lane] = m[r]; sz[w][r][lane] = z[r]; }
    __syncthreads();
    if (w != 0) return;
    hm_f32x4 mo, zo;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float mm = sm[0][r][lane];
        for (int k = 1; k < AT_STAT_WAVES; ++k) mm = fmaxf(mm, sm[k][r][lane]);
        float zz = 0.f;
        for (int k = 0; k < AT_STAT_WAVES; ++k) zz += sz[k][r][lane] * expf(sm[k][r][lane] - mm);   // an empty range: 0 * exp(-inf)
        mo[r] = mm; zo[r] = zz;
    }
    const int64_t so = (int64_t)(t0 + (lane & 15)) * P.TP + u0 + 4 * (lane >> 4);     // [t][u .. u + 3]
    *(hm_gf4*)(P.smax + so) = mo;
    *(hm_gf4*)(P.ssum + so) = zo;
}

// Launch 3: one wave per (utterance, 16 rows): the scores again, normalised with the statistics, times x; then the row is
// finished in LDS: W_v, proj + residual + LN1, FFN + residual + LN2.
__global__ __launch_bounds__(64) void attn_out_kernel(const AttnParams P) {
    __shared__ __attribute__((aligned(16))) float bufA[16 * AT_SA];
    __shared__ __attribute__((aligned(16))) float bufB[16 * AT_SB];
    const AttnWeights& W = P.w;
    const int lane = threadIdx.x, tiles = P.TP >> 4;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) << 4;
    const int d = W.d, ngd = W.ngd, DP = ngd << 4;
    const int r0 = 4 * (lane >> 4), c0 = lane & 15;
    const float* xb = P.xp + (int64_t)b * P.TP * DP;
    const hm_gf4* qrow = (const hm_gf4*)(P.qp + ((int64_t)b * P.TP + t0 + c0) * DP + r0);
    const hm_gf* xcol = (const hm_gf*)xb;
    hm_f32x4 cacc[AT_MAX_D / 16];
#pragma unroll
    for (int n = 0; n < AT_MAX_D / 16; ++n) cacc[n] = hm_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int u0 = 0; u0 < P.TP; u0 += 16) {
        const hm_f32x4 s = at_scores((const hm_gf4*)(xb + (int64_t)(u0 + c0) * DP + r0), qrow, ngd);
        const int64_t so = (int64_t)(t0 + c0) * P.TP + u0 + r0;
        const hm_f32x4 mx = *(const hm_gf4*)(P.smax + so), zs = *(const hm_gf4*)(P.ssum + so);
        hm_f32x4 a;
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = (u0 + r0 + r < P.T) ? expf(s[r] - mx[r]) / zs[r] : 0.f;    // the padded rows u >= T take no part
        // c^T[n][t] += sum_u x_b[u][n] a^T[u][t]: step e has k = u0 + 4 (l >> 4) + e, which is register e of the score tile
#pragma unroll
        for (int n = 0; n < AT_MAX_D / 16; ++n) {
            if (n < ngd) {
                const hm_gf* xc = xcol + (int64_t)(u0 + r0) * DP + 16 * n + c0;
                cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[0], a[0], cacc[n], 0, 0, 0);
                cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[DP], a[1], cacc[n], 0, 0, 0);
                cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[2 * DP], a[2], cacc[n], 0, 0, 0);
                cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[3 * DP], a[3], cacc[n], 0, 0, 0);
            }
        }
    }
    // c^T: the lane holds columns 16 n + 4 (l >> 4) + r of row t0 + (l & 15)
#pragma unroll
    for (int n = 0; n < AT_MAX_D / 16; ++n)
        if (n < ngd) *(hm_lf4*)(bufA + c0 * AT_SA + 16 * n + r0) = cacc[n];
    if (P.msave != nullptr) {
        float* mrow = P.msave + ((int64_t)b * P.TP + t0 + c0) * DP + r0;
#pragma unroll
        for (int n = 0; n < AT_MAX_D / 16; ++n)
            if (n < ngd) *(hm_gf4*)(mrow + 16 * n) = cacc[n];
    }
    __syncthreads();
    at_dense(bufA, AT_SA, W.wv, ngd, W.ngv, lane, [&](int t, const hm_f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bufB[(r0 + r) * AT_SB + 16 * t + c0] = acc[r];
    });
    __syncthreads();
    const float* xres = xb + (int64_t)t0 * DP;
    at_dense(bufB, AT_SB, W.wpt, W.ngv, ngd, lane, [&](int t, const hm_f32x4& acc) {
        const int c = 16 * t + c0;
#pragma unroll
        for (int r = 0; r < 4; ++r) bufA[(r0 + r) * AT_SA + c] = acc[r] + W.pb[c] + xres[(r0 + r) * DP + c];
    });
    __syncthreads();
    if (P.T > 1) {                                           // layers.py:136 on [B, T, d]
        at_layer_norm(bufA, AT_SA, d, W.ln1a, W.ln1b, W.eps, lane);
        __syncthreads();
    }
    at_dense(bufA, AT_SA, W.w1t, ngd, W.ngi, lane, [&](int t, const hm_f32x4& acc) {
        const int c = 16 * t + c0;
#pragma unroll
        for (int r = 0; r < 4; ++r) bufB[(r0 + r) * AT_SB + c] = fmaxf(acc[r] + W.b1[c], 0.f);
    });
    __syncthreads();
    at_dense(bufB, AT_SB, W.w2t, W.ngi, ngd, lane, [&](int t, const hm_f32x4& acc) {
        const int c = 16 * t + c0;
#pragma unroll
        for (int r = 0; r < 4; ++r) bufA[(r0 + r) * AT_SA + c] += acc[r] + W.b2[c];
    });
    __syncthreads();
    if (P.B > 1) {                                           // layers.py:136 on [T, B, d]
        at_layer_norm(bufA, AT_SA, d, W.ln2a, W.ln2b, W.eps, lane);
        __syncthreads();
    }
    for (int idx = lane; idx < 16 * d; idx += 64) {
        const int r = idx / d, j = idx - r * d, t = t0 + r;
        if (t < P.T) P.y[((int64_t)t * P.B + b) * d + j] = bufA[r * AT_SA + j];
    }
}

// Packs a [K][N] product (element (k, n) at src[k * sk + n * sn]) into float4 [ng][nt][64] on the host.
static inline void at_pack_host(float* dst, const float* src, int K, int N, int64_t sk, int64_t sn) {
    const int ng = at_pad16(K) >> 4, nt = at_pad16(N) >> 4;
    for (int g = 0; g < ng; ++g)
        for (int t = 0; t < nt; ++t)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 4; ++e) {
                    const int k = 16 * g + 4 * (l >> 4) + e, n = 16 * t + (l & 15);
                    dst[(((size_t)g * nt + t) * 64 + l) * 4 + e] = (k < K && n < N) ? src[k * sk + n * sn] : 0.f;
                }
}

// at_pack_host on the device (dsp_attn_refresh): one launch gathers the 12 matrices and 7 vectors of a handle into the packed
// buffer it already has.  blockIdx.y picks the job; a thread owns one float of the padded tile layout (K > 0) or one element of
// a vector (K == 0: dst[n] = src[n], the padding behind is left as create wrote it).  Pure data movement: the same bytes.
constexpr int AT_PACK_MATS = 12, AT_PACK_VECS = 7;
struct AtPackJob { const float* src; float* dst; int32_t K, N; int64_t sk, sn; };
struct AtPackJobs { AtPackJob job[AT_PACK_MATS + AT_PACK_VECS]; };

__global__ __launch_bounds__(256) void attn_pack_kernel(const AtPackJobs J) {
    const AtPackJob& j = J.job[blockIdx.y];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j.K == 0) {
        if (idx < j.N) j.dst[idx] = j.src[idx];
        return;
    }
    const int ng = (j.K + 15) >> 4, nt = (j.N + 15) >> 4;
    if (idx >=(int64_t)ng * nt * 256) return;
    const int e = (int)(idx & 3), l = (int)((idx >> 2) & 63);
    const int tile = (int)(idx >> 8), g = tile / nt, t = tile - g * nt;
    const int k = 16 * g + 4 * (l >> 4) + e, n = 16 * t + (l & 15);
    j.dst[idx] = (k < j.K && n < j.N) ? j.src[k * j.sk + n * j.sn] : 0.f;
}

// layers.SelfAttn for column b: e[t] = v . tanh(W y[t, b] + b_W) + c over all T rows, softmax over t, out[b] = sum_t w[t] y[t, b].
// One wave per column (d_rows: over the first min(*d_rows, T) rows only).  W [H, H] and y are read in place: row n of W is the B operand's column n (K = the input index), a
// float4 per lane and k-group; H is a multiple of 4, so a float4 lies inside the row or behind it.
__global__ __launch_bounds__(64) void selfattn_pool_kernel(const float* __restrict__ y, int T, int B, int H, const float* __restrict__ Wm,
                                                           const float* __restrict__ bW, const float* __restrict__ v,
                                                           const float* __restrict__ cb, float* __restrict__ out,
                                                           float* __restrict__ wsave /* training: the weights [T, B]; or NULL */,
                                                           const int32_t* __restrict__ d_rows /* the row count on the device; or NULL */) {
    __shared__ float e[AT_MAX_T];
    const int lane = threadIdx.x, b = blockIdx.x;
    // dsp_selfattn_pool_rows_batch: only the first *d_rows rows of the buffer exist for the softmax (one wave-uniform read; T,
    // the buffer's row count, stays the bound of every loop below)
    const int Tbuf = T;
    if (d_rows != nullptr) T = max(1, min(d_rows[0], T));
    const int ng = (H + 15) >> 4, nt = ng;
    const int r0 = 4 * (lane >> 4), c0 = lane & 15;
    const float c = cb[0];
    const hm_f32x4 zero4 = hm_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int m0 = 0; m0 < T; m0 += 16) {
        const int tt = m0 + c0;
        const hm_gf4* yrow = (const hm_gf4*)(y + ((int64_t)min(tt, T - 1) * B + b) * H);
        float p[4] = {0.f, 0.f, 0.f, 0.f};
        for (int n0 = 0; n0 < nt; n0 += 4) {
            hm_f32x4 acc[4];
            const hm_gf4* wrow[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[i] = zero4;
                wrow[i] = (const hm_gf4*)(Wm + (int64_t)min(16 * (n0 + i) + c0, H - 1) * H);
            }
            for (int g = 0; g < ng; ++g) {
                const int k = 16 * g + r0;
                const bool kin = k < H;
                const hm_f32x4 a = (kin && tt < T) ? yrow[k >> 2] : zero4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const hm_f32x4 w4 = (kin && 16 * (n0 + i) + c0 < H) ? wrow[i][k >> 2] : zero4;
                    acc[i] = at_mfma4(acc[i], a, w4);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = 16 * (n0 + i) + c0;
                if (n < H) {
                    const float vn = v[n], bn = bW[n];
#pragma unroll
                    for (int r = 0; r < 4; ++r) p[r] += vn * tanhf(acc[i][r] + bn);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = p[r];
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
            s += __shfl_xor(s, 8, 64);
            if (c0 == 0 && m0 + r0 + r < T) e[m0 + r0 + r] = s + c;
        }
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int t = lane; t < T; t += 64) mx = fmaxf(mx, e[t]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int t = lane; t < T; t += 64) sum += expf(e[t] - mx);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    __syncthreads();
    for (int t = lane; t < T; t += 64) e[t] = expf(e[t] - mx) / sum;
    __syncthreads();
    if (wsave != nullptr)                                   // (dsp_selfattn_pool_rows_train_batch: exact zeros behind the row count)
        for (int t = lane; t < Tbuf; t += 64) wsave[(int64_t)t * B + b] = t < T ? e[t] : 0.f;
    for (int h = lane; h < H; h += 64) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += e[t] * y[((int64_t)t * B + b) * H + h];
        out[(int64_t)b * H + h] = s;
    }
}
