// The gradients of the attention blocks of kernels_attn.h, fp32, on v_mfma_f32_16x16x4_f32 in the same operand layout.
//
// The encoder block (forward, n_head = 1, temper = sqrt(d), per utterance b):
//   Qt = tanh(x W_q);  q' = Qt W_k^T / temper;  s[b,t,u] = q'[b,t] . x_b[u];  A = exp(s - m[t,u]) / z[t,u]   (softmax over b)
//   M[b,t] = sum_u A[b,t,u] x_b[u];  o = M W_v;  r1 = o W_p^T + b_p + x;  z1 = LN1(r1);  h = relu(W_1 z1 + b_1);
//   r2 = W_2 h + b_2 + z1;  y = LN2(r2)
// Its backward is four launches, none of which holds a [B, T, T] tensor:
//   1. attn_bwd_row_kernel, one wave per (b, 16 rows): recomputes o .. r2 from the saved M and x, walks back through LN2, the
//      FFN, LN1, proj and W_v; writes the row gradients g_r2, g_pre1, g_z1, g_r1, g_o (the operands of the parameter-gradient
//      GEMMs) and the padded g_M and g_r1 rows the next launches read;
//   2. attn_bwd_stats_kernel, a workgroup per (u tile, t tile): D[t,u] = sum_b A[b,t,u] g_A[b,t,u], g_A = g_M[b,t] . x_b[u],
//      in the reduction order of attn_stats_kernel;
//   3. attn_bwd_q_kernel, one wave per (b, 16 rows t): g_S = A (g_A - D), g_q'[b,t] = sum_u g_S x_b[u] (u ascending), then
//      g_Qt = g_q' W_k / temper, g_preQ = g_Qt (1 - Qt^2), and the row part of dx: g_r1 + g_preQ W_q^T;
//   4. attn_bwd_col_kernel, one wave per (b, 16 columns u): dx[b,u] = row part + sum_t (A g_M[b,t] + g_S q'[b,t]), t ascending.
// Launches 2 to 4 recompute the score tiles from the padded x and q' of the tape with the saved m, z, exactly as attn_out_kernel
// does (launch 4 with the operands swapped: the tile comes out as D[t][u], the B operand of a sum over t; the products and
// their order are the same, so are the bits).  g_M is written as zero for the rows t >= T, which therefore add nothing to D,
// to g_S or to dx; u >= T weighs 0 as in the forward.  Fixed reduction orders, no atomics; every loop is bounded by an
// argument; no workgroup waits on another one; every load falls inside a padded buffer of the tape or the workspace.
//
// layers.SelfAttn's backward is one launch, one wave per column (selfattn_pool_bwd_kernel below).
#pragma once

#include "kernels_attn.h"

struct AttnBwdWeights {
    const float4* w2;      // [d][d_inner]   g_r2 -> g_h          (pos_ffn.w_2.weight as it lies)
    const float4* w1;      // [d_inner][d]   g_pre1 -> g_z1       (pos_ffn.w_1.weight)
    const float4* wp;      // [d][d_v]       g_r1 -> g_o          (proj.weight)
    const float4* wvt;     // [d_v][d]       g_o -> g_M           (w_vs^T)
    const float4* wk;      // [d][d_k]       g_q' -> g_Qt         (w_ks, in front of the temperature)
    const float4* wqt;     // [d_k][d]       g_preQ -> dx         (w_qs^T)
};

struct AttnBwdParams {
    AttnWeights w;
    AttnBwdWeights v;
    int32_t T, TP, B;
    int32_t di, dk, dv;    // d_inner, d_k, d_v as the caller's rows hold them
    const float *xp, *qp, *smax, *ssum, *mp;    // tape: [B, TP, DP] x 2, [TP, TP] x 2, [B, TP, DP]
    const float* gy;       // [T, B, d]
    float* gx;             // [T, B, d] or NULL
    float *g_r2, *g_pre1, *g_z1, *g_r1, *g_o, *g_q, *g_preq;    // da: dense [T, B, .] rows
    float* gm;             // workspace: [B, TP, DP]   g_M, zero rows behind T
    float* dxr;            //            [B, TP, DP]   the row part of dx (read only when gx is wanted)
    float* dstat;          //            [TP, TP]      D
};

// The wave's 16 rows of an LDS buffer into a dense [T, B, n] tensor; rows t >= T are not written.
__device__ __forceinline__ void at_store_rows(float* __restrict__ dst, const float* buf, int stride, int n, int t0, int b, int T, int B, int lane) {
    for (int idx = lane; idx < 16 * n; idx += 64) {
        const int r = idx / n, j = idx - r * n, t = t0 + r;
        if (t < T) dst[((int64_t)t * B + b) * n + j] = buf[r * stride + j];
    }
}

// at_layer_norm from src into dst (src is kept: the backward needs the rows in front of the normalisation).
__device__ __forceinline__ void at_layer_norm_to(const float* src, float* dst, int stride, int d, const float* __restrict__ a2,
                                                 const float* __restrict__ b2, float eps, int lane) {
    const float* row = src + (lane >> 2) * stride;
    float* out = dst + (lane >> 2) * stride;
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
    const float sigma = sqrtf(v / (float)(d - 1));
    const float inv = 1.0f / (sigma + eps);
    for (int j = q; j < d; j += 4) out[j] = (row[j] - mu) * inv * a2[j] + b2[j];
}

// The backward of layers.LayerNormalization over the wave's 16 rows, in place on g: with c = r - mu, s = sigma + eps and
// g_n = g a_2:  g_r = (g_n - mean(g_n)) / s - c sum(g_n c) / (s^2 sigma (d - 1)).  Four lanes per row, as at_layer_norm.
__device__ __forceinline__ void at_layer_norm_bwd(float* g, const float* r, int stride, int d, const float* __restrict__ a2, float eps, int lane) {
    const float* row = r + (lane >> 2) * stride;
    float* grow = g + (lane >> 2) * stride;
    const int q = lane & 3;
    float s = 0.f;
    for (int j = q; j < d; j += 4) s += row[j];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    const float mu = s / (float)d;
    float v = 0.f, sg = 0.f, sgc = 0.f;
    for (int j = q; j < d; j += 4) {
        const float c = row[j] - mu, gn = grow[j] * a2[j];
        v += c * c; sg += gn; sgc += gn * c;
    }
    v += __shfl_xor(v, 1, 64);   v += __shfl_xor(v, 2, 64);
    sg += __shfl_xor(sg, 1, 64); sg += __shfl_xor(sg, 2, 64);
    sgc += __shfl_xor(sgc, 1, 64); sgc += __shfl_xor(sgc, 2, 64);
    const float sigma = sqrtf(v / (float)(d - 1));
    const float sp = sigma + eps, inv = 1.0f / sp;
    const float mg = sg / (float)d;
    const float k = sgc / (sp * sp * sigma * (float)(d - 1));
    for (int j = q; j < d; j += 4) grow[j] = (grow[j] * a2[j] - mg) * inv - (row[j] - mu) * k;
}

// Launch 1: the row-wise part, one wave per (utterance, 16 rows).
__global__ __launch_bounds__(64) void attn_bwd_row_kernel(const AttnBwdParams P) {
    __shared__ __attribute__((aligned(16))) float bufM[16 * AT_SA];      // M, then r2
    __shared__ __attribute__((aligned(16))) float bufR[16 * AT_SA];      // r1
    __shared__ __attribute__((aligned(16))) float bufZ[16 * AT_SA];      // z1
    __shared__ __attribute__((aligned(16))) float bufG[16 * AT_SA];      // the gradient on its way back
    __shared__ __attribute__((aligned(16))) float bufB[16 * AT_SB];
    const AttnWeights& W = P.w;
    const AttnBwdWeights& V = P.v;
    const int lane = threadIdx.x, tiles = P.TP >> 4;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) << 4;
    const int d = W.d, ngd = W.ngd, DP = ngd << 4;
    const int r0 = 4 * (lane >> 4), c0 = lane & 15;
    const int64_t rows = ((int64_t)b * P.TP + t0) * DP;
    const float* xres = P.xp + rows;
    for (int idx = lane; idx < 16 * DP; idx += 64) {
        const int r = idx / DP, j = idx - r * DP, t = t0 + r;
        bufM[r * AT_SA + j] = P.mp[rows + idx];
        bufG[r * AT_SA + j] = (t < P.T && j < d) ? P.gy[((int64_t)t * P.B + b) * d + j] : 0.f;
    }
    __syncthreads();
    // ---- the forward rows again, in the forward's own order of operations
    at_dense(bufM, AT_SA, W.wv, ngd, W.ngv, lane, [&](int t, const hm_f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bufB[(r0 + r) * AT_SB + 16 * t + c0] = acc[r];
    });
    __syncthreads();
    at_dense(bufB, AT_SB, W.wpt, W.ngv, ngd, lane, [&](int t, const hm_f32x4& acc) {
        const int c = 16 * t + c0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = acc[r] + W.pb[c] + xres[(r0 + r) * DP + c];
            bufR[(r0 + r) * AT_SA + c] = v;
            bufZ[(r0 + r) * AT_SA + c] = v;
        }
    });
    __syncthreads();
    if (P.T > 1) {
        at_layer_norm_to(bufR, bufZ, AT_SA, d, W.ln1a, W.ln1b, W.eps, lane);
        __syncthreads();
    }
    at_dense(bufZ, AT_SA, W.w1t, ngd, W.ngi, lane, [&](int t, const hm_f32x4& acc) {
        const int c = 16 * t + c0;
#pragma unroll
        for (int r = 0; r < 4; ++r) bufB[(r0 + r) * AT_SB + c] = fmaxf(acc[r] + W.b1[c], 0.f);
    });
    __syncthreads();
    at_dense(bufB, AT_SB, W.w2t, W.ngi, ngd, lane, [&](int t, const hm_f32x4& acc) {
        const int c = 16 * t + c0;
#pragma unroll
        for (int r = 0; r < 4; ++r) bufM[(r0 + r) * AT_SA + c] = bufZ[(r0 + r) * AT_SA + c] + (acc[r] + W.b2[c]);
    });
    __syncthreads();
    // ---- and back
    if (P.B > 1) {
        at_layer_norm_bwd(bufG, bufM, AT_SA, d, W.ln2a, W.eps, lane);
        __syncthreads();
    }
    at_store_rows(P.g_r2, bufG, AT_SA, d, t0, b, P.T, P.B, lane);
    at_dense(bufG, AT_SA, V.w2, ngd, W.ngi, lane, [&](int t, const hm_f32x4& acc) {
        const int c = 16 * t + c0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* p = bufB + (r0 + r) * AT_SB + c;
            *p = (*p > 0.f) ? acc[r] : 0.f;                  // h in, g_pre1 out
        }
    });
    __syncthreads();
    at_store_rows(P.g_pre1, bufB, AT_SB, P.di, t0, b, P.T, P.B, lane);
    at_dense(bufB, AT_SB, V.w1, W.ngi, ngd, lane, [&](int t, const hm_f32x4& acc) {
        const int c = 16 * t + c0;
#pragma unroll
        for (int r = 0; r < 4; ++r) bufG[(r0 + r) * AT_SA + c] += acc[r];
    });
    __syncthreads();
    at_store_rows(P.g_z1, bufG, AT_SA, d, t0, b, P.T, P.B, lane);
    if (P.T > 1) {
        __syncthreads();
        at_layer_norm_bwd(bufG, bufR, AT_SA, d, W.ln1a, W.eps, lane);
        __syncthreads();
    }
    at_store_rows(P.g_r1, bufG, AT_SA, d, t0, b, P.T, P.B, lane);
    for (int idx = lane; idx < 16 * DP; idx += 64) {
        const int r = idx / DP, j = idx - r * DP;
        P.dxr[rows + idx] = (t0 + r < P.T) ? bufG[r * AT_SA + j] : 0.f;
    }
    __syncthreads();
    at_dense(bufG, AT_SA, V.wp, ngd, W.ngv, lane, [&](int t, const hm_f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bufB[(r0 + r) * AT_SB + 16 * t + c0] = acc[r];
    });
    __syncthreads();
    at_store_rows(P.g_o, bufB, AT_SB, P.dv, t0, b, P.T, P.B, lane);
    at_dense(bufB, AT_SB, V.wvt, W.ngv, ngd, lane, [&](int t, const hm_f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            P.gm[rows + (r0 + r) * DP + 16 * t + c0] = (t0 + r0 + r < P.T) ? acc[r] : 0.f;
    });
}

// The softmax weights of a transposed score tile D[u][t] (registers r: rows u0 + 4 (l >> 4) + r, column t0 + (l & 15)).
__device__ __forceinline__ hm_f32x4 at_weights_ut(const hm_f32x4 s, const float* smax, const float* ssum, int64_t so, int u_first, int T) {
    const hm_f32x4 mx = *(const hm_gf4*)(smax + so), zs = *(const hm_gf4*)(ssum + so);
    hm_f32x4 a;
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = (u_first + r < T) ? expf(s[r] - mx[r]) / zs[r] : 0.f;
    return a;
}

// Launch 2: D[t,u] = sum_b A g_A.  A workgroup per (u tile, t tile); wave w sums its range of b in ascending order, wave 0
// adds the eight partial sums in order.
__global__ __launch_bounds__(AT_STAT_WAVES * 64) void attn_bwd_stats_kernel(const AttnBwdParams P) {
    __shared__ float sd[AT_STAT_WAVES][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.x << 4, t0 = blockIdx.y << 4;
    const int ngd = P.w.ngd, DP = ngd << 4;
    const int chunk = (P.B + AT_STAT_WAVES - 1) / AT_STAT_WAVES;
    const int b_lo = w * chunk, b_hi = min(P.B, b_lo + chunk);
    const int64_t per_b = (int64_t)P.TP * DP;
    const int64_t xoff = (int64_t)(u0 + (lane & 15)) * DP + 4 * (lane >> 4), qoff = (int64_t)(t0 + (lane & 15)) * DP + 4 * (lane >> 4);
    const int64_t so = (int64_t)(t0 + (lane & 15)) * P.TP + u0 + 4 * (lane >> 4);     // [t][u .. u + 3]
    hm_f32x4 acc = hm_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int b = b_lo; b < b_hi; ++b) {
        const hm_gf4* xrow = (const hm_gf4*)(P.xp + b * per_b + xoff);
        const hm_f32x4 s = at_scores(xrow, (const hm_gf4*)(P.qp + b * per_b + qoff), ngd);
        const hm_f32x4 ga = at_scores(xrow, (const hm_gf4*)(P.gm + b * per_b + qoff), ngd);
        const hm_f32x4 a = at_weights_ut(s, P.smax, P.ssum, so, u0 + 4 * (lane >> 4), P.T);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += a[r] * ga[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) sd[w][r][lane] = acc[r];
    __syncthreads();
    if (w != 0) return;
    hm_f32x4 out;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = sd[0][r][lane];
        for (int k = 1; k < AT_STAT_WAVES; ++k) v += sd[k][r][lane];
        out[r] = v;
    }
    *(hm_gf4*)(P.dstat + so) = out;
}

// Launch 3: g_q', g_preQ and the row part of dx.  One wave per (utterance, 16 rows t).
__global__ __launch_bounds__(64) void attn_bwd_q_kernel(const AttnBwdParams P) {
    __shared__ __attribute__((aligned(16))) float bufA[16 * AT_SA];
    __shared__ __attribute__((aligned(16))) float xs[16 * AT_SA];
    __shared__ __attribute__((aligned(16))) float tq[16 * AT_SK];
    const AttnWeights& W = P.w;
    const AttnBwdWeights& V = P.v;
    const int lane = threadIdx.x, tiles = P.TP >> 4;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) << 4;
    const int d = W.d, ngd = W.ngd, DP = ngd << 4;
    const int r0 = 4 * (lane >> 4), c0 = lane & 15;
    const float* xb = P.xp + (int64_t)b * P.TP * DP;
    const int64_t rows = ((int64_t)b * P.TP + t0) * DP;
    const hm_gf4* qrow = (const hm_gf4*)(P.qp + rows + c0 * DP + r0);
    const hm_gf4* grow = (const hm_gf4*)(P.gm + rows + c0 * DP + r0);
    const hm_gf* xcol = (const hm_gf*)xb;
    hm_f32x4 cacc[AT_MAX_D / 16];
#pragma unroll
    for (int n = 0; n < AT_MAX_D / 16; ++n) cacc[n] = hm_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int u0 = 0; u0 < P.TP; u0 += 16) {
        const hm_gf4* xrow = (const hm_gf4*)(xb + (int64_t)(u0 + c0) * DP + r0);
        const hm_f32x4 s = at_scores(xrow, qrow, ngd);
        const hm_f32x4 ga = at_scores(xrow, grow, ngd);
        const int64_t so = (int64_t)(t0 + c0) * P.TP + u0 + r0;
        const hm_f32x4 a = at_weights_ut(s, P.smax, P.ssum, so, u0 + r0, P.T);
        const hm_f32x4 dd = *(const hm_gf4*)(P.dstat + so);
        hm_f32x4 gs;
#pragma unroll
        for (int r = 0; r < 4; ++r) gs[r] = a[r] * (ga[r] - dd[r]);
#pragma unroll
        for (int n = 0; n < AT_MAX_D / 16; ++n) {
            if (n < ngd) {
                const hm_gf* xc = xcol + (int64_t)(u0 + r0) * DP + 16 * n + c0;
                cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[0], gs[0], cacc[n], 0, 0, 0);
                cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[DP], gs[1], cacc[n], 0, 0, 0);
                cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[2 * DP], gs[2], cacc[n], 0, 0, 0);
                cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[3 * DP], gs[3], cacc[n], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < AT_MAX_D / 16; ++n)
        if (n < ngd) *(hm_lf4*)(bufA + c0 * AT_SA + 16 * n + r0) = cacc[n];
    for (int idx = lane; idx < 16 * DP; idx += 64) {
        const int r = idx / DP, j = idx - r * DP;
        xs[r * AT_SA + j] = xb[(int64_t)t0 * DP + idx];
    }
    __syncthreads();
    at_store_rows(P.g_q, bufA, AT_SA, d, t0, b, P.T, P.B, lane);
    at_dense(xs, AT_SA, W.wq, ngd, W.ngk, lane, [&](int t, const hm_f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) tq[(r0 + r) * AT_SK + 16 * t + c0] = tanhf(acc[r]);
    });
    __syncthreads();
    at_dense(bufA, AT_SA, V.wk, ngd, W.ngk, lane, [&](int t, const hm_f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* p = tq + (r0 + r) * AT_SK + 16 * t + c0;
            const float q = *p;
            *p = (acc[r] * W.inv_temper) * (1.0f - q * q);  // Qt in, g_preQ out
        }
    });
    __syncthreads();
    at_store_rows(P.g_preq, tq, AT_SK, P.dk, t0, b, P.T, P.B, lane);
    if (P.gx == nullptr) return;
    at_dense(tq, AT_SK, V.wqt, W.ngk, ngd, lane, [&](int t, const hm_f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* p = P.dxr + rows + (r0 + r) * DP + 16 * t + c0;
            *p += acc[r];                                    // this wave wrote these rows' g_r1 in launch 1; no other wave touches them
        }
    });
}

// Launch 4: dx.  One wave per (utterance, 16 columns u); the tile is D[t][u] here, the B operand of the sums over t.
__global__ __launch_bounds__(64) void attn_bwd_col_kernel(const AttnBwdParams P) {
    const AttnWeights& W = P.w;
    const int lane = threadIdx.x, tiles = P.TP >> 4;
    const int b = blockIdx.x / tiles, u0 = (blockIdx.x - b * tiles) << 4;
    const int d = W.d, ngd = W.ngd, DP = ngd << 4;
    const int r0 = 4 * (lane >> 4), c0 = lane & 15;
    const int64_t base = (int64_t)b * P.TP * DP;
    const float* qb = P.qp + base;
    const float* gb = P.gm + base;
    const hm_gf4* xrow = (const hm_gf4*)(P.xp + base + (int64_t)(u0 + c0) * DP + r0);
    const bool live = u0 + c0 < P.T;
    hm_f32x4 cacc[AT_MAX_D / 16];
#pragma unroll
    for (int n = 0; n < AT_MAX_D / 16; ++n) cacc[n] = hm_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < P.TP; t0 += 16) {
        const hm_gf4* qrow = (const hm_gf4*)(qb + (int64_t)(t0 + c0) * DP + r0);
        const hm_gf4* grow = (const hm_gf4*)(gb + (int64_t)(t0 + c0) * DP + r0);
        const hm_f32x4 s = at_scores(qrow, xrow, ngd);       // D[t][u]: the same products in the same order as D[u][t]
        const hm_f32x4 ga = at_scores(grow, xrow, ngd);
        hm_f32x4 a, gs;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t so = (int64_t)(t0 + r0 + r) * P.TP + u0 + c0;
            a[r] = live ? expf(s[r] - P.smax[so]) / P.ssum[so] : 0.f;
            gs[r] = a[r] * (ga[r] - P.dstat[so]);
        }
        // dx^T[n][u] += sum_t g_M[t][n] a[t][u] + q'[t][n] g_S[t][u]: step e has k = t0 + 4 (l >> 4) + e
#pragma unroll
        for (int n = 0; n < AT_MAX_D / 16; ++n) {
            if (n < ngd) {
                const hm_gf* gc = (const hm_gf*)gb + (int64_t)(t0 + r0) * DP + 16 * n + c0;
                const hm_gf* qc = (const hm_gf*)qb + (int64_t)(t0 + r0) * DP + 16 * n + c0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(gc[e * DP], a[e], cacc[n], 0, 0, 0);
                    cacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(qc[e * DP], gs[e], cacc[n], 0, 0, 0);
                }
            }
        }
    }
    // the lane holds columns 16 n + 4 (l >> 4) + r of row u0 + (l & 15)
    const int u = u0 + c0;
    const hm_gf4* rowpart = (const hm_gf4*)(P.dxr + base + (int64_t)u * DP + r0);
#pragma unroll
    for (int n = 0; n < AT_MAX_D / 16; ++n) {
        if (n < ngd) {
            const hm_f32x4 rp = rowpart[4 * n];
            if (live) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * n + r0 + r;
                    if (j < d) P.gx[((int64_t)u * P.B + b) * d + j] = rp[r] + cacc[n][r];
                }
            }
        }
    }
}

// layers.SelfAttn's backward for column b, one wave:
//   g_w[t] = g_out[b] . y[t,b];  g_e = w (g_w - sum_t w g_w);  g_pre[t] = g_e[t] v (1 - tanh^2(W y[t,b] + b_W));  g_y[t] = w[t] g_out[b] + g_pre[t] W
// The energies' pre-activations are recomputed on the matrix pipe as in the forward.  Writes g_pre [T, B, H], g_e [T, B], the
// per-column partial sums gv_part[b] = sum_t g_e[t] tanh(.) [B, H] (t ascending) and, unless gy is NULL, g_y [T, B, H].
__global__ __launch_bounds__(64) void selfattn_pool_bwd_kernel(const float* __restrict__ y, int T, int B, int H, const float* __restrict__ Wm,
                                                               const float* __restrict__ bW, const float* __restrict__ v,
                                                               const float* __restrict__ wsv, const float* __restrict__ gout,
                                                               float* __restrict__ gy, float* __restrict__ gpre, float* __restrict__ ge_out,
                                                               float* __restrict__ gvp_out,
                                                               const int32_t* __restrict__ d_rows /* the row count on the device; or NULL */) {
    __shared__ float ws[AT_MAX_T], ge[AT_MAX_T], gvp[AT_MAX_H];
    __shared__ __attribute__((aligned(16))) float gp[16 * AT_SB];
    const int lane = threadIdx.x, b = blockIdx.x;
    // dsp_selfattn_pool_rows_backward_batch: the first *d_rows rows of the buffers are the block (one wave-uniform read); the
    // rows behind them are written as zeros at the end
    const int Tbuf = T;
    if (d_rows != nullptr) T = max(1, min(d_rows[0], T));
    const int ng = (H + 15) >> 4, nt = ng, HP = ng << 4;
    const int r0 = 4 * (lane >> 4), c0 = lane & 15;
    const int TP = (T + 15) & ~15;
    const hm_f32x4 zero4 = hm_f32x4{0.f, 0.f, 0.f, 0.f};
    const hm_gf4* g4 = (const hm_gf4*)(gout + (int64_t)b * H);          // (row b of [B, H]: H a multiple of 4, gout 16-byte aligned)
    float part = 0.f;
    for (int t = lane; t < TP; t += 64) {
        float gw = 0.f, wt = 0.f;
        if (t < T) {
            const hm_gf4* yr = (const hm_gf4*)(y + ((int64_t)t * B + b) * H);
            for (int k = 0; k < (H >> 2); ++k) {
                const hm_f32x4 a = yr[k], g = g4[k];
                gw += a.x * g.x + a.y * g.y + a.z * g.z + a.w * g.w;
            }
            wt = wsv[(int64_t)t * B + b];
        }
        ws[t] = wt; ge[t] = gw;
        part += wt * gw;
    }
    for (int h = lane; h < AT_MAX_H; h += 64) gvp[h] = 0.f;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
    __syncthreads();
    for (int t = lane; t < TP; t += 64) {
        const float g = ws[t] * (ge[t] - part);
        ge[t] = g;
        if (t < T) ge_out[(int64_t)t * B + b] = g;
    }
    __syncthreads();
    for (int m0 = 0; m0 < T; m0 += 16) {
        const int tt = m0 + c0;
        const hm_gf4* yrow = (const hm_gf4*)(y + ((int64_t)min(tt, T - 1) * B + b) * H);
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
                if (n0 + i < nt) {
                    const int n = 16 * (n0 + i) + c0;
                    const bool nin = n < H;
                    const float vn = nin ? v[n] : 0.f, bn = nin ? bW[n] : 0.f;
                    float pv = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int t = m0 + r0 + r;              // (t < TP: ge is zero behind T)
                        const float th = tanhf(acc[i][r] + bn), g = ge[t];
                        const float gpv = nin ? g * vn * (1.0f - th * th) : 0.f;
                        gp[(r0 + r) * AT_SB + n] = gpv;
                        if (nin && t < T) gpre[((int64_t)t * B + b) * H + n] = gpv;
                        pv += g * th;
                    }
                    pv += __shfl_xor(pv, 16, 64);
                    pv += __shfl_xor(pv, 32, 64);
                    if (nin && lane < 16) gvp[n] += pv;         // one lane owns n: tiles m0 are added in ascending order
                }
            }
        }
        __syncthreads();
        if (gy != nullptr) {
            const hm_lf4* a4 = (const hm_lf4*)(gp + c0 * AT_SB + r0);
            for (int k0 = 0; k0 < nt; k0 += 4) {
                hm_f32x4 acc[4];
                int col[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { acc[i] = zero4; col[i] = 16 * min(k0 + i, nt - 1) + c0; }
                for (int g = 0; g < ng; ++g) {
                    const hm_f32x4 a = a4[4 * g];
                    const int n = 16 * g + r0;                  // rows n .. n + 3 of W: inside the matrix or wholly behind it (H % 4 == 0)
                    const bool nin = n < H;
                    const hm_gf* wr = (const hm_gf*)Wm + (int64_t)(nin ? n : 0) * H;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const bool in = nin && col[i] < H;
                        const int cc = in ? col[i] : 0;
                        hm_f32x4 w4;
                        w4.x = in ? wr[cc] : 0.f;
                        w4.y = in ? wr[H + cc] : 0.f;
                        w4.z = in ? wr[2 * H + cc] : 0.f;
                        w4.w = in ? wr[3 * H + cc] : 0.f;
                        acc[i] = at_mfma4(acc[i], a, w4);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (k0 + i < nt && col[i] < H) {
                        const float go = gout[(int64_t)b * H + col[i]];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int t = m0 + r0 + r;
                            if (t < T) gy[((int64_t)t * B + b) * H + col[i]] = ws[t] * go + acc[i][r];
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    for (int h = lane; h < H; h += 64) gvp_out[(int64_t)b * H + h] = gvp[h];
    for (int t = T; t < Tbuf; ++t) {
        for (int h = lane; h < H; h += 64) {
            gpre[((int64_t)t * B + b) * H + h] = 0.f;
            if (gy != nullptr) gy[((int64_t)t * B + b) * H + h] = 0.f;
        }
        if (lane == 0) ge_out[(int64_t)t * B + b] = 0.f;
    }
    (void)HP;
}
