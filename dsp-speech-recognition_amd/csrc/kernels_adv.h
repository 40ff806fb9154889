// The speaker discriminator of adv_clf.AdvHRNN on the pooled feature (adv_clf.py:34-38): a gradient reversal, Linear(F, H),
// tanh, Linear(H, S).  Its loss is terminal, so forward, loss and every gradient are formed by one native call
// (include/dsp_frontend.h: dsp_adv_disc_forward, dsp_adv_disc_train).  Two kernels here, both over tiles of ADV_ROWS batch rows:
//   adv_disc_fwd_kernel   a = tanh(feat W1^T + b1) -> global [B, H] and LDS;  z = a W2^T + b2 -> [B, S].  a stays in LDS between
//                         the two products.
//   adv_disc_bwd_kernel   da = dz W2;  dpre = da (1 - a^2) -> global [B, H] and LDS;  dfeat = -gamma (dpre W1), gamma applied as
//                         ONE final multiply (read from d_gamma when given, so a schedule moves it between graph replays).
// fp32 on v_mfma_f32_16x16x4_f32: exact f32, every element an fmaf chain in a fixed order (below).  No atomics, no memset, no
// grid barrier, no allocation; every store is a plain C++ assignment.  gfx950 only (wave64).
//
// Tiling: 512 threads = 8 waves.  Lane (i = l & 15, q = l >> 4) of a wave holds row i of the A operand and row i of the
// (transposed) B operand; one stage covers 16 steps of the reduced axis: the lane loads the four steps k0 + 4 q .. k0 + 4 q + 3
// (one 16-byte load where the operand allows it) and MFMA j of the stage takes element j, i.e. the steps k0 + j, k0 + 4 + j,
// k0 + 8 + j, k0 + 12 + j.  Both operands use the same map, so the products pair up; the order of every chain is
// stage by stage, j = 0 .. 3, q = 0 .. 3, whatever the batch size.  The accumulator of lane l holds rows 4 q + r (r = 0 .. 3)
// of column i.  A wave owns up to ADV_TILES column tiles at a time (tile = wave + 8 t), so the A operand is loaded once per
// stage for all of them.  Rows behind B, columns behind the matrix and steps behind the reduced axis are exact zeros that are
// never loaded.
// LDS: 16 x (512 + 4) x 4 B = 33 KiB per workgroup; the row stride of 516 words puts the 16 lanes of a 16-byte read on all 64
// banks once.
// LIMITS (checked on the host, csrc/dsp_adv.hip): B in [1, 16384], F in [1, 2048], H in [1, 512], S in [2, 64].
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels_wgrad.h"               // wgrad_f4, rows_load4

constexpr int ADV_ROWS = 16;             // batch rows per workgroup
constexpr int ADV_WAVES = 8;
constexpr int ADV_THREADS = 64 * ADV_WAVES;
constexpr int ADV_TILES = 4;             // column tiles a wave holds at a time: 8 x 4 x 16 = 512 columns
constexpr int ADV_MAX_B = 16384, ADV_MAX_F = 2048, ADV_MAX_H = 512, ADV_MAX_S = 64;
constexpr int ADV_LDS_STRIDE = ADV_MAX_H + 4;

struct AdvParams {
    const float* feat;       // [B, F], row stride ld_feat
    int64_t ld_feat;
    const float *W1, *b1, *W2, *b2;      // [H, F], [H], [S, H], [S]
    int32_t B, F, H, S;
    float* a;                // [B, H] (forward: may be NULL)
    float* z;                // [B, S], row stride ld_z
    int64_t ld_z;
    const float* dz;         // [B, S] dense
    float* dpre;             // [B, H]
    float* dfeat;            // [B, F], row stride ld_dfeat, or NULL
    int64_t ld_dfeat;
    const float* d_gamma;    // fp32 [1] or NULL
    float gamma;
    int32_t feat_vec, w1_vec, w2_vec, dz_vec;   // 16-byte loads allowed (pointer aligned, row stride a multiple of 4)
};

__device__ __forceinline__ wgrad_f4 adv_zero4() { return wgrad_f4{0.0f, 0.0f, 0.0f, 0.0f}; }

// One stage for one tile: the four MFMAs over the elements of the two 16-byte operands.
__device__ __forceinline__ void adv_stage(const wgrad_f4& a, const wgrad_f4& b, wgrad_f4& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
}

// Column `col` of the rows k .. k + 3 of a dense [rows, cols] matrix: zero behind either edge.
__device__ __forceinline__ wgrad_f4 adv_load_col4(const float* __restrict__ w, int k, int rows, int col, int cols) {
    wgrad_f4 v = adv_zero4();
    if (col >= cols) return v;
    const float* p = w + (int64_t)k * cols + col;
    if (k < rows) v.x = p[0];
    if (k + 1 < rows) v.y = p[cols];
    if (k + 2 < rows) v.z = p[2 * (int64_t)cols];
    if (k + 3 < rows) v.w = p[3 * (int64_t)cols];
    return v;
}

__global__ __launch_bounds__(ADV_THREADS) void adv_disc_fwd_kernel(AdvParams P) {
    __shared__ __attribute__((aligned(16))) float a_s[ADV_ROWS][ADV_LDS_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * ADV_ROWS;
    const int B = P.B, F = P.F, H = P.H, S = P.S;
    const int HP = (H + 15) & ~15;

    // 1. pre = feat W1^T: A = feat rows, B = W1 rows (both with the reduced axis along the row)
    const float* frow = row0 + i < B ? P.feat + (row0 + i) * P.ld_feat : nullptr;
    const float* wrow[ADV_TILES];
    wgrad_f4 acc[ADV_TILES];
#pragma unroll
    for (int t = 0; t < ADV_TILES; ++t) {
        const int h = 16 * (wave + ADV_WAVES * t) + i;
        wrow[t] = h < H ? P.W1 + (int64_t)h * F : nullptr;
        acc[t] = adv_zero4();
    }
    wgrad_f4 fa = rows_load4(frow, 4 * q, F, P.feat_vec != 0), wb[ADV_TILES];
#pragma unroll
    for (int t = 0; t < ADV_TILES; ++t) wb[t] = rows_load4(wrow[t], 4 * q, F, P.w1_vec != 0);
    for (int k0 = 0; k0 < F; k0 += 16) {
        const wgrad_f4 fc = fa;
        wgrad_f4 wc[ADV_TILES];
#pragma unroll
        for (int t = 0; t < ADV_TILES; ++t) wc[t] = wb[t];
        if (k0 + 16 < F) {                                                   // the next stage's loads in front of this one's MFMAs
            fa = rows_load4(frow, k0 + 16 + 4 * q, F, P.feat_vec != 0);
#pragma unroll
            for (int t = 0; t < ADV_TILES; ++t) wb[t] = rows_load4(wrow[t], k0 + 16 + 4 * q, F, P.w1_vec != 0);
        }
#pragma unroll
        for (int t = 0; t < ADV_TILES; ++t)
            if (16 * (wave + ADV_WAVES * t) < H) adv_stage(fc, wc[t], acc[t]);   // (uniform over the wave)
    }
#pragma unroll
    for (int t = 0; t < ADV_TILES; ++t) {
        const int h0 = 16 * (wave + ADV_WAVES * t);
        if (h0 >= HP) continue;
        const int col = h0 + i;
        const float bias = col < H ? P.b1[col] : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * q + r;
            const float v = col < H ? tanhf(acc[t][r] + bias) : 0.0f;        // exact zeros in the columns [H, HP)
            a_s[row][col] = v;
            if (P.a != nullptr && col < H && row0 + row < B) P.a[(row0 + row) * H + col] = v;
        }
    }
    __syncthreads();

    // 2. z = a W2^T + b2: wave w takes the columns 16 w .. 16 w + 15
    const int s0 = 16 * wave;
    if (s0 >= S) return;
    const float* w2row = s0 + i < S ? P.W2 + (int64_t)(s0 + i) * H : nullptr;
    wgrad_f4 zc = adv_zero4();
    for (int k0 = 0; k0 < HP; k0 += 16) {
        const wgrad_f4 av = *reinterpret_cast<const wgrad_f4*>(&a_s[i][k0 + 4 * q]);
        const wgrad_f4 wv = rows_load4(w2row, k0 + 4 * q, H, P.w2_vec != 0);
        adv_stage(av, wv, zc);
    }
    const int col = s0 + i;
    if (col < S) {
        const float bias = P.b2[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t g = row0 + 4 * q + r;
            if (g < B) P.z[g * P.ld_z + col] = zc[r] + bias;
        }
    }
}

__global__ __launch_bounds__(ADV_THREADS) void adv_disc_bwd_kernel(AdvParams P) {
    __shared__ __attribute__((aligned(16))) float dp_s[ADV_ROWS][ADV_LDS_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * ADV_ROWS;
    const int B = P.B, F = P.F, H = P.H, S = P.S;
    const int HP = (H + 15) & ~15;

    // 1. da = dz W2: A = dz rows (reduced axis along the row), B = columns of W2
    {
        const float* dzrow = row0 + i < B ? P.dz + (row0 + i) * S : nullptr;
        wgrad_f4 acc[ADV_TILES];
#pragma unroll
        for (int t = 0; t < ADV_TILES; ++t) acc[t] = adv_zero4();
        for (int k0 = 0; k0 < S; k0 += 16) {
            const wgrad_f4 dv = rows_load4(dzrow, k0 + 4 * q, S, P.dz_vec != 0);
#pragma unroll
            for (int t = 0; t < ADV_TILES; ++t) {
                const int h0 = 16 * (wave + ADV_WAVES * t);
                if (h0 >= H) continue;                                       // (uniform over the wave)
                adv_stage(dv, adv_load_col4(P.W2, k0 + 4 * q, S, h0 + i, H), acc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < ADV_TILES; ++t) {
            const int h0 = 16 * (wave + ADV_WAVES * t);
            if (h0 >= HP) continue;
            const int col = h0 + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                const int64_t g = row0 + row;
                float v = 0.0f;                                              // exact zeros behind B and in the columns [H, HP)
                if (col < H && g < B) {
                    const float av = P.a[g * H + col];
                    v = acc[t][r] * (1.0f - av * av);
                    P.dpre[g * H + col] = v;
                }
                dp_s[row][col] = v;
            }
        }
    }
    if (P.dfeat == nullptr) return;                                          // (uniform over the launch)
    __syncthreads();

    // 2. dfeat = -gamma (dpre W1): A = dpre rows from LDS, B = columns of W1; 32 column tiles per pass over the workgroup
    const float ng = -(P.d_gamma != nullptr ? P.d_gamma[0] : P.gamma);
    const int tiles = (F + 15) / 16;
    for (int base = 0; base < tiles; base += ADV_WAVES * ADV_TILES) {
        wgrad_f4 acc[ADV_TILES];
#pragma unroll
        for (int t = 0; t < ADV_TILES; ++t) acc[t] = adv_zero4();
        for (int k0 = 0; k0 < HP; k0 += 16) {
            const wgrad_f4 dv = *reinterpret_cast<const wgrad_f4*>(&dp_s[i][k0 + 4 * q]);
#pragma unroll
            for (int t = 0; t < ADV_TILES; ++t) {
                const int f0 = 16 * (base + wave + ADV_WAVES * t);
                if (f0 >= F) continue;                                       // (uniform over the wave)
                adv_stage(dv, adv_load_col4(P.W1, k0 + 4 * q, H, f0 + i, F), acc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < ADV_TILES; ++t) {
            const int col = 16 * (base + wave + ADV_WAVES * t) + i;
            if (col >= F) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t g = row0 + 4 * q + r;
                if (g < B) P.dfeat[g * P.ld_dfeat + col] = acc[t][r] * ng;
            }
        }
    }
}
