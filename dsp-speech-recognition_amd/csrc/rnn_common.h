// The matrix-pipe core of the recurrent kernels (kernels_hmlstm*.h, kernels_bigru*.h): the workgroup's shape, the product loop
// over the packed weight layout, and the pieces every cell built on them repeats.  The hm_ / HM_ prefix is historical.
#pragma once

#include <type_traits>

#include "dsp_common.h"

#define HM_COLS 16          // batch columns per workgroup = N of the 16x16x4 product
#define HM_WAVES 8          // 512 threads: two waves per SIMD, so dependent accumulators never stall the matrix pipe
#define HM_THREADS (HM_WAVES * 64)
#define HM_CHUNK 4          // tiles a wave accumulates side by side: independent accumulators, one read of the LDS operand

typedef float hm_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) hm_f32x4 hm_gf4;   // four floats in global memory
typedef __attribute__((address_space(3))) hm_f32x4 hm_lf4;   // four floats in LDS
typedef __attribute__((address_space(1))) const float hm_gf; // a float in global memory, read only
typedef __attribute__((address_space(1))) float hm_gfw;      // ... written

static inline int32_t hm_kgroups(int32_t k) { return (k + 15) >> 4; }      // K padded to 16: four products per packed float4
static inline int32_t hm_slices(int32_t B) { return (B + HM_COLS - 1) / HM_COLS; }
// chunks of four owner slots a wave needs for H units: H / 4 gate tiles over 8 waves, four slots per M tile
__host__ __device__ static inline int32_t hm_bwd_chunks(int32_t H) { return (((H >> 2) + HM_WAVES - 1) / HM_WAVES + 3) >> 2; }

// Float i of a packed matrix (nt tiles per k-group) -> element e of lane l's float4, tile t, k-group g, the K index k it holds.
struct HmPackIdx { int32_t e, l, t, g, k; };
__device__ __forceinline__ HmPackIdx hm_pack_idx(int64_t i, int32_t nt) {
    const int64_t gt = i >> 8;
    const int32_t e = (int32_t)(i & 3), l = (int32_t)((i >> 2) & 63), t = (int32_t)(gt % nt), g = (int32_t)(gt / nt);
    return HmPackIdx{e, l, t, g, 16 * g + 4 * (l >> 4) + e};
}
// The transposed packings: row i = l & 15 of M tile tt = 8 c + w holds m = 4 (w + 8 (4 c + (i & 3))) + (i >> 2).
__device__ __forceinline__ int32_t hm_pack_t_m(int32_t tt, int32_t l) {
    const int32_t ii = l & 15;
    return 4 * ((tt & 7) + 8 * (4 * (tt >> 3) + (ii & 3))) + (ii >> 2);
}

// float index of element (k, col) of an LDS operand buffer: lane l of k-group g reads the float4 at 64 g + l
__device__ __forceinline__ int hm_idx(int k, int col) { return (((k >> 2) * HM_COLS + col) << 2) + (k & 3); }

__device__ __forceinline__ float hm_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// A wave-uniform address, taken through readfirstlane and so held in scalar registers: the loads below are then "scalar base
// + the lane's own offset", and the per-slot addresses are not carried in vector registers across the step loop (which
// spills; see hm_product).  Used by the training mode and by the backward kernels.
template <class Tp>
__device__ __forceinline__ Tp* hm_uniform(Tp* p) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return reinterpret_cast<Tp*>(((uint64_t)hi << 32) | lo);
}

// acc[i] = (packed segment) x (LDS operand) for the N tiles t0, t0 + 8, ..  Two k-groups per trip through two register
// sets: the weights of the next k-group are in flight while the products of this one issue (L2 latency behind the matrix pipe).
template <int N>
__device__ __forceinline__ void hm_mfma4(hm_f32x4 (&acc)[HM_CHUNK], const hm_f32x4 (&a)[N], const hm_f32x4 b) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b.x, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b.y, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b.z, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b.w, acc[i], 0, 0, 0);
    }
}

template <int N>
__device__ __forceinline__ void hm_product(hm_f32x4 (&acc)[HM_CHUNK], const float4* __restrict__ wp, int ng, int nt,
                                           const float* lds_b, int t0, int lane) {
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = hm_f32x4{0.f, 0.f, 0.f, 0.f};
    const hm_lf4* lb = (const hm_lf4*)lds_b + lane;     // explicitly LDS: a generic pointer costs flat loads, which wait for every counter
    // The start address is wave-uniform and made opaque to the optimiser: otherwise the start addresses of every product of
    // both cells are hoisted out of the step loop and held in vector registers across it, which spills at 7 tiles per wave.
    // It goes back to a pointer into GLOBAL memory (a generic one costs flat loads, which wait for every counter).
    uint64_t wa = reinterpret_cast<uint64_t>(wp + (size_t)t0 * 64);
    asm volatile("" : "+s"(wa));
    const hm_gf4* wg = (const hm_gf4*)wa;
    const size_t stride = (size_t)nt * 64;
    const unsigned l = (unsigned)lane;
    hm_f32x4 a0[N], a1[N];
#pragma unroll
    for (int i = 0; i < N; ++i) a0[i] = wg[l + HM_WAVES * i * 64];
    int g = 0;
    for (; g + 1 < ng; g += 2) {
        const hm_gf4* w1 = wg + stride;
#pragma unroll
        for (int i = 0; i < N; ++i) a1[i] = w1[l + HM_WAVES * i * 64];
        __builtin_amdgcn_sched_barrier(0);          // the requests stay in front of the products they overlap with
        hm_mfma4<N>(acc, a0, lb[g * 64]);
        __builtin_amdgcn_sched_barrier(0);
        wg += (g + 2 < ng) ? 2 * stride : 0;        // behind the last k-group: re-request one already held (no branch, no read past the segment)
#pragma unroll
        for (int i = 0; i < N; ++i) a0[i] = wg[l + HM_WAVES * i * 64];
        __builtin_amdgcn_sched_barrier(0);
        hm_mfma4<N>(acc, a1, lb[(g + 1) * 64]);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (g < ng) hm_mfma4<N>(acc, a0, lb[g * 64]);
}

// A cell's walk over this wave's tiles w, w + 8, .. in chunks of HM_CHUNK: product(integral_constant<int, N>, acc, t0) fills a
// fresh Acc for the N = 4 / 3 / 2 / 1 tiles from t0 on (what the chunk holds and the wave has left), then tile(acc, i, s, t) runs
// for accumulator i = owner slot s = tile t of each.  w is wave-uniform, so the tile counts are scalar branches.
template <int MAXS, class Acc, class Product, class Tile>
__device__ __forceinline__ void hm_for_chunks(int nt, int w, Product&& product, Tile&& tile) {
#pragma unroll
    for (int s0 = 0; s0 < MAXS; s0 += HM_CHUNK) {
        const int t0 = w + HM_WAVES * s0;
        if (t0 >= nt) break;
        const int CAP = MAXS - s0 < HM_CHUNK ? MAXS - s0 : HM_CHUNK;          // tiles this chunk can hold (folds when unrolled)
        const int left = (nt - t0 + HM_WAVES - 1) / HM_WAVES;                   // tiles of this wave from t0 on
        Acc acc;
        if (CAP >= 4 && left >= 4) product(std::integral_constant<int, 4>{}, acc, t0);
        else if (CAP >= 3 && left >= 3) product(std::integral_constant<int, 3>{}, acc, t0);
        else if (CAP >= 2 && left >= 2) product(std::integral_constant<int, 2>{}, acc, t0);
        else product(std::integral_constant<int, 1>{}, acc, t0);
#pragma unroll
        for (int i = 0; i < HM_CHUNK; ++i) {
            const int s = s0 + i, t = t0 + HM_WAVES * i;
            if (i < CAP && t < nt) tile(acc, i, s, t);
        }
    }
}

// acc (as slots) = (packed transposed matrix) x dfs for this wave's M tiles w, w + 8
template <int NC>
__device__ __forceinline__ void hm_bwd_product(float (&r)[4 * NC], const float4* wp, int ng, int nc, const float* dfs, int w, int lane) {
    hm_f32x4 acc[HM_CHUNK];
    if (NC >= 2 && nc >= 2) hm_product<2>(acc, wp, ng, HM_WAVES * 2, dfs, w, lane);
    else {
        hm_product<1>(acc, wp, ng, HM_WAVES, dfs, w, lane);
        if (NC >= 2) acc[1] = hm_f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) { r[4 * c] = acc[c].x; r[4 * c + 1] = acc[c].y; r[4 * c + 2] = acc[c].z; r[4 * c + 3] = acc[c].w; }
}

// The owner lane's four gate gradients of tile tl, v0 .. v3 in row order, to out + {0, H, 2 H, 3 H} + 4 tl (uniform) + lo (the lane's).
__device__ __forceinline__ void hm_store_gate_grads(float* out, int H, int tl, int lo, float v0, float v1, float v2, float v3) {
    ((hm_gfw*)hm_uniform(out + 4 * tl))[lo] = v0;
    ((hm_gfw*)hm_uniform(out + H + 4 * tl))[lo] = v1;
    ((hm_gfw*)hm_uniform(out + 2 * H + 4 * tl))[lo] = v2;
    ((hm_gfw*)hm_uniform(out + 3 * H + 4 * tl))[lo] = v3;
}

// The lengths of a slice's columns, clamped to [1, T], into lens[HM_COLS] (0: a column that does not exist is never active),
// a barrier, and -- wave-uniform -- the steps the slice runs: the largest of them.
__device__ __forceinline__ int hm_slice_steps(const int32_t* len, int b0, int B, int T, int* lens) {
    if (threadIdx.x < HM_COLS) {
        const int bb = b0 + threadIdx.x;
        lens[threadIdx.x] = bb >= B ? 0 : len ? min(max(len[bb], 1), T) : T;
    }
    __syncthreads();
    int steps = 0;
#pragma unroll
    for (int c = 0; c < HM_COLS; ++c) steps = max(steps, lens[c]);
    return __builtin_amdgcn_readfirstlane(steps);
}

// The row bound of the HM-LSTM's training pair: T without one, else the word at `rows` clamped to [1, T] -- one wave-uniform
// read, held in a scalar register.  Whatever the word holds, the result is in [1, T]: no index and no loop bound derived
// from it leaves what the argument T allows.
__device__ __forceinline__ int hm_row_bound(const int32_t* rows, int T) {
    if (!rows) return T;
    return min(max(__builtin_amdgcn_readfirstlane(*rows), 1), T);
}

// Exact zeros behind row R of a [B, T, H] output (H a multiple of 4) for the slice's columns b0 .. : per column the
// (T - R) H floats from (b T + R) H on are contiguous, so they go out as 16-byte stores where the buffer's base allows.
__device__ __forceinline__ void hm_zero_tail_bth(float* out, int H, int R, int T, int b0, int B) {
    const int cols = min(HM_COLS, B - b0), n = (T - R) * H;
    if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        const int n4 = n >> 2;
        for (int idx = threadIdx.x; idx < cols * n4; idx += HM_THREADS) {
            const int c = idx / n4, j = idx - c * n4;
            ((hm_gf4*)(out + ((int64_t)(b0 + c) * T + R) * H))[j] = hm_f32x4{0.f, 0.f, 0.f, 0.f};
        }
    } else {
        for (int idx = threadIdx.x; idx < cols * n; idx += HM_THREADS) {
            const int c = idx / n, j = idx - c * n;
            out[((int64_t)(b0 + c) * T + R) * H + j] = 0.f;
        }
    }
}

// Exact zeros in the rows of the steps no column of the slice reaches (t in [steps, T)): per step and column of the slice
// `width` floats at out[(t * B + b) * stride + off ..].
__device__ __forceinline__ void hm_zero_rows(float* out, int width, int stride, int off, int steps, int T, int b0, int B) {
    const int n = min(HM_COLS, B - b0) * width;
    for (int t = steps; t < T; ++t) {
        float* row = out + ((int64_t)t * B + b0) * stride + off;
        for (int idx = threadIdx.x; idx < n; idx += HM_THREADS) {
            const int c = idx / width, j = idx - c * width;
            row[c * stride + j] = 0.f;
        }
    }
}
