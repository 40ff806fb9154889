// Reproducible dropout (include/dsp_frontend.h: dsp_rng_advance, dsp_dropout_*): a counter-based generator whose whole state is
// {seed, step}, two int64 words in device memory.  A multiplier is a pure function of (seed, step, site, element index):
//   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written from the paper's
//   round function;  key = (seed_lo, seed_hi);  counter = (element_index / 4, step_lo, step_hi, site);  the four output words
//   serve elements 4 block .. 4 block + 3 in order;  kept iff (word >> 8) < thr, thr = llrint((1 - p) 2^24) formed on the host.
// element_index is the row-major index into the LOGICAL tensor: no row bound, alignment or launch shape moves a draw.  A kept
// element is x * scale (one fp32 product), a dropped one exact +0.0f; thr = 2^24 (p = 0) copies the input's bits and draws
// nothing.  The state is read when a launch RUNS, so a recorded launch follows dsp_rng_advance.  No atomics, no LDS, no memset;
// every element belongs to exactly one lane: the same bits on every run.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define DROPOUT_THREADS 256
#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

struct Philox4 {
    uint32_t w[4];
};

// Ten rounds; the key is bumped between rounds (nine times).  The 64-bit products leave the choice of the multiply form
// (one 32 x 32 -> 64 multiply-add, or a low and a high multiply) to the compiler.
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// What one draw site of one step is keyed by, read from the state (or a saved key) once per lane: wave-uniform loads.
struct DropKey {
    uint32_t k0, k1, s0, s1;
};

__device__ __forceinline__ DropKey drop_key(long long s_seed, long long s_step) {
    const unsigned long long seed = (unsigned long long)s_seed, step = (unsigned long long)s_step;
    return DropKey{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32)};
}

__device__ __forceinline__ float drop_one(float x, uint32_t word, uint32_t thr, float scale) { return (word >> 8) < thr ? x * scale : 0.0f; }

// <<<1, 1>>>: the one place the step count moves.
__global__ void rng_advance_kernel(long long* state) { state[1] = state[1] + 1; }

// y = x * m over n elements; a lane takes whole blocks of four elements.  WIDE: x and y are 16-byte aligned, so a block inside
// n is one 16-byte load and one 16-byte store; the tail block and every block of a misaligned view go element by element.
// y == x is served: a lane reads its block before it writes it.  key_out: NULL, or two words that receive the {seed, step} used.
template <bool WIDE>
__global__ __launch_bounds__(DROPOUT_THREADS) void dropout_apply_kernel(const float* x, float* y, long long n, uint32_t thr, float scale, uint32_t site,
                                                                        const long long* __restrict__ state, long long* key_out) {
    const long long s_seed = state[0], s_step = state[1];
    if (key_out && blockIdx.x == 0 && threadIdx.x == 0) {
        key_out[0] = s_seed;
        key_out[1] = s_step;
    }
    const DropKey k = drop_key(s_seed, s_step);
    const bool copy = thr >= (1u << 24);                         // p = 0: the input's bits, nothing drawn
    const long long nblk = (n + 3) >> 2;
    for (long long b = (long long)blockIdx.x * DROPOUT_THREADS + threadIdx.x; b < nblk; b += (long long)gridDim.x * DROPOUT_THREADS) {
        const long long e = b << 2;
        if (copy) {
            if (x == y) continue;
            if (WIDE && e + 4 <= n) {
                reinterpret_cast<uint4*>(y)[b] = reinterpret_cast<const uint4*>(x)[b];
            } else {
                for (int i = 0; i < 4 && e + i < n; ++i) reinterpret_cast<uint32_t*>(y)[e + i] = reinterpret_cast<const uint32_t*>(x)[e + i];
            }
            continue;
        }
        const Philox4 r = philox4x32_10((uint32_t)b, k.s0, k.s1, site, k.k0, k.k1);
        if (WIDE && e + 4 <= n) {
            const float4 v = reinterpret_cast<const float4*>(x)[b];
            reinterpret_cast<float4*>(y)[b] = make_float4(drop_one(v.x, r.w[0], thr, scale), drop_one(v.y, r.w[1], thr, scale),
                                                          drop_one(v.z, r.w[2], thr, scale), drop_one(v.w, r.w[3], thr, scale));
        } else {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = e + i < n ? x[e + i] : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e + i < n) y[e + i] = drop_one(v[i], r.w[i], thr, scale);
        }
    }
}

// The multipliers [L, T, B, C] of dsp_bigru_forward_train's d_drop: layer l is keyed by site_base + l, element_index runs over
// [T, B, C].  Elements of rows t < R = clamp(*rows, 1, T) (T when rows is NULL) are drawn; every element behind is written as
// exact +0.0f by a plain store, and a block that lies wholly behind the bound draws nothing.  per_layer = T B C, row = B C.
// WIDE: m is 16-byte aligned and per_layer % 4 == 0, so every block is one 16-byte store.
template <bool WIDE>
__global__ __launch_bounds__(DROPOUT_THREADS) void dropout_multipliers_kernel(float* __restrict__ m, int32_t T, long long per_layer, long long row,
                                                                              uint32_t thr, float scale, uint32_t site_base,
                                                                              const long long* __restrict__ state, const int32_t* __restrict__ rows) {
    const DropKey k = drop_key(state[0], state[1]);
    int32_t R = T;
    if (rows) {
        R = rows[0];
        R = R < 1 ? 1 : (R > T ? T : R);
    }
    const long long bound = (long long)R * row;                  // elements of a layer that are drawn
    const long long nblk = (per_layer + 3) >> 2;
    const uint32_t l = blockIdx.y;                               // the grid's y extent is L
    for (long long b = (long long)blockIdx.x * DROPOUT_THREADS + threadIdx.x; b < nblk; b += (long long)gridDim.x * DROPOUT_THREADS) {
        const long long e = b << 2;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (e < bound) {
            const Philox4 r = philox4x32_10((uint32_t)b, k.s0, k.s1, site_base + l, k.k0, k.k1);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = e + i < bound ? drop_one(1.0f, r.w[i], thr, scale) : 0.0f;
        }
        float* out = m + l * per_layer;
        if (WIDE) {
            reinterpret_cast<float4*>(out)[b] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e + i < per_layer) out[e + i] = v[i];
        }
    }
}
