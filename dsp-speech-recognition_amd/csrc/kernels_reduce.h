// The column sums of the training step, bounded by a row count read on the device (include/dsp_frontend.h: dsp_rows_colsum).
// fp32, a fixed order: the sums torch forms with multi-workgroup reductions (a.sum(0).sum(0), (g * n).sum(0).sum(0), g.sum(0),
// g.sum()) as two launches without atomics, memset or a grid barrier.  gfx950 only.
//
//   rows_colsum_wide_kernel    cols >= 64: lanes along columns.  One workgroup per (block of 64 columns, chunk of
//                              wgrad_chunk_steps(B) whole time steps counted from t = 0).  Thread (cg = tid & 15, rg = tid >> 4)
//                              owns columns 4 cg .. 4 cg + 3 of the block and the chunk's rows rg, rg + 16, ..; the 16 row
//                              groups meet in LDS and are added in index order.
//   rows_colsum_narrow_kernel  cols < 64: lanes along rows.  One workgroup per (block of 8 columns, chunk).  Thread tid owns
//                              the chunk's rows tid, tid + 256, ..; a wave adds its 64 lanes by the xor tree 32, 16, 8, 4, 2,
//                              1 (every lane ends with the same bits), the 4 waves meet in LDS and are added in index order.
//   rows_colsum_reduce_kernel  one thread per column: the partials of the chunks below ceil(R / chunk), in index order.
//
// A chunk that starts at or behind R exits at once: nothing at t >= R is read.  A (t, b) row of the chunk that starts at t0 is
// g = (t - t0) B + b, so which thread adds which row -- the partition and the order of every sum -- is a function of (B, cols)
// alone; T does not enter.  With a second operand the term is a[t, b, c] * x[t, b, c], rounded to fp32 BEFORE it is added (no
// contraction into an fma): tools/rows_sum_emul.py restates the arithmetic in NumPy fp32, bit for bit.
//
// Memory-bound: every element is read once.  The wide kernel's 16 lanes of a row group read 256 contiguous bytes of one row with
// 16-byte loads where the operand allows them (rows_load4 of kernels_wgrad.h: the same values, and so the same bits, from a
// 4-byte-aligned view); the narrow kernel's lanes read consecutive rows, which for cols = 1 over a [T, B] view (stride_b = 1) is
// one contiguous run per wave.  LDS: 4 KiB (wide), 128 B (narrow).  LIMITS as kernels_wgrad.h; checked in csrc/dsp_reduce.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_wgrad.h"

constexpr int COLSUM_THREADS = 256;
constexpr int COLSUM_WIDE_MIN = 64;      // cols >= this: lanes along columns
constexpr int COLSUM_WIDE_COLS = 64;     // columns per workgroup, wide kernel (16 lanes x 4)
constexpr int COLSUM_WIDE_ROWGROUPS = COLSUM_THREADS / 16;
constexpr int COLSUM_NARROW_COLS = 8;    // columns per workgroup, narrow kernel

// The floats of scratch a dsp_rows_colsum of these sizes needs: one partial per (chunk, column).
inline int64_t colsum_scratch_floats(int32_t T, int32_t B, int32_t cols) {
    const int steps = wgrad_chunk_steps(B);
    const int64_t chunks = (T + steps - 1) / steps;
    return (chunks * cols + 3) & ~(int64_t)3;
}

inline int colsum_col_blocks(int32_t cols) {
    const int per = cols >= COLSUM_WIDE_MIN ? COLSUM_WIDE_COLS : COLSUM_NARROW_COLS;
    return (cols + per - 1) / per;
}

// a[t, b, c .. c + 3] (* x[t, b, c .. c + 3]), zero where c + j >= cols.
__device__ inline wgrad_f4 colsum_term4(const RowsOp& A, const RowsOp& X, bool has_x, int t, int b, int c) {
    wgrad_f4 v = rows_load4(A.p + (int64_t)t * A.st + (int64_t)b * A.sb, c, A.cols, A.vec != 0);
    if (has_x) {
        const wgrad_f4 w = rows_load4(X.p + (int64_t)t * X.st + (int64_t)b * X.sb, c, X.cols, X.vec != 0);
        float p0 = v.x * w.x, p1 = v.y * w.y, p2 = v.z * w.z, p3 = v.w * w.w;
        // the products pass through an empty asm statement, so that -ffp-contract=fast cannot fuse them into the sums behind
        asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));
        v = wgrad_f4{p0, p1, p2, p3};
    }
    return v;
}

// grid (ceil(cols / 64), ceil(T / chunk)); part: [chunk][cols].
static __global__ __launch_bounds__(COLSUM_THREADS) void rows_colsum_wide_kernel(RowsOp A, RowsOp X, int has_x, int T, int B,
                                                                                 const int32_t* __restrict__ d_rows,
                                                                                 float* __restrict__ part) {
    __shared__ float red[COLSUM_WIDE_ROWGROUPS][COLSUM_WIDE_COLS];
    const int R = rows_bound(d_rows, T);
    const int steps = wgrad_chunk_steps(B);
    const int t0 = blockIdx.y * steps;
    if (t0 >= R) return;                                                   // nothing behind R is read or written
    const int nt = R - t0 < steps ? R - t0 : steps;
    const int rows = nt * B;                                               // <= WGRAD_CHUNK_T_MAX * B
    const int tid = threadIdx.x, cg = tid & 15, rg = tid >> 4;
    const int cols = A.cols, c0 = blockIdx.x * COLSUM_WIDE_COLS + 4 * cg;

    wgrad_f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c0 < cols) {
        // (t, b) of row g advance with it: one division per thread, none per row
        const int dt = COLSUM_WIDE_ROWGROUPS / B, db = COLSUM_WIDE_ROWGROUPS % B;
        int t = t0 + rg / B, b = rg % B;
        for (int g = rg; g < rows; g += COLSUM_WIDE_ROWGROUPS) {
            const wgrad_f4 v = colsum_term4(A, X, has_x != 0, t, b, c0);
            acc.x += v.x;
            acc.y += v.y;
            acc.z += v.z;
            acc.w += v.w;
            t += dt;
            b += db;
            if (b >= B) {
                b -= B;
                ++t;
            }
        }
    }
    red[rg][4 * cg] = acc.x;
    red[rg][4 * cg + 1] = acc.y;
    red[rg][4 * cg + 2] = acc.z;
    red[rg][4 * cg + 3] = acc.w;
    __syncthreads();
    const int c = blockIdx.x * COLSUM_WIDE_COLS + tid;
    if (tid < COLSUM_WIDE_COLS && c < cols) {
        float s = red[0][tid];
#pragma unroll
        for (int k = 1; k < COLSUM_WIDE_ROWGROUPS; ++k) s += red[k][tid];
        part[(int64_t)blockIdx.y * cols + c] = s;
    }
}

// grid (ceil(cols / 8), ceil(T / chunk)); part: [chunk][cols].
static __global__ __launch_bounds__(COLSUM_THREADS) void rows_colsum_narrow_kernel(RowsOp A, RowsOp X, int has_x, int T, int B,
                                                                                   const int32_t* __restrict__ d_rows,
                                                                                   float* __restrict__ part) {
    __shared__ float red[COLSUM_THREADS / 64][COLSUM_NARROW_COLS];
    const int R = rows_bound(d_rows, T);
    const int steps = wgrad_chunk_steps(B);
    const int t0 = blockIdx.y * steps;
    if (t0 >= R) return;
    const int nt = R - t0 < steps ? R - t0 : steps;
    const int rows = nt * B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cols = A.cols, c0 = blockIdx.x * COLSUM_NARROW_COLS;

    float acc[COLSUM_NARROW_COLS];
#pragma unroll
    for (int j = 0; j < COLSUM_NARROW_COLS; ++j) acc[j] = 0.0f;
    const int dt = COLSUM_THREADS / B, db = COLSUM_THREADS % B;
    int t = t0 + tid / B, b = tid % B;
    for (int g = tid; g < rows; g += COLSUM_THREADS, t += dt, b += db) {
        if (b >= B) {                                                      // the carry of the step before
            b -= B;
            ++t;
        }
        const wgrad_f4 lo = colsum_term4(A, X, has_x != 0, t, b, c0);
        acc[0] += lo.x;
        acc[1] += lo.y;
        acc[2] += lo.z;
        acc[3] += lo.w;
        if (c0 + 4 < cols) {                                               // uniform over the workgroup
            const wgrad_f4 hi = colsum_term4(A, X, has_x != 0, t, b, c0 + 4);
            acc[4] += hi.x;
            acc[5] += hi.y;
            acc[6] += hi.z;
            acc[7] += hi.w;
        }
    }
#pragma unroll
    for (int j = 0; j < COLSUM_NARROW_COLS; ++j) {
        float s = acc[j];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);       // a + b == b + a: every lane holds the same bits
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    if (tid < COLSUM_NARROW_COLS && c0 + tid < cols) {
        float s = red[0][tid];
#pragma unroll
        for (int w = 1; w < COLSUM_THREADS / 64; ++w) s += red[w][tid];
        part[(int64_t)blockIdx.y * cols + c0 + tid] = s;
    }
}

// One thread per column: the partials of the chunks below ceil(R / chunk), in index order.  Every element of out is written.
static __global__ __launch_bounds__(256) void rows_colsum_reduce_kernel(const float* __restrict__ part, int cols, int T, int B,
                                                                        const int32_t* __restrict__ d_rows, float* __restrict__ out) {
    const int R = rows_bound(d_rows, T);
    const int steps = wgrad_chunk_steps(B);
    const int chunks = (R + steps - 1) / steps;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    float s = part[c];
    for (int k = 1; k < chunks; ++k) s += part[(int64_t)k * cols + c];
    out[c] = s;
}
