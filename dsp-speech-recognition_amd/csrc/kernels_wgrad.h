// The products between the recurrent backward kernels, bounded by a row count read on the device (include/dsp_frontend.h:
// dsp_rows_wgrad, dsp_rows_product).  fp32 on v_mfma_f32_16x16x4_f32: exact f32, every output element an fmaf chain in a
// fixed order.  gfx950 only.
//
//   rows_wgrad_kernel    C[m, n] = sum_{t < R, b < B} s[t, b] A[t, b, m] X[t + shift, b, n]   (and c[m] = sum A[t, b, m])
//                        one workgroup per (128 x 128 output tile, chunk of whole time steps counted from t = 0); a chunk
//                        that starts at or behind R exits at once; the others write their partial tile to scratch.
//   rows_wgrad_reduce_kernel   adds the partial tiles of the chunks below ceil(R / chunk) in index order: no atomics, no
//                        memset, no grid barrier.  The bits depend on (m, n, B, R) and the data, never on T.
//   rows_product_kernel  Y[t, b, :] = sum_p A_p[t, b, :] W_p for t < R, exact +0.0f for R <= t < T; every element written.
//
// LIMITS (checked on the host, csrc/dsp_wgrad.hip): m, n, k in [1, 2048]; T B < 2^31; every address is formed in int64;
// every pointer 4-byte aligned; operands have a unit column stride and non-negative t / b strides.  16-byte loads are
// taken where the pointer and both strides of an operand allow them; the values loaded, and so the bits, are the same.
// The kernels here are `static`: csrc/dsp_adv.hip launches the wgrad pair too, from a translation unit of its own.
//
// Tiling: 256 threads = 4 waves, each wave a 64 x 64 quarter of the tile as 4 x 4 MFMA tiles (64 accumulator registers).
// Both operands of a stage of WGRAD_KT rows lie in LDS as [row][128 columns]; lane (i = l & 15, k = l >> 4) reads the four
// columns 4 i .. 4 i + 3 of row k with ONE 16-byte LDS read per operand (the 16 lanes of a row cover all 64 banks once: no
// conflict) and feeds 16 MFMAs from the two reads: MFMA tile (ja, jb) owns output rows 4 (4 (l >> 4) + r) + ja and columns
// 4 (l & 15) + jb of the wave's quarter.  The next stage's global loads are issued before the MFMAs of this one.
// LDS: 2 x 16 x 128 x 4 B = 16 KiB per workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int WGRAD_TILE = 128;          // output tile edge
constexpr int WGRAD_KT = 16;             // rows of the reduced axis per LDS stage
constexpr int WGRAD_THREADS = 256;
constexpr int WGRAD_CHUNK_ROWS = 4096;   // a chunk holds about this many (t, b) rows ...
constexpr int WGRAD_CHUNK_T_MAX = 8;     // ... and at most this many time steps
constexpr int WGRAD_MAX_DIM = 2048;

// Time steps per chunk: a function of B alone, so the partition -- and with it the order of every sum -- ignores T.
__host__ __device__ inline int wgrad_chunk_steps(int B) {
    const int c = WGRAD_CHUNK_ROWS / B;
    return c < 1 ? 1 : (c > WGRAD_CHUNK_T_MAX ? WGRAD_CHUNK_T_MAX : c);
}

typedef float wgrad_f4 __attribute__((ext_vector_type(4)));

// The floats of scratch a dsp_rows_wgrad of these sizes needs: a partial tile per (chunk, tile) and the column-sum partials.
inline int64_t wgrad_scratch_floats(int32_t T, int32_t B, int32_t m, int32_t n) {
    const int steps = wgrad_chunk_steps(B);
    const int64_t chunks = (T + steps - 1) / steps;
    const int64_t tiles_m = (m + WGRAD_TILE - 1) / WGRAD_TILE, tiles_n = (n + WGRAD_TILE - 1) / WGRAD_TILE;
    return chunks * tiles_m * (tiles_n * WGRAD_TILE * WGRAD_TILE + WGRAD_TILE);
}

struct RowsOp {          // one [T, B, cols] view: element (t, b, c) at p[t st + b sb + c]
    const float* p;
    int64_t st, sb;
    int32_t cols;
    int32_t vec;         // p 16-byte aligned and st, sb multiples of 4: 16-byte loads allowed
};

__device__ inline int rows_bound(const int32_t* d_rows, int T) {
    if (!d_rows) return T;
    const int r = *d_rows;
    return r < 1 ? 1 : (r > T ? T : r);
}

// Columns c .. c + 3 of the row at `row` (NULL: zeros), zero where c + j >= cols.
__device__ inline wgrad_f4 rows_load4(const float* row, int c, int cols, bool vec) {
    wgrad_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!row) return v;
    if (vec && c + 3 < cols) return *reinterpret_cast<const wgrad_f4*>(row + c);
    if (c < cols) v.x = row[c];
    if (c + 1 < cols) v.y = row[c + 1];
    if (c + 2 < cols) v.z = row[c + 2];
    if (c + 3 < cols) v.w = row[c + 3];
    return v;
}

// The 16 k-steps x 16 MFMAs of one stage for the wave whose quarter starts at (wm0, wn0).
__device__ inline void rows_stage_mma(const float (*Ms)[WGRAD_TILE], const float (*Ns)[WGRAD_TILE], int wm0, int wn0, int lane,
                                      wgrad_f4 (&acc)[4][4]) {
    const int i4 = 4 * (lane & 15), kk = lane >> 4;
#pragma unroll
    for (int k0 = 0; k0 < WGRAD_KT; k0 += 4) {
        const wgrad_f4 a = *reinterpret_cast<const wgrad_f4*>(&Ms[k0 + kk][wm0 + i4]);
        const wgrad_f4 x = *reinterpret_cast<const wgrad_f4*>(&Ns[k0 + kk][wn0 + i4]);
#pragma unroll
        for (int ja = 0; ja < 4; ++ja)
#pragma unroll
            for (int jb = 0; jb < 4; ++jb)
                acc[ja][jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ja], x[jb], acc[ja][jb], 0, 0, 0);
    }
}

// grid (tiles_m * tiles_n, ceil(T / chunk)); part: [chunk][tile][128][128]; cpart: [chunk][tile_m][128] or NULL.
static __global__ __launch_bounds__(WGRAD_THREADS) void rows_wgrad_kernel(RowsOp A, RowsOp X, int shift, const float* __restrict__ init,
                                                                   int64_t init_sb, const float* __restrict__ scale, int T, int B,
                                                                   const int32_t* __restrict__ d_rows, int tiles_n,
                                                                   float* __restrict__ part, float* __restrict__ cpart) {
    __shared__ __attribute__((aligned(16))) float As[WGRAD_KT][WGRAD_TILE];
    __shared__ __attribute__((aligned(16))) float Xs[WGRAD_KT][WGRAD_TILE];
    const int R = rows_bound(d_rows, T);
    const int steps = wgrad_chunk_steps(B);
    const int t0 = blockIdx.y * steps;
    if (t0 >= R) return;                                                   // nothing behind R is read or written
    const int nt = R - t0 < steps ? R - t0 : steps;
    const int rows = nt * B;                                               // <= WGRAD_CHUNK_T_MAX * B
    const int tile = blockIdx.x, tm = tile / tiles_n, tn = tile % tiles_n;
    const int m0 = tm * WGRAD_TILE, n0 = tn * WGRAD_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int lr = tid >> 5, c4 = (tid & 31) * 4;                          // staging: rows lr and lr + 8, columns c4 .. c4 + 3
    const bool want_c = cpart != nullptr && tn == 0;

    wgrad_f4 acc[4][4];
#pragma unroll
    for (int ja = 0; ja < 4; ++ja)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) acc[ja][jb] = wgrad_f4{0.0f, 0.0f, 0.0f, 0.0f};
    float csum = 0.0f;

    wgrad_f4 ra[2], rx[2];
    auto fetch = [&](int s) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int g = s * WGRAD_KT + lr + 8 * p;
            ra[p] = wgrad_f4{0.0f, 0.0f, 0.0f, 0.0f};
            rx[p] = ra[p];
            if (g < rows) {
                const int t = t0 + g / B, b = g % B;
                ra[p] = rows_load4(A.p + (int64_t)t * A.st + (int64_t)b * A.sb, m0 + c4, A.cols, A.vec != 0);
                const int tx = t + shift;
                const float* xr = nullptr;
                if (tx < 0) xr = init ? init + (int64_t)b * init_sb : nullptr;
                else if (tx < R) xr = X.p + (int64_t)tx * X.st + (int64_t)b * X.sb;
                rx[p] = rows_load4(xr, n0 + c4, X.cols, X.vec != 0);
                if (scale) rx[p] *= scale[(int64_t)t * B + b];
            }
        }
    };

    const int stages = (rows + WGRAD_KT - 1) / WGRAD_KT;
    fetch(0);
    for (int s = 0; s < stages; ++s) {
        __syncthreads();                                                   // the MFMAs of the stage before are done with LDS
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            *reinterpret_cast<wgrad_f4*>(&As[lr + 8 * p][c4]) = ra[p];
            *reinterpret_cast<wgrad_f4*>(&Xs[lr + 8 * p][c4]) = rx[p];
        }
        __syncthreads();
        if (s + 1 < stages) fetch(s + 1);
        if (want_c && tid < WGRAD_TILE) {
#pragma unroll
            for (int k = 0; k < WGRAD_KT; ++k) csum += As[k][tid];
        }
        rows_stage_mma(As, Xs, wm0, wn0, lane, acc);
    }

    float* out = part + ((int64_t)blockIdx.y * gridDim.x + tile) * (WGRAD_TILE * WGRAD_TILE);
    const int i4 = 4 * (lane & 15), q = lane >> 4;
#pragma unroll
    for (int ja = 0; ja < 4; ++ja)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ml = wm0 + 4 * (4 * q + r) + ja;
            const wgrad_f4 v = {acc[ja][0][r], acc[ja][1][r], acc[ja][2][r], acc[ja][3][r]};
            *reinterpret_cast<wgrad_f4*>(out + ml * WGRAD_TILE + wn0 + i4) = v;
        }
    if (want_c && tid < WGRAD_TILE) cpart[((int64_t)blockIdx.y * (gridDim.x / tiles_n) + tm) * WGRAD_TILE + tid] = csum;
}

// One thread per element of C [m, n] and then of c [m]: the partials of the chunks below ceil(R / chunk), in index order.
static __global__ __launch_bounds__(256) void rows_wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ cpart, int m, int n,
                                                                int tiles_m, int tiles_n, int T, int B, const int32_t* __restrict__ d_rows,
                                                                float* __restrict__ C, float* __restrict__ csum) {
    const int R = rows_bound(d_rows, T);
    const int steps = wgrad_chunk_steps(B);
    const int chunks = (R + steps - 1) / steps;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t mn = (int64_t)m * n;
    if (e < mn) {
        const int mi = (int)(e / n), ni = (int)(e % n);
        const int tile = (mi / WGRAD_TILE) * tiles_n + ni / WGRAD_TILE;
        const int64_t stride = (int64_t)tiles_m * tiles_n * (WGRAD_TILE * WGRAD_TILE);
        const float* p = part + (int64_t)tile * (WGRAD_TILE * WGRAD_TILE) + (mi % WGRAD_TILE) * WGRAD_TILE + ni % WGRAD_TILE;
        float s = p[0];
        for (int c = 1; c < chunks; ++c) s += p[c * stride];
        C[e] = s;
    } else if (csum && e < mn + m) {
        const int mi = (int)(e - mn);
        const int64_t stride = (int64_t)tiles_m * WGRAD_TILE;
        const float* p = cpart + mi;                                       // [chunk][tile_m][128] is [chunk][tiles_m * 128]
        float s = p[0];
        for (int c = 1; c < chunks; ++c) s += p[c * stride];
        csum[mi] = s;
    }
}

struct RowsTerm {        // one product A [T, B, k] W [k, n]
    RowsOp a;
    const float* w;
    int32_t wvec;        // w 16-byte aligned and n a multiple of 4
};

// grid (ceil(T B / 128), ceil(n / 128)); Y dense [T B, n].
static __global__ __launch_bounds__(WGRAD_THREADS) void rows_product_kernel(RowsTerm P0, RowsTerm P1, int nterms, int n, int T, int B,
                                                                     const int32_t* __restrict__ d_rows, float* __restrict__ Y, int yvec) {
    __shared__ __attribute__((aligned(16))) float As[WGRAD_KT][WGRAD_TILE];   // [k][row of the tile]: transposed while staged
    __shared__ __attribute__((aligned(16))) float Ws[WGRAD_KT][WGRAD_TILE];   // [k][column]
    const int R = rows_bound(d_rows, T);
    const int64_t total = (int64_t)T * B, valid = (int64_t)R * B;
    const int64_t row0 = (int64_t)blockIdx.x * WGRAD_TILE;
    const int n0 = blockIdx.y * WGRAD_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int i4 = 4 * (lane & 15), q = lane >> 4;

    wgrad_f4 acc[4][4];
#pragma unroll
    for (int ja = 0; ja < 4; ++ja)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) acc[ja][jb] = wgrad_f4{0.0f, 0.0f, 0.0f, 0.0f};

    if (row0 < valid) {                                                    // a tile behind R reads nothing
        const int rl = tid & 127, kh = (tid >> 7) * 8;                     // A: row rl of the tile, k kh .. kh + 7 of the stage
        const int wr = tid >> 5, c4 = (tid & 31) * 4;                      // W: rows wr and wr + 8 of the stage, columns c4 .. c4 + 3
        const int64_t g = row0 + rl;
        const bool live = g < valid;
        const int t = live ? (int)(g / B) : 0, b = live ? (int)(g % B) : 0;
        for (int term = 0; term < nterms; ++term) {
            const RowsTerm& P = term == 0 ? P0 : P1;
            const float* arow = live ? P.a.p + (int64_t)t * P.a.st + (int64_t)b * P.a.sb : nullptr;
            const int K = P.a.cols;
            wgrad_f4 ra[2], rw[2];
            auto fetch = [&](int k0) {
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    ra[p] = rows_load4(arow, k0 + kh + 4 * p, K, P.a.vec != 0);
                    const int kr = k0 + wr + 8 * p;
                    rw[p] = rows_load4(kr < K ? P.w + (int64_t)kr * n : nullptr, n0 + c4, n, P.wvec != 0);
                }
            };
            fetch(0);
            for (int k0 = 0; k0 < K; k0 += WGRAD_KT) {
                __syncthreads();
#pragma unroll
                for (int p = 0; p < 2; ++p) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) As[kh + 4 * p + j][rl] = ra[p][j];
                    *reinterpret_cast<wgrad_f4*>(&Ws[wr + 8 * p][c4]) = rw[p];
                }
                __syncthreads();
                if (k0 + WGRAD_KT < K) fetch(k0 + WGRAD_KT);
                rows_stage_mma(As, Ws, wm0, wn0, lane, acc);
            }
        }
    }

#pragma unroll
    for (int ja = 0; ja < 4; ++ja)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t g = row0 + wm0 + 4 * (4 * q + r) + ja;
            if (g >= total) continue;
            const int c = n0 + wn0 + i4;
            wgrad_f4 v = {acc[ja][0][r], acc[ja][1][r], acc[ja][2][r], acc[ja][3][r]};
            if (g >= valid) v = wgrad_f4{0.0f, 0.0f, 0.0f, 0.0f};          // exact +0.0f behind R
            float* y = Y + g * n + c;
            if (yvec && c + 3 < n) *reinterpret_cast<wgrad_f4*>(y) = v;
            else {
                if (c < n) y[0] = v.x;
                if (c + 1 < n) y[1] = v.y;
                if (c + 2 < n) y[2] = v.z;
                if (c + 3 < n) y[3] = v.w;
            }
        }
}
