// Forward pass of the reference's hierarchical-multiscale LSTM (hmrnn.py:47-154: HM_LSTM over two HM_LSTMCell) for a
// whole batch, fp32, as ONE persistent launch.
//
// Shape.  The recurrence is independent per utterance (batch column), so a workgroup owns a slice of HM_COLS = 16 columns,
// runs all T steps for it (fewer when only h_2 at len - 1 is asked for, see the step loop) and never waits on another
// workgroup: no grid barrier, no flag, every loop bounded by an argument.
// h1 / h2 / x_t of the slice live in LDS (as the B operand of the matrix pipe), c and the owner's copy of h in registers,
// z1 / z2 in LDS.  The gate products are v_mfma_f32_16x16x4_f32 (an exact fp32 FMA chain): gate rows as M, the 16 columns
// as N, the hidden / input index as K.  Weights are streamed from L2 every step in a layout packed once at create
// (hm_pack_kernel): rows are permuted so that one 16-row tile holds the four gates f, i, o, g of four hidden units -- the
// accumulator registers of a lane are then exactly the four gates of ONE (hidden unit, column) pair and the whole
// FLUSH / COPY / UPDATE blend (hmrnn.py:96-97) runs in registers -- and the boundary row 4H gets a tile of its own.
// The three products of a cell (W_01 h_bottom, U_21 h_top, U_11 h) are accumulated separately and combined in the
// reference's order (hmrnn.py:84), z multiplied in as a factor, never branched on.
#pragma once

#include "rnn_common.h"

#define HM_MAX_SIZE 256     // input_size, H1, H2: multiples of 4 in [4, 256]
#define HM_BUF_FLOATS (HM_MAX_SIZE * HM_COLS)

static inline bool hm_size_ok(int32_t n) { return n >= 4 && n <= HM_MAX_SIZE && (n & 3) == 0; }
static inline int32_t hm_tiles(int32_t h) { return h / 4 + 1; }            // H / 4 gate tiles + the boundary row's tile

// One cell's packed parameters: for segment s (0: W_01, 1: U_21, 2: U_11), k-group g, tile t, lane l the float4
// W[row(t, l & 15)][16 g + 4 (l >> 4) + 0..3] at seg[s] + (g * n_tiles + t) * 64 + l; zero beyond the matrix.
struct HmCell {
    const float4* seg[3];
    const float* bias;          // [n_tiles * 16] in tile order
    int32_t ng[3];              // k-groups per segment (0: segment absent)
    int32_t H, n_tiles;
};

struct HmParams {
    HmCell c1, c2;
    int32_t I, T, B;
    float a;
    const float* x;             // [T, B, I]
    const int32_t* len;         // [B] or nullptr
    const float* state_in;      // h1 [H1,B] | c1 [H1,B] | z1 [B] | h2 [H2,B] | c2 [H2,B] | z2 [B], or nullptr (zeros)
    float* state_out;
    float* h1;                  // [B, T, H1]
    float* h2;                  // [B, T, H2]
    uint8_t* z1;                // [B, T]
    uint8_t* z2;
    float* zhat;                // [T, 2, B]
    float* last_h2;             // [B, H2]
    float* tape;                // training mode (the TAPE instantiations) only: hm_tape_* below
    const int32_t* rows;        // training mode only, or nullptr: one word, the row bound R = clamp(*rows, 1, T) (hm_row_bound)
};

// The tape of the training mode: what the backward recurrence (kernels_hmlstm_bwd.h) reads beside the outputs h1 / h2 / z1 / z2.
// Per slice of 16 columns and step, hm_tape_step floats:
//   cell 1: the gates (f, i, o, g) behind their non-linearities as one float4 per owner lane, [H1 / 4 tiles][64 lanes] -- lane
//           l of tile t is (hidden unit 4 t + (l >> 4), column l & 15), so a wave stores a contiguous 1 KiB per tile -- then
//           c' as one float per owner lane in the same order;
//   cell 2: the same;
//   m1 [16], m2 [16]: 1.0f where 0 <= (f_s[4H] a + 1) / 2 <= 1 (the clamp of hard_sigm passes the gradient), else 0.
// Slice s, step t starts at ((s * T) + t) * hm_tape_step: every column of the last slice is written, b >= B included.
// Under a row bound R (HmParams::rows) the stride stays T and only the steps t < R are written.
__host__ __device__ static inline int64_t hm_tape_step(int32_t H1, int32_t H2) { return 80 * (int64_t)(H1 + H2) + 32; }
static inline int64_t hm_tape_floats(int32_t H1, int32_t H2, int32_t T, int32_t B) {
    return (int64_t)hm_slices(B) * T * hm_tape_step(H1, H2);
}

// row of the reference's [4H + 1, K] matrix behind row r of tile t; -1: padding
__host__ __device__ static inline int32_t hm_row(int32_t t, int32_t r, int32_t H) {
    if (t < H / 4) return (r & 3) * H + 4 * t + (r >> 2);
    return r == 0 ? 4 * H : -1;
}

// dst[(g * n_tiles + t) * 64 + l].{x,y,z,w} for one segment; one thread per float.
__global__ __launch_bounds__(256) void hm_pack_kernel(const float* __restrict__ src, int32_t H, int32_t K, int32_t ng,
                                                      float* __restrict__ dst) {
    const int32_t nt = H / 4 + 1;
    const int64_t total = (int64_t)ng * nt * 256;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const HmPackIdx p = hm_pack_idx(i, nt);
        const int32_t row = hm_row(p.t, p.l & 15, H);
        dst[i] = (row >= 0 && p.k < K) ? src[(int64_t)row * K + p.k] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void hm_pack_bias_kernel(const float* __restrict__ src, int32_t H, float* __restrict__ dst) {
    const int32_t n = (H / 4 + 1) * 16;
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int32_t row = hm_row(i >> 4, i & 15, H);
        dst[i] = row >= 0 ? src[row] : 0.0f;
    }
}

// The three products of a cell for N tiles: fs = W_01 h_bottom + z U_21 h_top, acc = U_11 h (hmrnn.py:75-84)
template <int N>
__device__ __forceinline__ void hm_products(hm_f32x4 (&fs)[HM_CHUNK], hm_f32x4 (&acc)[HM_CHUNK], const HmCell& cp,
                                            const float* lds_bottom, const float* lds_top, const float* lds_h, float z,
                                            int t0, int lane) {
    hm_product<N>(fs, cp.seg[0], cp.ng[0], cp.n_tiles, lds_bottom, t0, lane);
    if (cp.ng[1] > 0) {
        hm_product<N>(acc, cp.seg[1], cp.ng[1], cp.n_tiles, lds_top, t0, lane);
#pragma unroll
        for (int i = 0; i < N; ++i) fs[i] += z * acc[i];
    }
    hm_product<N>(acc, cp.seg[2], cp.ng[2], cp.n_tiles, lds_h, t0, lane);
}

// One cell for this wave's tiles w, w + 8, ..: f_s = ((W_01 h_bottom + z U_21 h_top) + z_bottom U_11 h) + bias
// (hmrnn.py:75-84) and the blend of hmrnn.py:86-97 into the owner lane's registers c, h.  Nothing is written to LDS here
// (other waves still read the operands): hm_publish does that behind the barrier.  Returns z_hat (boundary tile, q = 0).
// w is wave-uniform (the caller passes it through readfirstlane), so the tile counts below are scalar branches.
// TAPE: tape points at this cell's gates of this step, mask at its 16 mask words (see hm_tape_step).
template <int MAXS, bool TAPE = false>
__device__ __forceinline__ float hm_cell(const HmCell& cp, const float* lds_bottom, const float* lds_top, const float* lds_h,
                                         float (&c)[MAXS], float (&h)[MAXS], float z, float zb, float a, int w, int lane,
                                         float* tape = nullptr, float* mask = nullptr) {
    const int q = lane >> 4, nt = cp.n_tiles;
    const float nz = 1.0f - z, keep = nz * (1.0f - zb), upd = nz * zb;
    float zh = 0.f;
    // The chunk walk of rnn_common.h's hm_for_chunks, written out: through the helper's callables the eight instantiations of
    // the forward kernel compile to other code, which measured 1.3 - 2.4 % slower (profiles/rnn_common_refactor_ab.txt).
#pragma unroll
    for (int s0 = 0; s0 < MAXS; s0 += HM_CHUNK) {
        const int t0 = w + HM_WAVES * s0;
        if (t0 >= nt) break;
        const int CAP = MAXS - s0 < HM_CHUNK ? MAXS - s0 : HM_CHUNK;          // tiles this chunk can hold (folds when unrolled)
        const int left = (nt - t0 + HM_WAVES - 1) / HM_WAVES;                   // tiles of this wave from t0 on
        hm_f32x4 fs[HM_CHUNK], acc[HM_CHUNK];
        if (CAP >= 4 && left >= 4) hm_products<4>(fs, acc, cp, lds_bottom, lds_top, lds_h, z, t0, lane);
        else if (CAP >= 3 && left >= 3) hm_products<3>(fs, acc, cp, lds_bottom, lds_top, lds_h, z, t0, lane);
        else if (CAP >= 2 && left >= 2) hm_products<2>(fs, acc, cp, lds_bottom, lds_top, lds_h, z, t0, lane);
        else hm_products<1>(fs, acc, cp, lds_bottom, lds_top, lds_h, z, t0, lane);
#pragma unroll
        for (int i = 0; i < HM_CHUNK; ++i) {
            const int s = s0 + i, t = t0 + HM_WAVES * i;
            if (i < CAP && t < nt) {
                const float4 bv = *reinterpret_cast<const float4*>(cp.bias + t * 16 + 4 * q);
                hm_f32x4 f4 = fs[i] + zb * acc[i];
                f4 += hm_f32x4{bv.x, bv.y, bv.z, bv.w};
                if (t < nt - 1) {
                    const float f = hm_sigmoid(f4.x), gi = hm_sigmoid(f4.y), gg = tanhf(f4.w), ig = gi * gg, o = hm_sigmoid(f4.z);
                    const float cn = z * ig + keep * c[s] + upd * (f * c[s] + ig);
                    if (TAPE) {
                        ((hm_gf4*)hm_uniform(tape + t * 256))[lane] = hm_f32x4{f, gi, o, gg};
                        ((hm_gfw*)hm_uniform(tape + (nt - 1) * 256 + t * 64))[lane] = cn;
                    }
                    const float ot = o * tanhf(cn);
                    h[s] = z * ot + keep * h[s] + upd * ot;
                    c[s] = cn;
                } else {
                    // hard_sigm (hmrnn.py:25-28) in the reference's own rounding steps
                    const float pre = __fmul_rn(__fadd_rn(__fmul_rn(f4.x, a), 1.0f), 0.5f);
                    zh = fminf(fmaxf(pre, 0.0f), 1.0f);
                    if (TAPE && q == 0) ((hm_gfw*)hm_uniform(mask))[lane & 15] = (pre >= 0.0f && pre <= 1.0f) ? 1.0f : 0.0f;
                }
            }
        }
    }
    return zh;
}

// Behind the barrier: the new h of this wave's tiles into the LDS operand buffer, the boundary (hmrnn.py:34,109) into
// the slice's z and the outputs.
template <int MAXS>
__device__ __forceinline__ void hm_publish(const float (&h)[MAXS], int nt, float zh, float* lds_h, float* lds_z, int w,
                                           int lane, float* zhat_out, uint8_t* z_out, bool col_ok) {
    const int q = lane >> 4, col = lane & 15;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        const int t = w + HM_WAVES * s;
        if (t < nt - 1) lds_h[hm_idx(4 * t + q, col)] = h[s];
    }
    if (w == ((nt - 1) & (HM_WAVES - 1)) && q == 0) {
        lds_z[col] = zh > 0.5f ? 1.0f : 0.0f;
        if (col_ok) {
            if (zhat_out) *zhat_out = zh;
            if (z_out) *z_out = (uint8_t)(zh > 0.5f);
        }
    }
}

// rows [b0 .. b0 + 16) x [0, H) of an LDS operand buffer -> out[(b * T + t) * H + j] (and the last valid row of h2)
__device__ __forceinline__ void hm_store_rows(const float* lds_h, int H, int b0, int B, int T, int t, float* out,
                                              float* last, const int* lds_len) {
    for (int idx = threadIdx.x; idx < HM_COLS * H; idx += HM_THREADS) {
        const int col = idx / H, j = idx - col * H;
        const int b = b0 + col;
        if (b >= B) break;
        const float v = lds_h[hm_idx(j, col)];
        if (out) out[((int64_t)b * T + t) * H + j] = v;
        if (last && t == lds_len[col] - 1) last[(int64_t)b * H + j] = v;
    }
}

template <int MAXS, bool TAPE = false>
__global__ __launch_bounds__(HM_THREADS) void hmlstm_forward_kernel(const HmParams P) {
    __shared__ __attribute__((aligned(16))) float xbuf[HM_BUF_FLOATS];
    __shared__ __attribute__((aligned(16))) float h1buf[HM_BUF_FLOATS];
    __shared__ __attribute__((aligned(16))) float h2buf[HM_BUF_FLOATS];
    __shared__ float z1s[HM_COLS], z2s[HM_COLS];
    __shared__ int lens[HM_COLS];

    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), q = lane >> 4, col = lane & 15;
    const int b0 = blockIdx.x * HM_COLS, b = b0 + col;
    const int H1 = P.c1.H, H2 = P.c2.H, I = P.I, T = P.T, B = P.B;
    const bool col_ok = b < B;
    const int nt1 = P.c1.n_tiles, nt2 = P.c2.n_tiles;
    // The rows this call runs.  Training mode under a row bound: the call is the one at T = R on the rows in front of R (the
    // buffers keep their strides of T) and leaves exact zeros behind.  Everywhere else R is T.
    const int R = TAPE ? hm_row_bound(P.rows, T) : T;

    for (int i = tid; i < HM_BUF_FLOATS; i += HM_THREADS) { xbuf[i] = 0.f; h1buf[i] = 0.f; h2buf[i] = 0.f; }
    if (tid < HM_COLS) {
        const int bb = b0 + tid;
        float v1 = 0.f, v2 = 0.f;
        int n = R;
        if (bb < B) {
            if (P.state_in) {
                v1 = P.state_in[(int64_t)2 * H1 * B + bb];
                v2 = P.state_in[(int64_t)(2 * H1 + 1 + 2 * H2) * B + bb];
            }
            if (P.len) n = min(max(P.len[bb], 1), R);
        }
        z1s[tid] = v1;
        z2s[tid] = v2;
        lens[tid] = n;
    }
    __syncthreads();

    // the owner lane's c and h of (hidden unit 4 t + q, column col), tile t = w + 8 s
    float c1[MAXS], h1[MAXS], c2[MAXS], h2[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        const int t = w + HM_WAVES * s, j = 4 * t + q;
        c1[s] = h1[s] = c2[s] = h2[s] = 0.f;
        if (P.state_in && col_ok) {
            if (t < nt1 - 1) {
                h1[s] = P.state_in[(int64_t)j * B + b];
                c1[s] = P.state_in[(int64_t)(H1 + j) * B + b];
                h1buf[hm_idx(j, col)] = h1[s];
            }
            if (t < nt2 - 1) {
                const float* s2 = P.state_in + (int64_t)(2 * H1 + 1) * B;
                h2[s] = s2[(int64_t)j * B + b];
                c2[s] = s2[(int64_t)(H2 + j) * B + b];
                h2buf[hm_idx(j, col)] = h2[s];
            }
        }
    }

    // x_t of the slice: (column, 4 inputs) per thread, at most two per thread (16 * 256 / 4 = 1024 float4)
    const int nx = HM_COLS * (I >> 2);
    float4 xr[2];
    auto load_x = [&](int t) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int idx = tid + r * HM_THREADS;
            xr[r] = float4{0.f, 0.f, 0.f, 0.f};
            if (idx < nx) {
                const int xc = idx / (I >> 2), i4 = idx - xc * (I >> 2);
                if (b0 + xc < B)
                    xr[r] = *reinterpret_cast<const float4*>(P.x + ((int64_t)t * B + b0 + xc) * I + 4 * i4);
            }
        }
    };
    auto put_x = [&]() {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int idx = tid + r * HM_THREADS;
            if (idx < nx) {
                const int xc = idx / (I >> 2), i4 = idx - xc * (I >> 2);
                reinterpret_cast<float4*>(xbuf)[i4 * HM_COLS + xc] = xr[r];
            }
        }
    };
    load_x(0);
    put_x();
    __syncthreads();

    // When h_2 at len - 1 is the ONLY output asked for, nothing behind the longest column of the slice can reach it: the slice
    // stops there (wave-uniform, at most T).  Any other output is defined over all T steps (R under a row bound).
    int steps = R;
    if (!TAPE && P.len && P.last_h2 && !P.state_out && !P.h1 && !P.h2 && !P.z1 && !P.z2 && !P.zhat) {
        steps = 1;
        for (int c = 0; c < HM_COLS; ++c)
            if (b0 + c < B) steps = max(steps, lens[c]);
        steps = __builtin_amdgcn_readfirstlane(steps);
    }

    float* tp = nullptr;                    // this slice's tape rows of step t
    if (TAPE) tp = P.tape + (int64_t)blockIdx.x * T * hm_tape_step(H1, H2);
    for (int t = 0; t < steps; ++t) {
        if (t + 1 < steps) load_x(t + 1);
        // ---- cell 1: bottom = x_t with z_bottom = 1, top = h2 of the previous step (hmrnn.py:146)
        const float zh1 = hm_cell<MAXS, TAPE>(P.c1, xbuf, h2buf, h1buf, c1, h1, z1s[col], 1.0f, P.a, w, lane, tp,
                                              TAPE ? tp + 80 * (H1 + H2) : nullptr);
        __syncthreads();                    // every wave has read xbuf, h1buf and z1s
        if (t + 1 < steps) put_x();
        hm_publish<MAXS>(h1, nt1, zh1, h1buf, z1s, w, lane, P.zhat ? P.zhat + ((int64_t)t * 2) * B + b : nullptr,
                         P.z1 ? P.z1 + (int64_t)b * T + t : nullptr, col_ok);
        __syncthreads();                    // h1buf / z1s hold step t
        if (P.h1) hm_store_rows(h1buf, H1, b0, B, T, t, P.h1, nullptr, lens);
        // ---- cell 2: bottom = h1 and z1 of THIS step, no top-down term (hmrnn.py:147)
        const float zh2 = hm_cell<MAXS, TAPE>(P.c2, h1buf, nullptr, h2buf, c2, h2, z2s[col], z1s[col], P.a, w, lane,
                                              TAPE ? tp + 80 * H1 : nullptr, TAPE ? tp + 80 * (H1 + H2) + 16 : nullptr);
        __syncthreads();                    // every wave has read h2buf and z2s
        hm_publish<MAXS>(h2, nt2, zh2, h2buf, z2s, w, lane, P.zhat ? P.zhat + ((int64_t)t * 2 + 1) * B + b : nullptr,
                         P.z2 ? P.z2 + (int64_t)b * T + t : nullptr, col_ok);
        __syncthreads();                    // h2buf / z2s hold step t
        if (P.h2 || P.last_h2) hm_store_rows(h2buf, H2, b0, B, T, t, P.h2, P.last_h2, lens);
        if (TAPE) tp += hm_tape_step(H1, H2);
    }

    if (TAPE && R < T) {                    // behind the bound: every element of every output is still written, as an exact zero
        if (P.h1) hm_zero_tail_bth(P.h1, H1, R, T, b0, B);
        if (P.h2) hm_zero_tail_bth(P.h2, H2, R, T, b0, B);
        const int cols = min(HM_COLS, B - b0), nz = T - R;
        for (int idx = tid; idx < cols * nz; idx += HM_THREADS) {
            const int c = idx / nz, j = idx - c * nz;
            const int64_t at = (int64_t)(b0 + c) * T + R + j;
            if (P.z1) P.z1[at] = 0;
            if (P.z2) P.z2[at] = 0;
        }
        if (P.zhat)
            for (int idx = tid; idx < 2 * nz * cols; idx += HM_THREADS) {
                const int row = idx / cols, c = idx - row * cols;
                P.zhat[((int64_t)2 * R + row) * B + b0 + c] = 0.f;
            }
    }

    if (P.state_out && col_ok) {
        float* s1 = P.state_out;
        float* s2 = P.state_out + (int64_t)(2 * H1 + 1) * B;
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
            const int tl = w + HM_WAVES * s, j = 4 * tl + q;
            if (tl < nt1 - 1) { s1[(int64_t)j * B + b] = h1[s]; s1[(int64_t)(H1 + j) * B + b] = c1[s]; }
            if (tl < nt2 - 1) { s2[(int64_t)j * B + b] = h2[s]; s2[(int64_t)(H2 + j) * B + b] = c2[s]; }
        }
        if (w == 0 && q == 0) {
            s1[(int64_t)2 * H1 * B + b] = z1s[col];
            s2[(int64_t)2 * H2 * B + b] = z2s[col];
        }
    }
}
