// Forward pass of the reference's layers.DynamicEncoder (layers.py:42-76): n_layers bidirectional GRU layers over ragged
// lengths, fp32, one launch per layer plus one that sums the two directions of the last layer.
//
// Shape.  As in kernels_hmlstm.h (rnn_common.h) a workgroup owns a slice of HM_COLS = 16 batch columns for all steps of ONE direction
// (grid = slices x 2) and never waits on another workgroup: no grid barrier, no flag, every loop bounded by an argument.
// A slice runs max(len) of its columns steps; the reverse direction starts there, so neither sorting nor packing is needed.
//
// Layout (the "four slots per hidden unit" one).  A 16-row tile holds the slots (r, z, n_x, n_h) of four hidden units, so the
// four accumulator registers of a lane are exactly the gates of ONE (hidden unit, column) pair and the blend runs in
// registers.  The input part and the hidden part are ONE product over the concatenated K axis [x (padded to 16) | h]:
// rows r and z carry weights in both parts, n_x only in the x part (W_in), n_h only in the h part (W_hn), zeros elsewhere,
// which keeps W_in x and W_hn h in separate registers as  n = tanh(n_x + r * n_h)  needs.  The operand [x_t | h] is one LDS
// buffer in the hm_idx layout and the product loop is hm_product of rnn_common.h, unchanged.
#pragma once

#include "rnn_common.h"

#define GRU_MAX_IN 512      // input_size: 1 .. 512 (inner layers read 2 H <= 512)
#define GRU_MAX_H 256       // hidden: multiple of 4 in [4, 256]
#define GRU_MAX_LAYERS 4
#define GRU_BUF_FLOATS ((GRU_MAX_IN + GRU_MAX_H) * HM_COLS)
#define GRU_X_ROUNDS (GRU_MAX_IN * HM_COLS / HM_THREADS)    // floats of x_t a thread stages per step, at most

// One direction's packed parameters: k-group g, tile t, lane l hold the float4 W[row(t, l & 15)][16 g + 4 (l >> 4) + 0..3]
// of the concatenated matrix at w + (g * n_tiles + t) * 64 + l; bias [n_tiles * 16] in tile order (r: b_ir + b_hr, z: b_iz + b_hz,
// n_x: b_in, n_h: b_hn).
struct GruDir {
    const float4* w;
    const float* bias;
};

struct GruParams {
    GruDir d[2];                // forward, reverse
    int32_t I, H, ngx, ng;      // k-groups of the x part, and of x and h together
    int32_t T, B;
    const float* x;             // [>= T, B, I]
    const int32_t* len;         // [B] or nullptr
    float* out;                 // [T, B, 2 H]: forward | reverse, or nullptr
    float* hn;                  // [2, B, H] of this layer, or nullptr
    float* tape;                // training mode (the TAPE instantiations) only: this layer's gates, gru_tape_* below
    const float* drop;          // training mode only: [T, B, I] multipliers of x (inter-layer dropout), or nullptr
};

// The tape of the training mode (dsp_bigru_forward_train): what the backward recurrence (kernels_bigru_bwd.h) reads.
//   rows:  per layer the [T, B, 2 H] output rows (forward | reverse), EVERY row written: exact zeros at t >= len[b], also
//          behind a slice's last step -- layer l at float l * T * B * 2 H;
//   gates: behind the rows of all layers, per layer, direction, slice of 16 columns and step gru_tape_step floats: the owner
//          lane's float4 (r, z, n behind their non-linearities, n_h = W_hn h + b_hn), [H / 4 tiles][64 lanes] -- lane l of tile t
//          is (hidden unit 4 t + (l >> 4), column l & 15), so a wave stores a contiguous 1 KiB per tile.  Only the steps a
//          slice visits (t < max len of its columns) are stored; every column of the last slice is, b >= B included.
__host__ __device__ static inline int64_t gru_tape_step(int32_t H) { return 64 * (int64_t)H; }
static inline int64_t gru_tape_rows_floats(int32_t H, int32_t T, int32_t B) { return (int64_t)T * B * 2 * H; }
static inline int64_t gru_tape_layer_gates_floats(int32_t H, int32_t T, int32_t B) {
    return 2 * (int64_t)hm_slices(B) * T * gru_tape_step(H);
}
static inline int64_t gru_tape_floats(int32_t H, int32_t L, int32_t T, int32_t B) {
    return L * (gru_tape_rows_floats(H, T, B) + gru_tape_layer_gates_floats(H, T, B));
}

// dst[((g * nt + t) * 64 + l) * 4 + e]; one thread per float.  w_ih [3H, I], w_hh [3H, H], rows r | z | n.
__global__ __launch_bounds__(256) void gru_pack_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, int32_t H,
                                                       int32_t I, int32_t ngx, int32_t ng, float* __restrict__ dst) {
    const int32_t nt = H / 4;
    const int64_t total = (int64_t)ng * nt * 256;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const HmPackIdx p = hm_pack_idx(i, nt);
        const int32_t r = p.l & 15, slot = r & 3, unit = 4 * p.t + (r >> 2), k = p.k;
        float v = 0.0f;
        if (p.g < ngx) {
            if (slot < 3 && k < I) v = w_ih[(int64_t)(slot * H + unit) * I + k];
        } else {
            const int32_t kh = k - 16 * ngx, gate = slot == 3 ? 2 : slot;
            if (slot != 2 && kh < H) v = w_hh[(int64_t)(gate * H + unit) * H + kh];
        }
        dst[i] = v;
    }
}

__global__ __launch_bounds__(256) void gru_pack_bias_kernel(const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                            int32_t H, float* __restrict__ dst) {
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < 4 * H; i += gridDim.x * blockDim.x) {
        const int32_t slot = i & 3, unit = i >> 2;
        dst[i] = slot < 2 ? b_ih[slot * H + unit] + b_hh[slot * H + unit] : slot == 2 ? b_ih[2 * H + unit] : b_hh[2 * H + unit];
    }
}

// One step for this wave's tiles w, w + 8, ..: the gates of (hidden unit 4 t + q, column col) into the owner lane's h.
// Nothing is written to LDS here (other waves still read the operand).  w is wave-uniform.
// TAPE: tape points at this slice's gates of this step (see gru_tape_step).
template <int MAXS, bool TAPE = false>
__device__ __forceinline__ void gru_cell(const GruDir& dp, int ng, int nt, const float* lds, float (&h)[MAXS], bool active,
                                         int w, int lane, float* tape = nullptr) {
    const int q = lane >> 4;
    struct Acc { hm_f32x4 acc[HM_CHUNK]; };
    hm_for_chunks<MAXS, Acc>(
        nt, w, [&](auto n, Acc& p, int t0) { hm_product<decltype(n)::value>(p.acc, dp.w, ng, nt, lds, t0, lane); },
        [&](const Acc& p, int i, int s, int t) {
            const float4 bv = *reinterpret_cast<const float4*>(dp.bias + t * 16 + 4 * q);
            const hm_f32x4 f4 = p.acc[i] + hm_f32x4{bv.x, bv.y, bv.z, bv.w};
            const float r = hm_sigmoid(f4.x), z = hm_sigmoid(f4.y), n = tanhf(f4.z + r * f4.w);
            if (TAPE) ((hm_gf4*)hm_uniform(tape + t * 256))[lane] = hm_f32x4{r, z, n, f4.w};
            const float hn = (1.0f - z) * n + z * h[s];
            h[s] = active ? hn : h[s];                                          // a column behind its end keeps its h
        });
}

template <int MAXS, bool TAPE = false>
__global__ __launch_bounds__(HM_THREADS) void bigru_layer_kernel(const GruParams P) {
    __shared__ __attribute__((aligned(16))) float buf[GRU_BUF_FLOATS];       // [x_t, K padded to 16 | h] of the slice
    __shared__ int lens[HM_COLS];

    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), q = lane >> 4, col = lane & 15;
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * HM_COLS, b = b0 + col;
    const int H = P.H, I = P.I, T = P.T, B = P.B, nt = H >> 2, ng = P.ng;
    const GruDir dp = P.d[dir];
    float* hbuf = buf + P.ngx * (16 * HM_COLS);

    for (int i = tid; i < ng * (16 * HM_COLS); i += HM_THREADS) buf[i] = 0.f;
    const int steps = hm_slice_steps(P.len, b0, B, T, lens);
    const int mylen = lens[col];

    // x_t of the slice is one contiguous run of (columns of the slice) * I floats; rows need not be 16-byte aligned
    const int nx = min(HM_COLS, B - b0) * I;
    float xr[GRU_X_ROUNDS];
    auto load_x = [&](int t) {
        const float* src = P.x + ((int64_t)t * B + b0) * I;
#pragma unroll
        for (int r = 0; r < GRU_X_ROUNDS; ++r) {
            const int idx = tid + r * HM_THREADS;
            xr[r] = 0.f;
            if (idx < nx) xr[r] = src[idx];
        }
        if (TAPE && P.drop) {                   // the same layout as x: a second load with the same index
            const float* dsrc = P.drop + ((int64_t)t * B + b0) * I;
#pragma unroll
            for (int r = 0; r < GRU_X_ROUNDS; ++r) {
                const int idx = tid + r * HM_THREADS;
                if (idx < nx) xr[r] *= dsrc[idx];
            }
        }
    };
    auto put_x = [&]() {
#pragma unroll
        for (int r = 0; r < GRU_X_ROUNDS; ++r) {
            const int idx = tid + r * HM_THREADS;
            if (idx < nx) {
                const int xc = idx / I, k = idx - xc * I;
                buf[hm_idx(k, xc)] = xr[r];
            }
        }
    };
    auto step_t = [&](int s) { return dir ? steps - 1 - s : s; };

    float h[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) h[s] = 0.f;

    if (steps > 0) {
        load_x(step_t(0));
        put_x();
    }
    __syncthreads();

    float* tp = nullptr;                    // this slice's gates of step 0
    if (TAPE) tp = P.tape + ((int64_t)dir * gridDim.x + blockIdx.x) * T * gru_tape_step(H);
    for (int s = 0; s < steps; ++s) {
        const int t = step_t(s);
        if (s + 1 < steps) load_x(step_t(s + 1));
        gru_cell<MAXS, TAPE>(dp, ng, nt, buf, h, t < mylen, w, lane, TAPE ? tp + t * gru_tape_step(H) : nullptr);
        __syncthreads();                    // every wave has read x_t and h
        if (s + 1 < steps) put_x();
#pragma unroll
        for (int i = 0; i < MAXS; ++i) {
            const int tl = w + HM_WAVES * i;
            if (tl < nt) hbuf[hm_idx(4 * tl + q, col)] = h[i];
        }
        __syncthreads();                    // the buffer holds x of the next step and h of this one
        if (P.out) {
            for (int idx = tid; idx < HM_COLS * H; idx += HM_THREADS) {
                const int c = idx / H, j = idx - c * H;
                if (b0 + c >= B) break;
                const float v = t < lens[c] ? hbuf[hm_idx(j, c)] : 0.f;     // an exact zero row behind the column's end
                P.out[((int64_t)t * B + b0 + c) * (2 * H) + dir * H + j] = v;
            }
        }
    }

    // the rows no step visited: the backward's GEMMs read every row of a layer
    if (TAPE && P.out) hm_zero_rows(P.out, H, 2 * H, dir * H, steps, T, b0, B);

    if (P.hn && b < B) {
#pragma unroll
        for (int i = 0; i < MAXS; ++i) {
            const int tl = w + HM_WAVES * i;
            if (tl < nt) P.hn[((int64_t)dir * B + b) * H + 4 * tl + q] = h[i];
        }
    }
}

// y[t, b, :] = forward + reverse halves of the last layer where t < len[b], an exact zero row elsewhere: every element of y
// is written, in a fixed order of additions.
__global__ __launch_bounds__(256) void bigru_sum_kernel(const float* __restrict__ halves, const int32_t* __restrict__ len,
                                                        int32_t T, int32_t B, int32_t H, float* __restrict__ y) {
    const int64_t total = (int64_t)T * B * H;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / H;
        const int32_t j = (int32_t)(i - row * H), bb = (int32_t)(row % B), t = (int32_t)(row / B);
        const int32_t n = len ? min(max(len[bb], 1), T) : T;
        y[i] = t < n ? halves[row * (2 * H) + j] + halves[row * (2 * H) + H + j] : 0.f;
    }
}
