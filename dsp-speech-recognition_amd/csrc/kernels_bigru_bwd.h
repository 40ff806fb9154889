// Backward recurrence of one bidirectional GRU layer (kernels_bigru.h is the forward; its training mode leaves the tape read
// here), fp32, one launch per layer of the forward's shape: grid = slices of HM_COLS = 16 batch columns x 2 directions, 512
// threads; a workgroup owns its columns of one direction for all steps, runs them in the OPPOSITE order of the forward's
// (forward direction t = steps - 1 .. 0, reverse direction t = 0 .. steps - 1) and never waits on another workgroup -- no grid
// barrier, no flag, every loop bounded by an argument.  What it leaves is
//   da [T, B, 2, 4 H]: per step, column and direction the gradients of the four pre-activations, H floats each, in the order
//                      n_x | r | z | n_h  (a_r = W_ir x + W_hr h + b, a_z likewise, n_x = W_in x + b_in, n_h = W_hn h + b_hn):
//                      floats [0, 3 H) are the rows of weight_ih's gradient GEMM (n | r | z), floats [H, 4 H) those of weight_hh's
//                      (r | z | n), both contiguous.  Every element is written on every call (exact zeros at t >= len[b]).
// The gradients of x and of the parameters are plain GEMMs over it (include/dsp_frontend.h states the formulas).
//
// Ownership is the forward's: lane l of wave w holds, in slot s, (hidden unit 4 (w + 8 s) + (l >> 4), column l & 15) -- the lane
// that wrote the unit's gates to the tape reads them back, and dh of the unit lives in its registers for all steps.  Per step
// the owners compute the four gate gradients of their units and write them, as one float4, into the LDS operand of the matrix
// pipe: its K order is (unit, slot), so float4 unit * 16 + col IS the owner's place (tile * 64 + lane, conflict free).  The n_x
// slot stays in K (K = 4 H, its weights are zeros): the operand is 64 H floats, 64 KiB at H = 256.  dh += W_hh^T (da_r, da_z,
// da_nh) is hm_bwd_product of rnn_common.h: the weights are packed transposed at create (gru_pack_t_kernel, hm_pack_t_kernel's scheme) with the
// rows of an M tile permuted so that accumulator register r of chunk c is slot 4 c + r of the lane that owns the unit -- the
// product lands in the owners' registers and nothing but da crosses LDS.  Two barriers per step.
#pragma once

#include "kernels_bigru.h"
#include "rnn_common.h"

struct GruBwdParams {
    const float4* wt[2];        // packed transposed W_hh of the forward and the reverse direction (gru_pack_t_kernel)
    int32_t H, T, B;
    int32_t g_stride;           // floats per (t, b) row of g: H (top layer: y is the sum, both directions read the same row) or 2 H
    const int32_t* len;         // [B] or nullptr
    const float* gates;         // this layer's gates in the tape (gru_tape_step)
    const float* out;           // [T, B, 2 H]  this layer's output rows in the tape
    const float* g;             // [T, B, g_stride] or nullptr
    const float* g_hn;          // [2, B, H] of this layer, or nullptr
    float* da;                  // [T, B, 2, 4 H]
};

static inline int64_t gru_bwd_packed_floats(int32_t H) { return (int64_t)(H / 4) * HM_WAVES * hm_bwd_chunks(H) * 256; }
static inline size_t gru_bwd_lds_bytes(int32_t H) { return (size_t)64 * H * sizeof(float); }

// The transposed copy of one weight_hh [3 H, H] (rows r | z | n): dst[(g * nt + tt) * 64 + l].{x,y,z,w}, nt = 8 * hm_bwd_chunks(H),
// is W[row(k)][m] with k = 16 g + 4 (l >> 4) + 0..3 = 4 unit + slot -> row unit (slot 0: r), H + unit (1: z), none (2: n_x, zeros),
// 2 H + unit (3: n_h); and for M tile tt = 8 c + w, row i = l & 15: m = 4 (w + 8 (4 c + (i & 3))) + (i >> 2), zero beyond H.
__global__ __launch_bounds__(256) void gru_pack_t_kernel(const float* __restrict__ w_hh, int32_t H, int32_t nt, float* __restrict__ dst) {
    const int64_t total = (int64_t)(H / 4) * nt * 256;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const HmPackIdx p = hm_pack_idx(i, nt);
        const int32_t slot = p.k & 3, unit = p.k >> 2, m = hm_pack_t_m(p.t, p.l);
        const int32_t row = slot == 2 ? -1 : (slot == 3 ? 2 * H + unit : slot * H + unit);
        dst[i] = (row >= 0 && m < H) ? w_hh[(int64_t)row * H + m] : 0.0f;
    }
}

// What the owners read for one step: the gates of the step, h in front of it, the incoming gradient of h'.
template <int NS>
struct GruBwdIn { hm_f32x4 gt[NS]; float hp[NS], g[NS]; };

template <int NC>
__global__ __launch_bounds__(HM_THREADS) void bigru_backward_kernel(const GruBwdParams P) {
    constexpr int NS = 4 * NC;
    extern __shared__ __attribute__((aligned(16))) float grb_smem[];     // the B operand: H / 4 k-groups of 64 float4
    __shared__ int lens[HM_COLS];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), q = lane >> 4, col = lane & 15;
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * HM_COLS, b = b0 + col;
    const int H = P.H, T = P.T, B = P.B, nt = H >> 2, nc = hm_bwd_chunks(H);
    const bool col_ok = b < B;

    const int steps = hm_slice_steps(P.len, b0, B, T, lens);
    const int mylen = lens[col];

    const int64_t step = gru_tape_step(H);
    const float* tape = P.gates + ((int64_t)dir * gridDim.x + blockIdx.x) * T * step;
    const int gs = P.g_stride, goff = gs > H ? dir * H : 0;
    auto step_t = [&](int s) { return dir ? s : steps - 1 - s; };

    // h_n of the forward direction is h at len - 1, kept through the inactive steps behind it; h_n of the reverse direction is h
    // at t = 0, the last step its forward runs.  Both are therefore the state this kernel starts from (inactive steps hand dh
    // through unchanged), and g_hn seeds dh here.
    float dh[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int tl = w + HM_WAVES * s;
        dh[s] = 0.f;
        if (P.g_hn && col_ok && tl < nt) dh[s] = ((hm_gf*)hm_uniform(P.g_hn + ((int64_t)dir * B + b0) * H + 4 * tl))[col * H + q];
    }

    GruBwdIn<NS> in;
    auto load = [&](int t) {
        const bool active = t < mylen;                                          // (implies col_ok)
        const int tp = dir ? t + 1 : t - 1;                                     // the step the forward ran in front of t
        const bool has_prev = dir ? tp < mylen : tp >= 0;                       // tested on the length, never on the rows' contents
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int tl = w + HM_WAVES * s;
            in.gt[s] = hm_f32x4{0.f, 0.f, 0.f, 0.f};
            in.hp[s] = in.g[s] = 0.f;
            if (tl < nt) {
                in.gt[s] = ((const hm_gf4*)hm_uniform(tape + t * step + tl * 256))[lane];
                if (active) {
                    if (has_prev) in.hp[s] = ((hm_gf*)hm_uniform(P.out + ((int64_t)tp * B + b0) * (2 * H) + dir * H + 4 * tl))[col * 2 * H + q];
                    if (P.g) in.g[s] = ((hm_gf*)hm_uniform(P.g + ((int64_t)t * B + b0) * gs + goff + 4 * tl))[col * gs + q];
                }
            }
        }
    };

    hm_lf4* d4 = (hm_lf4*)grb_smem;
    if (steps > 0) load(step_t(0));

    for (int s0 = 0; s0 < steps; ++s0) {
        const int t = step_t(s0);
        const bool active = t < mylen;
        float* out = P.da + (((int64_t)t * B + b0) * 2 + dir) * (4 * H);      // row of column b0, this direction
        const int lo = col * 8 * H + q;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int tl = w + HM_WAVES * s;
            if (tl < nt) {
                const float r = in.gt[s].x, z = in.gt[s].y, n = in.gt[s].z, nh = in.gt[s].w;
                const float d = dh[s] + in.g[s];
                const float dn = d * (1.0f - z), dz = d * (in.hp[s] - n), dnp = dn * (1.0f - n * n);
                hm_f32x4 v = hm_f32x4{dnp * nh * r * (1.0f - r), dz * z * (1.0f - z), dnp, dnp * r};
                if (!active) v = hm_f32x4{0.f, 0.f, 0.f, 0.f};              // a column behind its end: an exact zero row,
                dh[s] = active ? d * z : dh[s];                                 // and dh passes through
                d4[tl * 64 + lane] = v;
                if (col_ok) hm_store_gate_grads(out, H, tl, lo, v.z, v.x, v.y, v.w);        // rows n_x | r | z | n_h
            }
        }
        if (s0 + 1 < steps) load(step_t(s0 + 1));       // in flight behind the product
        __syncthreads();                                // the operand holds da of this step
        {
            float u[NS];
            hm_bwd_product<NC>(u, P.wt[dir], nt, nc, grb_smem, w, lane);
#pragma unroll
            for (int s = 0; s < NS; ++s) dh[s] += u[s];
        }
        __syncthreads();                                // every wave has read da
    }

    // the steps no column of the slice reaches: exact zero rows
    hm_zero_rows(P.da, 4 * H, 8 * H, dir * 4 * H, steps, T, b0, B);
}
