// Backward recurrence of the HM-LSTM (kernels_hmlstm.h is the forward; its training mode leaves the tape read here), fp32,
// as ONE persistent launch of the same shape: a workgroup of 512 threads owns a slice of HM_COLS = 16 batch columns, runs the
// steps t = T - 1 .. 0 for it (R - 1 .. 0 under a row bound, HmBwdParams::rows) and never waits on another workgroup -- no
// grid barrier, no flag, every loop bounded by an argument.  What it leaves are dfs1 [T, B, 4 H1 + 1] and dfs2 [T, B, 4 H2 + 1], the gradients of the two cells'
// pre-activations f_s (hmrnn.py:84); the gradients of x and of the parameters are plain GEMMs over them
// (include/dsp_frontend.h states the formulas).
//
// Ownership is the forward's: lane l of wave w holds, in slot s, (hidden unit 4 (w + 8 s) + (l >> 4), column l & 15) -- the
// lane that wrote the unit's gates to the tape reads them back, and dh / dc of the unit live in its registers for all
// steps.  Per step and cell the owners compute the four gate gradients of their units and write them, as one float4, into
// the LDS operand of the matrix pipe: its K order is (unit, gate), so float4 j * 16 + col IS the owner's place
// (tile * 64 + lane, conflict free), and row 4 H (the boundary) follows in a k-group of its own.  The four transposed
// products of a step (U_11(2)^T dfs2, W_01(2)^T dfs2, U_21^T dfs1, U_11(1)^T dfs1) are v_mfma_f32_16x16x4_f32 with the
// hidden index as M, through hm_product of the forward: the weights are packed transposed at create
// (hm_pack_t_kernel), with the rows of an M tile permuted so that accumulator register r of chunk c is slot 4 c + r of the
// lane that owns the unit -- the products land in the owners' registers and nothing is exchanged through LDS but dfs.
// dz and dz_bottom are sums over the hidden units of a column: lanes of a wave are combined by two butterfly steps, the
// eight waves through LDS in wave order, every lane of a column adding the same eight words in the same order.
#pragma once

#include "kernels_hmlstm.h"
#include "rnn_common.h"

struct HmBwdParams {
    const float4* wt[4];        // packed transposed: U_11(2)^T, W_01(2)^T, U_21^T, U_11(1)^T
    int32_t H1, H2, T, B;
    float a;
    const int32_t* len;         // [B] or nullptr
    const float* state_in;      // as HmParams, or nullptr (zeros)
    const float* tape;          // hm_tape_step
    const float* h1;            // [B, T, H1]  the forward's outputs
    const float* h2;
    const uint8_t* z1;          // [B, T]
    const uint8_t* z2;
    const float* g_h1;          // [B, T, H1]  gradients of the loss, each may be nullptr
    const float* g_h2;
    const float* g_last;        // [B, H2]
    float* dfs1;                // [T, B, 4 H1 + 1]
    float* dfs2;
    const int32_t* rows;        // nullptr, or the word the forward was given: the row bound R = clamp(*rows, 1, T) (hm_row_bound)
};

static inline int64_t hm_bwd_packed_floats(int32_t Hcell, int32_t Hout) { return (int64_t)(Hcell / 4 + 1) * HM_WAVES * hm_bwd_chunks(Hout) * 256; }
static inline size_t hm_bwd_lds_bytes(int32_t H1, int32_t H2) { return ((size_t)((H1 > H2 ? H1 : H2) / 4 + 1) * 256 + 2 * HM_WAVES * HM_COLS) * sizeof(float); }

// The transposed copy of one [4 H + 1, K] matrix: dst[(g * nt + tt) * 64 + l].{x,y,z,w}, nt = 8 * hm_bwd_chunks(K), is
// W[row(k)][m] with k = 16 g + 4 (l >> 4) + 0..3 -> row (k & 3) * H + (k >> 2) (gate k & 3 of unit k >> 2), k = 4 H -> row
// 4 H, zero beyond; and for M tile tt = 8 c + w, row i = l & 15: m = 4 (w + 8 (4 c + (i & 3))) + (i >> 2), zero beyond K.
__global__ __launch_bounds__(256) void hm_pack_t_kernel(const float* __restrict__ src, int32_t H, int32_t K, int32_t nt,
                                                        float* __restrict__ dst) {
    const int64_t total = (int64_t)(H / 4 + 1) * nt * 256;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const HmPackIdx p = hm_pack_idx(i, nt);
        const int32_t k = p.k, m = hm_pack_t_m(p.t, p.l);
        const int32_t row = k < 4 * H ? (k & 3) * H + (k >> 2) : (k == 4 * H ? 4 * H : -1);
        dst[i] = (row >= 0 && m < K) ? src[(int64_t)row * K + m] : 0.0f;
    }
}

// What the owners of one cell read for one step: the gates and c' of the step, c and h in front of it, the loss's gradient
// of h'.  tp / tp_prev: the cell's gates of step t / t - 1 in the tape (hm_tape_step); hout / gout [B, T, H]; st_h / st_c: the
// [H, B] rows of state_in, or nullptr.  Addresses: a uniform part (slice b0, step, tile) + the lane's (column, q) part.
template <int NS>
struct HmBwdIn { hm_f32x4 gt[NS]; float cn[NS], cp[NS], hp[NS], g[NS]; };

template <int NS>
__device__ __forceinline__ void hm_bwd_load(HmBwdIn<NS>& in, const float* tp, const float* tp_prev, const float* hout,
                                            const float* st_h, const float* st_c, const float* gout, const float* glast,
                                            bool last_here, int H, int T, int B, int t, int b0, bool col_ok, int w, int lane) {
    const int q = lane >> 4, col = lane & 15, ntg = H >> 2;
    const int64_t lo_bt = (int64_t)col * T * H + q;             // the lane's part of [b, t, j]
    const int lo_st = q * B + col, lo_last = col * H + q;       // ... of [j, b] and of [b, j]
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int tl = w + HM_WAVES * s;
        in.gt[s] = hm_f32x4{0.f, 0.f, 0.f, 0.f};
        in.cn[s] = in.cp[s] = in.hp[s] = in.g[s] = 0.f;
        if (tl < ntg) {
            in.gt[s] = ((const hm_gf4*)hm_uniform(tp + tl * 256))[lane];
            in.cn[s] = ((hm_gf*)hm_uniform(tp + ntg * 256 + tl * 64))[lane];
            if (t > 0) in.cp[s] = ((hm_gf*)hm_uniform(tp_prev + ntg * 256 + tl * 64))[lane];
            if (col_ok) {
                if (t > 0) in.hp[s] = ((hm_gf*)hm_uniform(hout + ((int64_t)b0 * T + t - 1) * H + 4 * tl))[lo_bt];
                else if (st_h) {
                    in.hp[s] = ((hm_gf*)hm_uniform(st_h + (int64_t)4 * tl * B + b0))[lo_st];
                    in.cp[s] = ((hm_gf*)hm_uniform(st_c + (int64_t)4 * tl * B + b0))[lo_st];
                }
                if (gout) in.g[s] = ((hm_gf*)hm_uniform(gout + ((int64_t)b0 * T + t) * H + 4 * tl))[lo_bt];
                if (glast && last_here) in.g[s] += ((hm_gf*)hm_uniform(glast + (int64_t)b0 * H + 4 * tl))[lo_last];
            }
        }
    }
}

// One (unit, column) of one cell, one step: the gate gradients; dc becomes the gradient of c in front of the step, pz / pzb
// collect the pointwise parts of dz and dz_bottom.  dh, dc: the gradients of h' and c'.
__device__ __forceinline__ hm_f32x4 hm_bwd_point(const hm_f32x4 gt, float cn, float c, float h, float z, float zb, float dh,
                                                 float& dc, float& pz, float& pzb) {
    const float f = gt.x, i = gt.y, o = gt.z, g = gt.w;
    const float nz = 1.0f - z, nzb = 1.0f - zb, keep = nz * nzb, upd = nz * zb, s = z + upd;
    const float tc = tanhf(cn);
    const float dot = dh * s, dcn = dc + dot * o * (1.0f - tc * tc), d_o = dot * tc, dig = dcn * s, df = dcn * upd * c;
    const float ig = i * g, fcig = f * c + ig, otc = o * tc;
    pz += dcn * (ig - nzb * c - zb * fcig) + dh * (otc - nzb * h - zb * otc);
    pzb += dcn * nz * (fcig - c) + dh * nz * (otc - h);
    dc = dcn * (keep + upd * f);
    return hm_f32x4{df * f * (1.0f - f), dig * g * i * (1.0f - i), d_o * o * (1.0f - o), dig * i * (1.0f - g * g)};
}

// The owners' part of one cell: dfs of their units into the LDS operand and into out [4 H + 1] rows of (t, b); the boundary
// row's k-group (row 4 H = zrow, fifteen zero rows) by wave 0.  dh comes in without the loss's part in.g and leaves with it.
template <int NS>
__device__ __forceinline__ void hm_bwd_cell(const HmBwdIn<NS>& in, int H, float z, float zb, float zrow, float (&dh)[NS],
                                            float (&dc)[NS], float& pz, float& pzb, float* dfs, float* out, bool col_ok,
                                            int w, int lane) {
    const int q = lane >> 4, ntg = H >> 2;
    const int lo = (lane & 15) * (4 * H + 1) + q;               // out: row 0 of column b0 at step t; the lane's part
    hm_lf4* d4 = (hm_lf4*)dfs;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int tl = w + HM_WAVES * s;
        if (tl < ntg) {
            dh[s] += in.g[s];
            const hm_f32x4 d = hm_bwd_point(in.gt[s], in.cn[s], in.cp[s], in.hp[s], z, zb, dh[s], dc[s], pz, pzb);
            d4[tl * 64 + lane] = d;
            if (col_ok) hm_store_gate_grads(out, H, tl, lo, d.x, d.y, d.z, d.w);      // rows f | i | o | g
        }
    }
    if (w == 0) {
        d4[ntg * 64 + lane] = hm_f32x4{q == 0 ? zrow : 0.f, 0.f, 0.f, 0.f};
        if (q == 0 && col_ok) ((hm_gfw*)hm_uniform(out + 4 * H))[lo] = zrow;
    }
}

// sum over the hidden units of each column: lanes q = 0..3 of a wave, then the eight waves in order through red [8][16]
__device__ __forceinline__ void hm_bwd_wave_sum(float v, float* red, int w, int lane) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lane < HM_COLS) red[w * HM_COLS + lane] = v;
}
__device__ __forceinline__ float hm_bwd_col_sum(const float* red, int col) {
    float v = red[col];
#pragma unroll
    for (int i = 1; i < HM_WAVES; ++i) v += red[i * HM_COLS + col];
    return v;
}

template <int NC>
__global__ __launch_bounds__(HM_THREADS) void hmlstm_backward_kernel(const HmBwdParams P) {
    constexpr int NS = 4 * NC;
    extern __shared__ __attribute__((aligned(16))) float hmb_smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 15;
    const int b0 = blockIdx.x * HM_COLS, b = b0 + col;
    const int H1 = P.H1, H2 = P.H2, T = P.T, B = P.B;
    // Under a row bound the steps run from R - 1 down: nothing of the rows t >= R is read (neither the tape nor the
    // forward's outputs nor g_h1 / g_h2), and dfs1 / dfs2 get exact zeros there.  Strides stay those of T.
    const int R = hm_row_bound(P.rows, T);
    const bool col_ok = b < B;
    const int ng1 = (H1 >> 2) + 1, ng2 = (H2 >> 2) + 1, nc1 = hm_bwd_chunks(H1), nc2 = hm_bwd_chunks(H2);
    const int ngmax = ng1 > ng2 ? ng1 : ng2;
    float* dfs = hmb_smem;                              // the B operand: k-groups of 64 float4
    float* red0 = dfs + ngmax * 256;                    // [8][16] partial sums
    float* red1 = red0 + HM_WAVES * HM_COLS;
    for (int i = tid; i < ngmax * 256; i += HM_THREADS) dfs[i] = 0.f;

    const int64_t step = hm_tape_step(H1, H2);
    const float* tape = P.tape + (int64_t)blockIdx.x * T * step;
    const float* st = P.state_in;
    const float* st_h1 = st, *st_c1 = st ? st + (int64_t)H1 * B : nullptr;
    const float* st_h2 = st ? st + (int64_t)(2 * H1 + 1) * B : nullptr, *st_c2 = st ? st + (int64_t)(2 * H1 + 1 + H2) * B : nullptr;
    int last_t = R - 1;
    if (P.len && col_ok) last_t = min(max(P.len[b], 1), R) - 1;
    const float half_a = 0.5f * P.a;

    // Every element of dfs is written on every call: the rows the loop below does not reach, first (in front of the loop
    // nothing of this stays live across it).
    if (R < T) {
        hm_zero_rows(P.dfs1, 4 * H1 + 1, 4 * H1 + 1, 0, R, T, b0, B);
        hm_zero_rows(P.dfs2, 4 * H2 + 1, 4 * H2 + 1, 0, R, T, b0, B);
    }

    float dh1[NS], dc1[NS], dh2[NS], dc2[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) dh1[s] = dc1[s] = dh2[s] = dc2[s] = 0.f;
    float dz1 = 0.f, dz2 = 0.f;                         // per column, the same value in every lane of the column

    HmBwdIn<NS> in1, in2;
    auto load2 = [&](int t) {
        const float* tp = tape + t * step + 80 * H1;
        hm_bwd_load<NS>(in2, tp, tp - step, P.h2, st_h2, st_c2, P.g_h2, P.g_last, t == last_t, H2, T, B, t, b0, col_ok, w, lane);
    };
    auto load1 = [&](int t) {
        const float* tp = tape + t * step;
        hm_bwd_load<NS>(in1, tp, tp - step, P.h1, st_h1, st_c1, P.g_h1, nullptr, false, H1, T, B, t, b0, col_ok, w, lane);
    };
    // the boundaries around a step and the masks of its two clamps, read one step ahead like the tape rows (z1 of the step
    // itself is z1 "before" of the step behind it)
    typedef __attribute__((address_space(1))) const uint8_t hm_gu8;
    float z1t = 0.f, nz1p, nz2p, nm1, nm2;
    auto loadz = [&](int t) {
        nz1p = nz2p = 0.f;
        if (col_ok) {
            if (t > 0) {
                nz1p = (float)((hm_gu8*)hm_uniform(P.z1 + (int64_t)b0 * T + t - 1))[col * T];
                nz2p = (float)((hm_gu8*)hm_uniform(P.z2 + (int64_t)b0 * T + t - 1))[col * T];
            } else if (st) {
                nz1p = ((hm_gf*)hm_uniform(st + (int64_t)2 * H1 * B + b0))[col];
                nz2p = ((hm_gf*)hm_uniform(st + (int64_t)(2 * H1 + 1 + 2 * H2) * B + b0))[col];
            }
        }
        hm_gf* tm = (hm_gf*)hm_uniform(tape + t * step + 80 * (H1 + H2));
        nm1 = tm[col];
        nm2 = tm[16 + col];
    };
    if (col_ok) z1t = (float)((hm_gu8*)hm_uniform(P.z1 + (int64_t)b0 * T + R - 1))[col * T];
    load2(R - 1);
    loadz(R - 1);
    __syncthreads();

    for (int t = R - 1; t >= 0; --t) {
        const float z1p = nz1p, z2p = nz2p, m1 = nm1, m2 = nm2;
        float* out2 = P.dfs2 + ((int64_t)t * B + b0) * (4 * H2 + 1);
        float* out1 = P.dfs1 + ((int64_t)t * B + b0) * (4 * H1 + 1);

        // ---- cell 2: z = z2 of the step before, z_bottom = z1 of this step
        float pz = 0.f, pzb = 0.f;
        hm_bwd_cell<NS>(in2, H2, z2p, z1t, dz2 * m2 * half_a, dh2, dc2, pz, pzb, dfs, out2, col_ok, w, lane);
        float hp2[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) hp2[s] = in2.hp[s];
        load1(t);                                       // in flight behind the products of cell 2
        __syncthreads();                                // dfs holds dfs2 of this step
        {
            float uh[NS], db[NS];
            hm_bwd_product<NC>(uh, P.wt[0], ng2, nc2, dfs, w, lane);
            hm_bwd_product<NC>(db, P.wt[1], ng2, nc1, dfs, w, lane);
            const float keep = (1.0f - z2p) * (1.0f - z1t);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                dh2[s] = dh2[s] * keep + z1t * uh[s];
                pzb += uh[s] * hp2[s];
                dh1[s] += db[s];
            }
        }
        hm_bwd_wave_sum(pz, red0, w, lane);
        hm_bwd_wave_sum(pzb, red1, w, lane);
        __syncthreads();                                // every wave has read dfs2; the partial sums are in place
        dz2 = hm_bwd_col_sum(red0, col);
        dz1 += hm_bwd_col_sum(red1, col);

        // ---- cell 1: z = z1 of the step before, z_bottom = 1, top = h2 of the step before
        pz = 0.f; pzb = 0.f;
        hm_bwd_cell<NS>(in1, H1, z1p, 1.0f, dz1 * m1 * half_a, dh1, dc1, pz, pzb, dfs, out1, col_ok, w, lane);
        if (t > 0) { load2(t - 1); loadz(t - 1); }      // in flight behind the products
        __syncthreads();                                // dfs holds dfs1 of this step
        {
            float ut[NS], uh[NS];
            hm_bwd_product<NC>(ut, P.wt[2], ng1, nc2, dfs, w, lane);
            hm_bwd_product<NC>(uh, P.wt[3], ng1, nc1, dfs, w, lane);
            const float keep = (1.0f - z1p) * 0.0f;     // z_bottom = 1: COPY never happens in cell 1
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                dh1[s] = dh1[s] * keep + uh[s];
                dh2[s] += z1p * ut[s];
                pz += ut[s] * hp2[s];
            }
        }
        hm_bwd_wave_sum(pz, red0, w, lane);
        __syncthreads();                                // every wave has read dfs1
        dz1 = hm_bwd_col_sum(red0, col);
        z1t = z1p;
    }

}
