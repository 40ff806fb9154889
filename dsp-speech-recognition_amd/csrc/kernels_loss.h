// The scoring of the reference on the device: F.cross_entropy at its defaults with its gradient (model.py:141-147), the
// prediction of model.py:156-157, and the epoch metrics RNNModel.test / EnsembleModel.test collect on the host batch by batch
// (model.py:162-187, ensemble.py:44-64: the err list, accuracy_score, confusion_matrix), accumulated in ONE caller-owned
// block of device memory.  Two launches (include/dsp_frontend.h: dsp_xent_metrics_batch):
//   xent_rows_kernel    one wavefront per clip: softmax / arg-max (softmax_row.h, shared with the ensemble gate), nll, prob,
//                       pred and the scaled gradient.  n_scored, which the gradient is divided by, is an integer count over the
//                       labels alone, so every workgroup counts it for itself in front of its rows: no launch and no buffer
//                       stands between the count and the scaling.
//   xent_reduce_kernel  ONE workgroup, one clip per thread: the per-clip values again (row_softmax_thread adds in the wave
//                       butterfly's order: the same bits), the fp64 loss sum in a fixed order, the counters, every confusion
//                       cell by the one thread that owns it, and the wrong list by a fixed prefix scan in clip order.  (One
//                       wave per clip here, as in the first launch, left fifteen of sixteen waves' worth of lanes idle and ran
//                       the clips one behind the other: 63 us at 512 clips against 10 at 32.)
// No atomics, no memset, no allocation; every store is a plain C++ assignment.  gfx950 only (wave64).
// The kernels here are `static`: csrc/dsp_adv.hip launches them too, from a translation unit of its own.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "softmax_row.h"

#define XENT_ROWS_PER_BLOCK 4            // xent_rows_kernel: one wave per clip, 256 threads
#define XENT_REDUCE_THREADS 512          // xent_reduce_kernel: one workgroup of 8 waves, one clip per thread
#define XENT_REDUCE_WAVES (XENT_REDUCE_THREADS / 64)
#define XENT_MAX_UTT 16384
#define XENT_MAX_CLASSES 64
#define XENT_IGNORE_INDEX (-100)         // torch's ignore_index
#define XENT_MAX_WRONG (1 << 24)         // wrong_capacity

// The epoch state (include/dsp_frontend.h): int64 counts[8] | fp64 loss_sum | int64 confusion[C][C] | int32 wrong[cap][3].
#define XENT_N_COUNTS 8
enum { XC_SEEN = 0, XC_SCORED, XC_CORRECT, XC_IGNORED, XC_BAD_LABEL, XC_WRONG_TOTAL, XC_CALLS, XC_RESERVED };

__host__ __device__ inline int64_t xent_state_bytes(int32_t C, int32_t cap) {
    const int64_t b = (int64_t)XENT_N_COUNTS * 8 + 8 + (int64_t)C * C * 8 + (int64_t)cap * 12;
    return (b + 7) / 8 * 8;
}

struct XentParams {
    const float* logits;
    int64_t ld_logits;
    int32_t n_utt, C;
    const int64_t* labels;
    const int32_t* pred_in;
    const float* grad_out;
    float* nll;
    float* loss;
    int32_t* pred;
    float* prob;
    float* dlogits;
    int64_t ld_dlogits;
    long long* state;
    int32_t wrong_cap;
};

// The per-clip values both kernels need, from one wave.  `live`: the wave has a row (wave-uniform).
struct XentRow {
    RowSoftmax sm;
    long long y;        // the label as given
    bool scored;        // y in [0, C)
    double nll;         // logsumexp(row) - row[y], unrounded; 0 where the row is not scored
};

__device__ __forceinline__ XentRow xent_row_wave(const XentParams& P, int64_t b, bool live, int lane) {
    XentRow r;
    const bool mine = live && lane < P.C;              // no lane reads outside its row: idle lanes load nothing
    float lf = -INFINITY;
    if (mine) lf = P.logits[b * P.ld_logits + lane];
    r.sm = row_softmax_wave(lf, mine);
    r.y = XENT_IGNORE_INDEX;
    if (live) r.y = P.labels[b];
    r.scored = r.y >= 0 && r.y < P.C;
    const double ly = (double)__shfl(lf, r.scored ? (int)r.y : 0, 64);
    r.nll = r.scored ? (log(r.sm.s) + (double)r.sm.mx) - ly : 0.0;
    return r;
}

static __global__ __launch_bounds__(64 * XENT_ROWS_PER_BLOCK) void xent_rows_kernel(XentParams P) {
    __shared__ int s_cnt[XENT_ROWS_PER_BLOCK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * XENT_ROWS_PER_BLOCK + w;
    const bool live = b < P.n_utt;                    // (no wave leaves early: the count below synchronises the workgroup)
    int n_scored = 0;
    if (P.dlogits != nullptr) {
        int c = 0;
        for (int i = threadIdx.x; i < P.n_utt; i += 64 * XENT_ROWS_PER_BLOCK) {
            const long long y = P.labels[i];
            c += (y >= 0 && y < P.C) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_cnt[w] = c;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < XENT_ROWS_PER_BLOCK; ++k) n_scored += s_cnt[k];
    }
    const XentRow r = xent_row_wave(P, b, live, lane);
    if (!live) return;
    const bool mine = lane < P.C;
    if (lane == 0) {
        if (P.nll != nullptr) P.nll[b] = (float)r.nll;
        if (P.pred != nullptr) P.pred[b] = r.sm.pred;
    }
    if (mine && P.prob != nullptr) P.prob[b * P.C + lane] = r.sm.p;
    if (mine && P.dlogits != nullptr) {
        float g = 0.0f;                               // exact zeros in an ignored row
        if (r.scored) {
            const double go = P.grad_out != nullptr ? (double)P.grad_out[0] : 1.0;
            const double d = r.sm.e / r.sm.s - (lane == (int)r.y ? 1.0 : 0.0);
            g = (float)(d * go / (double)n_scored);
        }
        P.dlogits[b * P.ld_dlogits + lane] = g;
    }
}

// A clip as the reduce kernel keeps it in LDS: bits 0-5 the true label, 6-11 the scored label, then the flags.
#define XR_SCORED 0x1000u
#define XR_WRONG 0x2000u
#define XR_CELL 0x4000u                  // the scored label lies in [0, C): the clip has a confusion cell

static __global__ __launch_bounds__(XENT_REDUCE_THREADS) void xent_reduce_kernel(XentParams P) {
    __shared__ __attribute__((aligned(8))) uint16_t s_code[XENT_MAX_UTT];
    __shared__ double s_sum[XENT_REDUCE_WAVES];
    __shared__ int s_part[XENT_REDUCE_WAVES][5];      // scored, correct, ignored, bad_label, wrong
    __shared__ int s_scan[XENT_REDUCE_WAVES];
    __shared__ long long s_seen0, s_wrong0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int C = P.C, n = P.n_utt;
    const int n4 = (n + 3) & ~3;                      // the codes are read four at a time: zero codes behind the batch

    // 1. every clip by one thread (row_softmax_thread: the bits of the wave's softmax); thread t takes the clips t, t + 512, ...
    //    in ascending order and adds their nll as it goes
    double acc = 0.0;
    int part[5] = {0, 0, 0, 0, 0};
    for (int b = tid; b < n4; b += XENT_REDUCE_THREADS) {
        unsigned code = 0;
        if (b < n) {
            const long long y = P.labels[b];
            const float* row = P.logits + (int64_t)b * P.ld_logits;
            if (y >= 0 && y < C) {
                float mx;
                int sl;
                double s;
                row_softmax_thread(row, C, mx, sl, s);
                if (P.pred_in != nullptr) sl = P.pred_in[b];
                const bool cell = sl >= 0 && sl < C, wrong = sl != (int)y;
                code = XR_SCORED | (unsigned)y | (cell ? XR_CELL | ((unsigned)sl << 6) : 0u) | (wrong ? XR_WRONG : 0u);
                acc += (log(s) + (double)mx) - (double)row[y];
                part[0] += 1;
                part[1] += wrong ? 0 : 1;
                part[4] += wrong ? 1 : 0;
            } else {
                part[2] += 1;
                part[3] += y == XENT_IGNORE_INDEX ? 0 : 1;
            }
        }
        s_code[b] = (uint16_t)code;
    }
    acc = ens_wave_sum(acc);                          // the 64 lanes of a wave in the butterfly's fixed order
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part[j] += __shfl_xor(part[j], o, 64);
    if (lane == 0) {
        s_sum[w] = acc;
        for (int j = 0; j < 5; ++j) s_part[w][j] = part[j];
    }
    __syncthreads();

    // 2. one thread adds the waves' partial sums in order, writes the loss and moves the counters
    if (tid == 0) {
        double sum = 0.0;
        long long t[5] = {0, 0, 0, 0, 0};
        for (int k = 0; k < XENT_REDUCE_WAVES; ++k) {
            sum += s_sum[k];
            for (int j = 0; j < 5; ++j) t[j] += s_part[k][j];
        }
        if (P.loss != nullptr) P.loss[0] = (float)(sum / (double)t[0]);        // 0 / 0 = NaN with no scored clip, as torch
        long long seen0 = 0, wrong0 = 0;
        if (P.state != nullptr) {
            long long* cnt = P.state;
            seen0 = cnt[XC_SEEN];
            wrong0 = cnt[XC_WRONG_TOTAL];
            cnt[XC_SEEN] = seen0 + n;
            cnt[XC_SCORED] += t[0];
            cnt[XC_CORRECT] += t[1];
            cnt[XC_IGNORED] += t[2];
            cnt[XC_BAD_LABEL] += t[3];
            cnt[XC_WRONG_TOTAL] = wrong0 + t[4];
            cnt[XC_CALLS] += 1;
            double* loss_sum = reinterpret_cast<double*>(P.state + XENT_N_COUNTS);
            loss_sum[0] += sum;
        }
        s_seen0 = seen0;
        s_wrong0 = wrong0;
    }
    if (P.state == nullptr) return;                   // (uniform over the workgroup)
    __syncthreads();

    // 3. the confusion matrix: thread t owns the cells t, t + 512, ... and counts its clips itself, four codes per LDS read
    //    (every lane reads the same address: a broadcast)
    long long* conf = P.state + XENT_N_COUNTS + 1;
    const uint2* code4 = reinterpret_cast<const uint2*>(s_code);
    for (int cell = tid; cell < C * C; cell += XENT_REDUCE_THREADS) {
        const unsigned want = XR_SCORED | XR_CELL | (unsigned)(cell / C) | ((unsigned)(cell % C) << 6);
        const unsigned mask = 0xffffu & ~XR_WRONG;
        int c = 0;
        for (int q = 0; q < n4 / 4; ++q) {
            const uint2 v = code4[q];
            c += ((v.x & mask) == want ? 1 : 0) + (((v.x >> 16) & mask) == want ? 1 : 0) + ((v.y & mask) == want ? 1 : 0) +
                 (((v.y >> 16) & mask) == want ? 1 : 0);
        }
        if (c) conf[cell] += c;
    }

    // 4. the wrong list in clip order: thread t holds the clips [t K, (t + 1) K); an exclusive scan of the threads' counts
    //    (shuffles within a wave, the wave totals through LDS) gives every thread its first slot
    const int K = (n + XENT_REDUCE_THREADS - 1) / XENT_REDUCE_THREADS;
    const int b0 = min(tid * K, n), b1 = min(b0 + K, n);
    int mine = 0;
    for (int b = b0; b < b1; ++b) mine += (s_code[b] & XR_WRONG) ? 1 : 0;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_scan[w] = incl;
    __syncthreads();
    int before = incl - mine;
    for (int k = 0; k < w; ++k) before += s_scan[k];
    int32_t* wrong = reinterpret_cast<int32_t*>(conf + (int64_t)C * C);
    long long slot = s_wrong0 + before;
    for (int b = b0; b < b1; ++b) {
        const unsigned code = s_code[b];
        if (!(code & XR_WRONG)) continue;
        if (slot >= 0 && slot < P.wrong_cap) {       // (a block that was never reset must not steer a store)
            int sl = (int)((code >> 6) & 63u);
            if (P.pred_in != nullptr) sl = P.pred_in[b];
            wrong[slot * 3 + 0] = (int32_t)(s_seen0 + b);
            wrong[slot * 3 + 1] = sl;
            wrong[slot * 3 + 2] = (int32_t)(code & 63u);
        }
        ++slot;
    }
}

// dsp_metrics_reset: every 32-bit word of the block becomes 0 (a recorded memset of more than 4 bytes replays wrong).
static __global__ __launch_bounds__(256) void xent_reset_kernel(int32_t* __restrict__ words, long long n_words) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (long long)gridDim.x * 256) words[i] = 0;
}
