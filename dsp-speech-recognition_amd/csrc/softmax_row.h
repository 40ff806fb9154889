// One row of logits on one wavefront: the softmax and the arg-max that the ensemble gate (kernels_ensemble.h) and the loss
// kernels (kernels_loss.h) share, so that both return the same bits.  Device functions only.  gfx950 only (wave64).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// Sum over the 64 lanes in a fixed order (the xor butterfly: every lane ends with the same bits, on every call).
__device__ __forceinline__ double ens_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct RowSoftmax {
    float mx;       // the largest logit of the row
    int pred;       // the lowest index among the largest logits (0 if no lane compares equal: a NaN logit)
    double e, s;    // this lane's exp(logit - mx) (0 behind the row) and the row's sum of them
    float p;        // this lane's probability: e / s rounded once
};

// model.py:156-157 for one row: lane c < C holds logit c in `lf` with `mine` set; every other lane passes (-INFINITY, false).
//   p    = softmax in fp64 (max subtracted), rounded to fp32          F.softmax(out, dim=1)
//   pred = the lowest index among the largest logits                  torch.max(out, 1)
// The whole wave must call it (it shuffles over all 64 lanes).
__device__ __forceinline__ RowSoftmax row_softmax_wave(float lf, bool mine) {
    RowSoftmax r;
    float mx = lf;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const unsigned long long at_max = __ballot(mine && lf == mx);
    r.mx = mx;
    r.pred = at_max ? __ffsll(at_max) - 1 : 0;
    r.e = mine ? exp((double)lf - (double)mx) : 0.0;
    r.s = ens_wave_sum(r.e);
    r.p = (float)(r.e / r.s);
    return r;
}

// The same row by ONE thread, for a kernel that holds a row per lane: the largest logit, the lowest index that holds it, and the
// sum of exp(logit - mx) added in the order of the butterfly above -- level o adds entry i + o to entry i for i < o, o = 32 .. 1,
// with exact zeros behind the row -- so mx, pred and s equal row_softmax_wave's in every bit (fp addition is commutative, and
// exp sees the same argument).  `row` points at the C logits of the row; nothing behind them is read.
__device__ __forceinline__ void row_softmax_thread(const float* __restrict__ row, int C, float& mx_out, int& pred_out, double& s_out) {
    float mx = row[0];
    int pred = 0;
    for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (v > mx) { mx = v; pred = c; }
    }
    double e[64];
#pragma unroll
    for (int c = 0; c < 64; ++c) {
        e[c] = 0.0;
        if (c < C) e[c] = exp((double)row[c] - (double)mx);      // (C is uniform over the launch: a scalar branch)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < o; ++i) e[i] += e[i + o];
    mx_out = mx;
    pred_out = pred;
    s_out = e[0];
}
