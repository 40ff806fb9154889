// Launch plumbing shared by the kernel headers and dsp_frontend.hip: the index tables of ragged batches (who builds
// them, where they live, when the buffer goes back to the pool), the run-time -> compile-time wave dtype dispatch,
// and the delta normaliser.
#pragma once

#include <type_traits>

#include "dsp_common.h"
#include "kernels_generic.h"
#include "workspace.h"

// f(std::integral_constant<int, DTYPE>) for the run-time wave dtype.  Callers have validated it: anything but int16 is float.
template <class F>
static inline auto dsp_dispatch_wave(int dtype, F&& f) {
    if (dtype == DSP_WAVE_I16) return f(std::integral_constant<int, DSP_WAVE_I16>{});
    return f(std::integral_constant<int, DSP_WAVE_F32>{});
}

// 1 / (2 sum_{i=1..N} i^2): the regression normaliser of the delta features (base.py:74)
static inline float dsp_delta_inv_den(int N) {
    int den = 0;
    for (int i = 1; i <= N; ++i) den += i * i;
    return (float)(1.0 / (2.0 * den));
}

// Ragged index tables built by the caller in one launch together with its own (dsp_mfcc_delta_batch).
struct DspRaggedTables {
    int32_t* group_off = nullptr;   // [n_utt + 1] prefix of ceil(T_b / 2^shift)
    int32_t* group_utt = nullptr;   // utterance of every group
    int shift = 0;                  // 3: NFFT=512 kernel (8 frames per wave), 2: NFFT=1536 kernel
    // a second set for another group size (a dsp_layout holds the tables of the int16 VAD kernel's 8-frame groups beside
    // those of the 4-frame groups the other VAD kernels use, when the two differ)
    int32_t* group_off2 = nullptr;
    int32_t* group_utt2 = nullptr;
    int shift2 = 0;
};

// Ragged batches: group_off[b] = sum_{i<b} ceil(T_i / 2^shift) (exclusive prefix, single block), then the
// utterance of every group.  Both are tiny next to the main kernel and run on the same stream.
__global__ __launch_bounds__(1024) void f512_group_prefix_kernel(const int64_t* __restrict__ frame_off, int32_t n_utt,
                                                                 int32_t shift, int32_t* __restrict__ group_off,
                                                                 int32_t* __restrict__ group_utt = nullptr,
                                                                 int32_t tile_shift = 0,
                                                                 int64_t* __restrict__ tile_off = nullptr,
                                                                 double* __restrict__ zero_stats = nullptr) {
    // optional second table in the same launch: tile_off[b] = sum_{i<b} ceil(T_i / 2^tile_shift) (the delta pass)
    __shared__ int32_t wsum[16], wsum_t[16];
    const int tid = threadIdx.x;
    const int per = (n_utt + 1023) / 1024;
    const int lo = tid * per, hi = min(lo + per, n_utt);
    const int64_t rnd = ((int64_t)1 << shift) - 1, rnd_t = ((int64_t)1 << tile_shift) - 1;
    int32_t sum = 0, sum_t = 0;
    for (int b = lo; b < hi; ++b) {
        const int64_t T = frame_off[b + 1] - frame_off[b];
        sum += (int32_t)((T + rnd) >> shift);
        sum_t += (int32_t)((T + rnd_t) >> tile_shift);
        if (zero_stats != nullptr) { zero_stats[2 * b] = 0.0; zero_stats[2 * b + 1] = 0.0; }
    }
    // inclusive scan of the per-thread sums: inside each wave with shuffles, across the 16 waves through LDS
    int32_t inc = sum, inc_t = sum_t;
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t v = __shfl_up(inc, off, 64), vt = __shfl_up(inc_t, off, 64);
        if (lane >= off) { inc += v; inc_t += vt; }
    }
    if (lane == 63) { wsum[w] = inc; wsum_t[w] = inc_t; }
    __syncthreads();
    int32_t before = 0, before_t = 0, total = 0, total_t = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int32_t a = wsum[k], at = wsum_t[k];
        if (k < w) { before += a; before_t += at; }
        total += a;
        total_t += at;
    }
    inc += before;
    inc_t += before_t;
    int32_t run = inc - sum;
    int64_t run_t = inc_t - sum_t;
    for (int b = lo; b < hi; ++b) {
        group_off[b] = run;
        const int64_t T = frame_off[b + 1] - frame_off[b];
        const int32_t n = (int32_t)((T + rnd) >> shift);
        if (group_utt != nullptr)   // small batches: fill the group -> utterance table in the same launch
            for (int32_t g = 0; g < n; ++g) group_utt[run + g] = b;
        run += n;
        if (tile_off != nullptr) {
            tile_off[b] = run_t;
            run_t += (T + rnd_t) >> tile_shift;
        }
    }
    if (tid == 1023) {
        group_off[n_utt] = total;
        if (tile_off != nullptr) tile_off[n_utt] = total_t;
    }
}

__global__ __launch_bounds__(256) void f512_group_fill_kernel(const int32_t* __restrict__ group_off, int32_t n_utt,
                                                              int32_t* __restrict__ group_utt) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < n_utt; b += gridDim.x * blockDim.x)
        for (int g = group_off[b]; g < group_off[b + 1]; ++g) group_utt[g] = b;
}

// Builds both ragged index tables on `st`: one launch for small batches, prefix + parallel fill otherwise.
static inline void f512_build_group_tables(const int64_t* frame_off, int32_t n_utt, int32_t shift,
                                           int32_t* group_off, int32_t* group_utt, hipStream_t st,
                                           int64_t* tile_off = nullptr, double* zero_stats = nullptr) {
    if (n_utt <= 4096) {
        f512_group_prefix_kernel<<<1, 1024, 0, st>>>(frame_off, n_utt, shift, group_off, group_utt, DT_SHIFT, tile_off, zero_stats);
        return;
    }
    f512_group_prefix_kernel<<<1, 1024, 0, st>>>(frame_off, n_utt, shift, group_off, nullptr, DT_SHIFT, tile_off, zero_stats);
    const int fill_blocks = (int)((n_utt + 255) / 256 < 1024 ? (n_utt + 255) / 256 : 1024);
    f512_group_fill_kernel<<<fill_blocks, 256, 0, st>>>(group_off, n_utt, group_utt);
}

// Points P.group_off / P.group_utt at the tables of 2^shift-frame groups: the caller's prebuilt ones where their group
// size matches, otherwise tables built on `st` in a pooled, event-guarded workspace (no host sync) that is left in `w`
// for dsp_ragged_tables_release.  `bound` >= sum ceil(T_b / 2^shift).  False: no workspace to be had.
template <class Params>
static inline bool dsp_ragged_tables_acquire(Params& P, const DspRaggedTables* pre, int shift, const BatchGeom& bg,
                                             int64_t bound, hipStream_t st, DspWorkspace*& w) {
    w = nullptr;
    if (pre != nullptr && pre->shift == shift) {
        P.group_off = pre->group_off;
        P.group_utt = pre->group_utt;
    } else if (pre != nullptr && pre->shift2 == shift) {
        P.group_off = pre->group_off2;
        P.group_utt = pre->group_utt2;
    } else {
        w = dsp_workspace_pool().acquire(((size_t)bg.n_utt + 1 + (size_t)bound) * sizeof(int32_t), st);
        if (!w) return false;
        int32_t* group_off = static_cast<int32_t*>(w->ptr);
        int32_t* group_utt = group_off + bg.n_utt + 1;
        f512_build_group_tables(bg.frame_off, bg.n_utt, shift, group_off, group_utt, st);
        P.group_off = group_off;
        P.group_utt = group_utt;
    }
    return true;
}

// Hands the workspace (if one was leased) back behind the launch on `st`; the launch's `rc`, or DSP_EHIP if that fails.
static inline int dsp_ragged_tables_release(DspWorkspace* w, hipStream_t st, int rc) {
    if (w != nullptr && dsp_workspace_pool().release(w, st) != 0 && rc == DSP_OK) rc = DSP_EHIP;
    return rc;
}
