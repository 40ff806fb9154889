// The reference's pitch arithmetic that more than one kernel needs (kernels_pitch.h: the autocorrelation tracker,
// kernels_cepstrum.h: the cepstral one), each piece stated once.  Every piece keeps a habit of the reference bit for
// bit, so none of them may be restated beside a kernel.
#pragma once

#include "dsp_common.h"

#define PITCH_LDS_FRAMES 2048   // pitch values of an utterance kept in LDS (global memory beyond)

// Frame prologue of the per-frame kernels: block g -> the frame's first sample `first` within its utterance, which
// starts at s0 and has nsamp samples.  False when the block has no frame.
__device__ __forceinline__ bool pitch_frame_locate(const BatchGeom& bg, int64_t g, int32_t S, int64_t& first, int64_t& s0,
                                                   int64_t& nsamp) {
    if (bg.uniform_frames <= 0 && g >= bg.frame_off[bg.n_utt]) return false;   // the grid may be sized by an upper bound of the frame count
    int32_t utt;
    int64_t t;
    dsp_locate(bg, g, utt, t, s0, nsamp);
    first = t * (int64_t)S;
    return true;
}

// ---- centre clipping, pitch.center_clip (pitch.py:145-155), for a frame spread over the registers of one wave ----

// Order statistics are found on the bit patterns: non-negative floats order like unsigned integers, everything else is
// 0xffffffff.  x + 0 turns -0 into +0.
__device__ __forceinline__ uint32_t pitch_clip_key(float x) {
    return x >= 0.f ? __float_as_uint(x + 0.f) : 0xffffffffu;
}

// The clip level: numpy.median of the non-negative samples, whose keys the wave holds NR per lane; NaN when there is
// none.  A 31-step bisection on the bit patterns (ballot + popcount per step): no sort, no LDS, no barrier.
template <int NR>
__device__ __forceinline__ float pitch_clip_level(const uint32_t (&kb)[NR]) {
    // wave-wide count of keys below a candidate: one v_cmp per register, popcount of the masks
    auto count_below = [&](uint32_t cand) {
        int c = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) c += __popcll(__ballot(kb[r] < cand));
        return c;
    };
    int m = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) m += __popcll(__ballot(kb[r] != 0xffffffffu));
    if (m == 0) return __int_as_float(0x7fc00000);         // no non-negative sample: NaN clip level, every sample clips to 0
    // k-th smallest (0-based): the largest v with fewer than k + 1 keys below it, bit by bit
    const int k1 = (m - 1) >> 1, k2 = m >> 1;
    uint32_t v1 = 0;
    for (int bit = 30; bit >= 0; --bit) {
        const uint32_t cand = v1 | (1u << bit);
        if (count_below(cand) <= k1) v1 = cand;
    }
    uint32_t v2 = v1;
    if (k2 != k1 && count_below(v1 + 1) < k2 + 1) {
        uint32_t mn = 0xffffffffu;                         // the next distinct key above v1
#pragma unroll
        for (int r = 0; r < NR; ++r) mn = (kb[r] > v1 && kb[r] < mn) ? kb[r] : mn;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)mn, o, 64);
            mn = other < mn ? other : mn;
        }
        v2 = mn;
    }
    return 0.5f * (__uint_as_float(v1) + __uint_as_float(v2));   // numpy.median: mean of the two middle ones
}

// the non-binary form (pitch.py:152-155); a NaN level fails both comparisons
__device__ __forceinline__ float pitch_center_clip(float x, float med) {
    return x > med ? x - med : (x < -med ? x + med : 0.f);
}

// ---- the causal complex FIR of sigproc.window (sigproc.py:22-46), y[k] = sum_{m < n} h[m] c[k - m] ----
// A lane owns W consecutive outputs from kl and W from kh, keeps the 2 W samples it needs in a register ring and reads
// one new sample per output group and tap: 3 LDS reads per 4 W multiply-adds.  cl[] needs n readable zeros below index
// 0 (the samples before the frame), so the tap loop is uniform and branch free; n is a multiple of W.
template <int W>
__device__ __forceinline__ void pitch_fir_pair(const float* cl, const float2* h, int kl, int kh, int n, float (&alr)[W],
                                               float (&ali)[W], float (&ahr)[W], float (&ahi)[W]) {
    float wl[W], wh[W];                                    // ring: the sample at position p sits in slot p % W
#pragma unroll
    for (int e = 0; e < W; ++e) {
        wl[e] = cl[kl + e];
        wh[e] = cl[kh + e];
        alr[e] = ali[e] = ahr[e] = ahi[e] = 0.f;
    }
    for (int m0 = 0; m0 < n; m0 += W) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int m = m0 + j;
            if (m > 0) {                                   // position k0 - m enters slot (-m) % W == (W - j) % W
                wl[(W - j) % W] = cl[kl - m];
                wh[(W - j) % W] = cl[kh - m];
            }
            const float2 hm = h[m];
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float vl = wl[(e - j + W) % W], vh = wh[(e - j + W) % W];
                alr[e] = fmaf(hm.x, vl, alr[e]); ali[e] = fmaf(hm.y, vl, ali[e]);
                ahr[e] = fmaf(hm.x, vh, ahr[e]); ahi[e] = fmaf(hm.y, vh, ahi[e]);
            }
        }
    }
}

// ---- radix-2 transforms of L complex points in LDS by one wave, tw[k] = exp(-2 pi i k / L), k < L / 2 ----
// A twiddle of exactly one is never multiplied: a silent frame (log 0 = -inf in every bin) then comes out of the
// inverse as [inf, nan, nan, ...], as NumPy's does.

// forward, decimation in frequency: natural order in, bit-reversed out
template <int L>
__device__ __forceinline__ void pitch_fft_dif(float2* buf, const float2* tw, int lane) {
    for (int half = L / 2; half >= 1; half >>= 1) {
        const int tstep = (L / 2) / half;
        for (int b = lane; b < L / 2; b += 64) {
            const int j = b & (half - 1), i0 = ((b - j) << 1) + j, i1 = i0 + half;
            const float2 u = buf[i0], v = buf[i1];
            float2 d = make_float2(u.x - v.x, u.y - v.y);
            if (j) d = cmul(d, tw[j * tstep]);
            buf[i0] = make_float2(u.x + v.x, u.y + v.y);
            buf[i1] = d;
        }
        __syncthreads();
    }
}

// inverse (not scaled), decimation in time with conjugate twiddles: bit-reversed in, natural order out
template <int L>
__device__ __forceinline__ void pitch_ifft_dit(float2* buf, const float2* tw, int lane) {
    for (int half = 1; half <= L / 2; half <<= 1) {
        const int tstep = (L / 2) / half;
        for (int b = lane; b < L / 2; b += 64) {
            const int j = b & (half - 1), i0 = ((b - j) << 1) + j, i1 = i0 + half;
            const float2 u = buf[i0];
            float2 v = buf[i1];
            if (j) {
                const float2 w = tw[j * tstep];
                v = cmul(v, make_float2(w.x, -w.y));
            }
            buf[i0] = make_float2(u.x + v.x, u.y + v.y);
            buf[i1] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
}

// ---- the trackers: pitch.smooth (pitch.py:157-164), pitch.max_pitch (pitch.py:166-172) and the octave-repair sweeps
// of pitch.robust_max_pitch (pitch.py:191-206).  Sequential over the frames of an utterance, fp64 as the reference ----

// smooth() works IN PLACE: row i becomes the mean of rows [max(i - degree, 0), right), where rows below i are already
// smoothed and right = i + degree if i + degree < T else T - 1.  So the last rows average over a window that EXCLUDES
// the last row, and a one-frame utterance averages over nothing.
__device__ __forceinline__ void pitch_window_bounds(int i, int degree, int T, int& left, int& right) {
    left = i - degree >= 0 ? i - degree : 0;
    right = i + degree < T ? i + degree : T - 1;           // exclusive
}

// numpy's mean over rows [left, right) of one column: the first value, then the others added in order, divided once;
// NaN when the window is empty (whose arg-max is index 0).  row(r) yields row r of the column.
template <class Row>
__device__ __forceinline__ double pitch_window_mean(int left, int right, Row row) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double acc = qnan;
    bool have = false;
    for (int r = left; r < right; ++r) {
        const double v = row(r);
        acc = have ? acc + v : v;
        have = true;
    }
    return have ? acc / (double)(right - left) : qnan;
}

__device__ __forceinline__ void pitch_argmax_combine(double& v, int& ix, double ov, int oix) {
    // numpy.argmax order: a NaN beats everything, then the larger value, then the smaller index
    const bool vn = v != v, on = ov != ov;
    const bool take = (on && !vn) || (on == vn && (ov > v || (ov == v && oix < ix))) || (on && vn && oix < ix);
    if (take) { v = ov; ix = oix; }
}

// every lane's best (value, index) -> the wave's, in all lanes.  A lane without a candidate brings (-inf, 0x7fffffff),
// which loses to every real one.
__device__ __forceinline__ void pitch_wave_argmax(double& v, int& ix) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(ix, o, 64);
        pitch_argmax_combine(v, ix, ov, oi);
    }
}

// pitch.py:169-170: arg-max index on the 10 kHz lag / quefrency grid -> Hz
__device__ __forceinline__ double pitch_hz(int bias, int idx) {
    return 1.0 / (0.0001 * (double)(bias + idx));
}

// pitch.py:199-204: a value whose double is within 50 Hz of its (already repaired) neighbour is an octave error; one
// sweep up against the left neighbour, one down against the right.  One dependency chain: a single lane runs it.
template <class Get, class Put>
__device__ __forceinline__ void pitch_octave_repair(Get get, Put put, int T) {
    const double C = 50.0;
    for (int i = 1; i < T; ++i) {                          // pitch.py:199-201
        const double p = get(i);
        if (fabs(2.0 * p - get(i - 1)) < C && p < 170.0) put(i, 2.0 * p);
    }
    for (int i = T - 2; i > 0; --i) {                      // pitch.py:202-204
        const double p = get(i);
        if (fabs(2.0 * p - get(i + 1)) < C && p < 170.0) put(i, 2.0 * p);
    }
}

// The pitch values of one utterance while a kernel walks them: the first PITCH_LDS_FRAMES in LDS (`lds`, a __shared__
// array of that size in the kernel), the rest in place in global memory (`glob`, the utterance's slice).  P is
// `const double` where the kernel only reads.  The caller puts a barrier between put / load and the reads of other lanes.
template <class P>
struct PitchTrackStore {
    double* lds;
    P* glob;
    __device__ __forceinline__ double get(int i) const { return i < PITCH_LDS_FRAMES ? lds[i] : glob[i]; }
    __device__ __forceinline__ void put(int i, double v) const { if (i < PITCH_LDS_FRAMES) lds[i] = v; else glob[i] = v; }
    __device__ __forceinline__ void load(int T, int lane) const {
        for (int i = lane; i < T && i < PITCH_LDS_FRAMES; i += 64) lds[i] = glob[i];
    }
    __device__ __forceinline__ void flush(int T, int lane) const {
        for (int i = lane; i < T && i < PITCH_LDS_FRAMES; i += 64) glob[i] = lds[i];
    }
};
