// Pitch scores of pitch.pitch_detect_sr (pitch.py:96-132), one workgroup per frame of the 10 kHz
// signal:
//   centre clipping at the median of the non-negative samples   pitch.center_clip   pitch.py:145-155
//   causal complex band-pass FIR truncated to the frame, |.|     sigproc.window      sigproc.py:22-46
//   autocorrelation at lags lag_min .. lag_max - 1               sigproc.acr         sigproc.py:48-53
// The FIR taps (inverse FFT of the ideal band, times the window, times 2 pi) are built on the host
// in fp64 and handed over as float2[L].  Everything else (smoothing across frames, arg-max, octave
// repair) is O(T * lags) sequential host logic in the Python mirror, as in the reference.
#pragma once

#include "pitch_common.h"

#define PITCH_THREADS 256
#define PITCH_MAX_L 1024

// dynamic LDS of pitch_scores_kernel: the carve-up at its top, in bytes
inline size_t pitch_scores_lds_bytes(int L, int P) {
    return ((size_t)P + (size_t)((L + 3) & ~3) + 2 * (size_t)L + (size_t)L) * sizeof(float);
}

// frames: rectangular, frame t = samples [t S, t S + L) of the utterance, zero padded (to_frames).
__global__ __launch_bounds__(PITCH_THREADS) void pitch_scores_kernel(
    const float* __restrict__ sig, BatchGeom bg, int32_t L, int32_t S, int32_t P /* pow2 >= L */,
    const float2* __restrict__ taps, int32_t do_clip, int32_t lag_min, int32_t n_lags,
    float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) float smem_p[];
    float* key = smem_p;                                   // [P]  sort keys
    float* cl = key + P;                                   // [L]  clipped frame, later |filtered|
    float2* h = reinterpret_cast<float2*>(cl + ((L + 3) & ~3));   // [L]  FIR taps
    float* f = reinterpret_cast<float*>(h + L);            // [L]  |filtered frame|
    __shared__ int s_m;
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    int64_t first, s0, nsamp;
    if (!pitch_frame_locate(bg, g, S, first, s0, nsamp)) return;
    if (tid == 0) s_m = 0;
    __syncthreads();
    // ---- load the frame; sort keys: non-negative samples, everything else +inf ----
    int mloc = 0;
    for (int i = tid; i < P; i += PITCH_THREADS) {
        float x = 0.f;
        const bool in = i < L;
        if (in && first + i < nsamp) x = sig[s0 + first + i];
        if (in) cl[i] = x;
        const bool nn = in && x >= 0.f;
        key[i] = nn ? x : __int_as_float(0x7f800000);
        mloc += nn ? 1 : 0;
    }
    for (int i = tid; i < L; i += PITCH_THREADS) h[i] = taps[i];
    if (do_clip) {
        if (mloc) atomicAdd(&s_m, mloc);
        __syncthreads();
        // bitonic sort, ascending
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < P; i += PITCH_THREADS) {
                    const int p = i ^ j;
                    if (p > i) {
                        const float a = key[i], b = key[p];
                        const bool up = (i & k) == 0;
                        if ((a > b) == up) { key[i] = b; key[p] = a; }
                    }
                }
                __syncthreads();
            }
        }
        const int m = s_m;
        // numpy.median: mean of the two middle order statistics; no non-negative sample -> NaN
        const float med = m > 0 ? 0.5f * (key[(m - 1) >> 1] + key[m >> 1]) : __int_as_float(0x7fc00000);
        for (int i = tid; i < L; i += PITCH_THREADS) {
            const float x = cl[i];
            cl[i] = x > med ? x - med : (x < -med ? x + med : 0.f);
        }
    }
    __syncthreads();
    // ---- y[k] = sum_{j <= k} c[j] h[k - j]; outputs k and L - 1 - k share a thread (L + 1 taps each) ----
    for (int k1 = tid; 2 * k1 < L; k1 += PITCH_THREADS) {
        const int k2 = L - 1 - k1;
        float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f;
        int j = 0;
        for (; j <= k1; ++j) {
            const float c = cl[j];
            const float2 ha = h[k1 - j], hb = h[k2 - j];
            ar = fmaf(c, ha.x, ar); ai = fmaf(c, ha.y, ai);
            br = fmaf(c, hb.x, br); bi = fmaf(c, hb.y, bi);
        }
        for (; j <= k2; ++j) {
            const float c = cl[j];
            const float2 hb = h[k2 - j];
            br = fmaf(c, hb.x, br); bi = fmaf(c, hb.y, bi);
        }
        f[k1] = sqrtf(fmaf(ar, ar, ai * ai));
        if (k2 != k1) f[k2] = sqrtf(fmaf(br, br, bi * bi));
    }
    __syncthreads();
    // ---- autocorrelation, one lag per thread ----
    for (int q = tid; q < n_lags; q += PITCH_THREADS) {
        const int n = lag_min + q;
        float acc = 0.f;
        if (n == 0) {
            for (int i = 0; i < L; ++i) acc = fmaf(f[i], f[i], acc);
            acc /= (float)L;
        } else if (n < L) {
            for (int i = 0; i + n < L; ++i) acc = fmaf(f[i], f[i + n], acc);
            acc /= (float)(L - n);
        } else {
            acc = __int_as_float(0x7fc00000);   // numpy: sum of an empty product / 0 -> nan
        }
        scores[g * n_lags + q] = acc;
    }
}

// Register-blocked variant, one wavefront per frame.  Every lane owns W consecutive FIR outputs at
// the bottom of the frame and W at the top, so all lanes do the same work in pitch_fir_pair: 3 LDS
// reads per 4 W multiply-adds instead of 3 per 4.  The frame length is a run-time value here, so
// outputs and taps are padded to Lp, the next multiple of W.  The autocorrelation is blocked the same
// way (4 lags per lane).  The clip level comes from the frame's bit patterns held in registers
// (pitch_clip_level): no sort, no LDS, no barrier.
// Requires lag_min % 4 == 0, n_lags <= 256, ceil(L / (2 W)) <= 64 (so L <= 512).
#define PITCH2_GUARD 256   // zeros behind f[] (>= lag_max + 4)

// dynamic LDS of pitch_scores_kernel_v2<W>: the carve-up at its top, in bytes
template <int W>
inline size_t pitch_scores_v2_lds_bytes(int L) {
    const size_t Lp = (size_t)((L + W - 1) / W * W);
    return (2 * Lp + 2 * Lp + Lp + PITCH2_GUARD) * sizeof(float);
}

template <int W>
__global__ __launch_bounds__(64) void pitch_scores_kernel_v2(
    const float* __restrict__ sig, BatchGeom bg, int32_t L, int32_t S, int32_t P, const float2* __restrict__ taps,
    int32_t do_clip, int32_t lag_min, int32_t n_lags, float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) float smem_p[];
    const int Lp = (L + W - 1) / W * W;                    // outputs are produced in chunks of W
    float* cl0 = smem_p;                                   // [Lp zeros][Lp samples]: index i lives at cl0[Lp + i]
    float2* h = reinterpret_cast<float2*>(cl0 + 2 * Lp);   // [Lp] taps, zero beyond L
    float* f = reinterpret_cast<float*>(h + Lp);           // [Lp + PITCH2_GUARD]
    (void)P;
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x;
    int64_t first, s0, nsamp;
    if (!pitch_frame_locate(bg, g, S, first, s0, nsamp)) return;
    float* cl = cl0 + Lp;
    // frame samples: lane owns elements lane + 64 r (r < 8, L <= 512)
    float xr[8];
    uint32_t kb[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int i = lane + 64 * r;
        float x = 0.f;
        const bool in = i < L;
        if (in && first + i < nsamp) x = sig[s0 + first + i];
        xr[r] = x;
        kb[r] = in ? pitch_clip_key(x) : 0xffffffffu;
    }
    for (int i = lane; i < Lp; i += 64) {
        cl0[i] = 0.f;                                      // guard band: samples before the frame
        if (i >= L) cl[i] = 0.f;
        h[i] = i < L ? taps[i] : make_float2(0.f, 0.f);
    }
    for (int i = lane; i < Lp + PITCH2_GUARD; i += 64) f[i] = 0.f;
    const float med = do_clip ? pitch_clip_level(kb) : 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int i = lane + 64 * r;
        if (i < L) {
            const float x = xr[r];
            cl[i] = do_clip ? pitch_center_clip(x, med) : x;
        }
    }
    __syncthreads();
    // ---- FIR: y[k] = sum_m h[m] c[k - m]; lane q owns outputs [W q, W q + W) and [Lp - W q - W, Lp - W q) ----
    const int nchunk = (Lp / W + 1) / 2;
    if (lane < nchunk) {
        const int kl = W * lane, kh = Lp - W * (lane + 1);
        float alr[W], ali[W], ahr[W], ahi[W];
        pitch_fir_pair<W>(cl, h, kl, kh, Lp, alr, ali, ahr, ahi);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            if (kl + e < L) f[kl + e] = sqrtf(fmaf(alr[e], alr[e], ali[e] * ali[e]));
            if (kh + e < L) f[kh + e] = sqrtf(fmaf(ahr[e], ahr[e], ahi[e] * ahi[e]));
        }
    }
    __syncthreads();
    // ---- autocorrelation: lane q owns lags lag_min + 4 q .. + 3; f is zero beyond L ----
    const int nq = (n_lags + 3) / 4;
    for (int q = lane; q < nq; q += 64) {
        const int n0 = lag_min + 4 * q;                    // multiple of 4
        float w[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 3; ++e) w[e] = f[n0 + e];      // positions n0 .. n0 + 2 in slots 0..2
        for (int i0 = 0; i0 < L; i0 += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + j;                      // window positions i + n0 .. i + n0 + 3
                w[(j + 3) % 4] = f[i + n0 + 3];
                const float a = i < L ? f[i] : 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(a, w[(j + e) % 4], acc[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = n0 + e;
            if (4 * q + e < n_lags) {
                float v;
                if (n == 0 || n < L) v = acc[e] / (float)(L - n);
                else v = __int_as_float(0x7fc00000);
                scores[g * n_lags + 4 * q + e] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The tracker behind the scores: pitch.smooth (pitch.py:157-164), pitch.max_pitch (pitch.py:166-172) and the two
// octave-repair sweeps of pitch.robust_max_pitch (pitch.py:191-206) for a whole batch, one wavefront per utterance.
// The pieces, and the habits of the reference they keep, are pitch_common.h's; here the two smoothed rows below row i
// are carried in registers and the raw rows come from global memory.  fp64 throughout, as the reference (its scores are
// this library's fp32 scores promoted to double).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pitch_track_kernel(const float* __restrict__ scores,
                                                         const int64_t* __restrict__ frame_off, int32_t n_lags,
                                                         int32_t bias, double* __restrict__ pitch) {
    __shared__ double s_pitch[PITCH_LDS_FRAMES];
    const int u = blockIdx.x, lane = threadIdx.x;
    const int64_t base = frame_off[u];
    const int T = (int)(frame_off[u + 1] - base);
    if (T <= 0) return;
    const float* sc = scores + base * n_lags;
    const PitchTrackStore<double> track{s_pitch, pitch + base};
    double p2[4], p1[4];                    // smoothed rows i - 2 and i - 1 (lags lane, lane + 64, ...)
#pragma unroll
    for (int k = 0; k < 4; ++k) p2[k] = p1[k] = 0.0;
    for (int i = 0; i < T; ++i) {
        int left, right;
        pitch_window_bounds(i, 2, T, left, right);
        double cur[4];
        double bv = -__longlong_as_double(0x7ff0000000000000ll);   // -inf, index "none": loses to every real candidate
        int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lag = lane + 64 * k;
            cur[k] = 0.0;
            if (lag < n_lags) {
                cur[k] = pitch_window_mean(left, right, [&](int r) {
                    return r == i - 2 ? p2[k] : (r == i - 1 ? p1[k] : (double)sc[(int64_t)r * n_lags + lag]);
                });
                pitch_argmax_combine(bv, bi, cur[k], lag);
            }
        }
        pitch_wave_argmax(bv, bi);
        if (lane == 0) track.put(i, pitch_hz(bias, bi));
#pragma unroll
        for (int k = 0; k < 4; ++k) { p2[k] = p1[k]; p1[k] = cur[k]; }
    }
    __syncthreads();
    if (lane == 0) pitch_octave_repair([&](int i) { return track.get(i); }, [&](int i, double v) { track.put(i, v); }, T);
    __syncthreads();
    track.flush(T, lane);
}

// ------------------------------------------------------------------------------------------------
// Device-side glue of the optional streams of model.py:90-101, so that ModelFeatureBatch never brings the trimmed
// clips to the host: decimation to 10 kHz (preprocess.downsampling, preprocess.py:21-28), frame offsets of a
// framing on the device, the [max_len, B, 2] pitch stream, and the tracker's parts for fp64 score rows.
// ------------------------------------------------------------------------------------------------

// preprocess.py:21-28 keeps sample i whenever  i * dst / src > kept - 1 + 1e-8  (Python: exact integer product, one
// fp64 division).  For a decimation (dst < src) the k-th kept index is the smallest i that passes the test for tick k.
__device__ __forceinline__ bool dsp_dec_pass(int64_t i, int64_t k, int64_t src, int64_t dst) {
    return (double)(i * dst) / (double)src > (double)(k - 1) + 1e-8;
}
__device__ __forceinline__ int64_t dsp_dec_index(int64_t k, int64_t src, int64_t dst) {
    int64_t i = (int64_t)floor(((double)(k - 1) + 1e-8) * (double)src / (double)dst);
    if (i < 0) i = 0;
    while (!dsp_dec_pass(i, k, src, dst)) ++i;
    while (i > 0 && dsp_dec_pass(i - 1, k, src, dst)) --i;
    return i;
}
__device__ __forceinline__ int64_t dsp_dec_count(int64_t n, int64_t src, int64_t dst) {   // samples kept of n
    if (n <= 0) return 0;
    int64_t k = (int64_t)floor((double)((n - 1) * dst) / (double)src) + 1;
    while (dsp_dec_index(k, src, dst) < n) ++k;
    while (k > 0 && dsp_dec_index(k - 1, src, dst) >= n) --k;
    return k;
}

// One 1024-thread block: lengths n_b = src_off[b+1] - src_off[b]  ->  (optional) decimated lengths and their exclusive
// prefix dst_off, and the exclusive prefix frame_off of the frame counts of the (decimated) lengths at (L, S)
// (sigproc.py:79-82).  dst_rate == 0: no decimation (frame offsets of another framing of the same clips).
__global__ __launch_bounds__(1024) void resample_layout_kernel(const int64_t* __restrict__ src_off, int32_t n_utt,
                                                               int64_t src_rate, int64_t dst_rate, int32_t L, int32_t S,
                                                               int64_t* __restrict__ dst_off, int64_t* __restrict__ frame_off) {
    __shared__ int64_t part_s[16], part_f[16];
    const int tid = threadIdx.x;
    const int per = (n_utt + 1023) / 1024;
    const int lo = tid * per, hi = min(lo + per, n_utt);
    int64_t sum_s = 0, sum_f = 0;
    for (int b = lo; b < hi; ++b) {
        int64_t n = src_off[b + 1] - src_off[b];
        if (dst_rate > 0) n = dsp_dec_count(n, src_rate, dst_rate);
        sum_s += n;
        sum_f += n <= L ? 1 : 1 + (n - L + S - 1) / S;
    }
    const int64_t in_s = dsp_wave_scan_i64(sum_s), in_f = dsp_wave_scan_i64(sum_f);
    if ((tid & 63) == 63) { part_s[tid >> 6] = in_s; part_f[tid >> 6] = in_f; }
    __syncthreads();
    int64_t base_s = in_s - sum_s, base_f = in_f - sum_f;
    for (int w = 0; w < (tid >> 6); ++w) { base_s += part_s[w]; base_f += part_f[w]; }
    for (int b = lo; b < hi; ++b) {
        int64_t n = src_off[b + 1] - src_off[b];
        if (dst_rate > 0) n = dsp_dec_count(n, src_rate, dst_rate);
        if (dst_off) dst_off[b] = base_s;
        frame_off[b] = base_f;
        base_s += n;
        base_f += n <= L ? 1 : 1 + (n - L + S - 1) / S;
    }
    if (hi == n_utt && lo < hi) {
        if (dst_off) dst_off[n_utt] = base_s;
        frame_off[n_utt] = base_f;
    }
    if (n_utt == 0 && tid == 0) { if (dst_off) dst_off[0] = 0; frame_off[0] = 0; }
}

// out[dst_off[b] + k] = in[src_off[b] + index of the k-th kept sample]  (preprocess.py:21-28), one thread per output
__global__ __launch_bounds__(256) void decimate_gather_kernel(const float* __restrict__ in, const int64_t* __restrict__ src_off,
                                                              const int64_t* __restrict__ dst_off, int32_t n_utt,
                                                              int64_t src_rate, int64_t dst_rate, float* __restrict__ out) {
    const int64_t total = dst_off[n_utt];
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = dsp_find_utt(dst_off, n_utt, o);
        out[o] = in[src_off[u] + dsp_dec_index(o - dst_off[u], src_rate, dst_rate)];
    }
}

// model.py:90-95: out[t, b, 0] = pitch[t] / 150, out[t, b, 1] = their first difference (T - 1 rows), zero padded /
// truncated to max_len rows (model.py:35-50).  One wave per utterance.
__global__ __launch_bounds__(64) void pitchfeat_finalize_kernel(const double* __restrict__ pitch,
                                                                const int64_t* __restrict__ frame_off, int32_t n_utt,
                                                                int32_t max_len, float* __restrict__ out, OutPlacement pl) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t base = frame_off[b];
    const int T = (int)(frame_off[b + 1] - base);
    const double* p = pitch + base;
    float* ob = pl.base(out, pl.col(b));
    const int64_t row = pl.stride();
    for (int t = lane; t < max_len; t += 64) {
        float z0 = 0.f, z1 = 0.f;
        if (t < T) {
            const double a = p[t] / 150.0;
            z0 = (float)a;
            if (t + 1 < T) z1 = (float)(p[t + 1] / 150.0 - a);
        }
        float* o = ob + (int64_t)t * row;
        o[0] = z0;
        o[1] = z1;
    }
}

// The tracker's parts on fp64 score rows (the host helpers pitch.smooth / max_pitch / robust_max_pitch are batches of
// one through this): flags bit 0 = smooth in place over rows [i - degree, i + degree) (pitch.py:157-164: the rows
// before i are already smoothed; the window's end is exclusive and stops at T - 1; an empty window is a NaN row),
// bit 1 = arg-max -> 1 / (1e-4 (bias + idx)) (pitch.py:166-172), bit 2 = the two octave-repair sweeps
// (pitch.py:191-206).  `rows` is overwritten by the smoothed rows when bit 0 is set.  One wave per utterance.
__global__ __launch_bounds__(64) void pitch_rows_kernel(double* __restrict__ rows, const int64_t* __restrict__ frame_off,
                                                        int32_t n_lags, int32_t bias, int32_t degree, int32_t flags,
                                                        double* __restrict__ pitch) {
    const int u = blockIdx.x, lane = threadIdx.x;
    const int64_t base = frame_off[u];
    const int T = (int)(frame_off[u + 1] - base);
    if (T <= 0) return;
    double* g = rows + base * n_lags;
    double* out = pitch ? pitch + base : nullptr;
    for (int i = 0; i < T; ++i) {
        double bv = -__longlong_as_double(0x7ff0000000000000ll);
        int bi = 0x7fffffff;
        for (int lag = lane; lag < n_lags; lag += 64) {
            double cur = g[(int64_t)i * n_lags + lag];
            if (flags & 1) {
                int left, right;
                pitch_window_bounds(i, degree, T, left, right);
                // rows below i are already smoothed: the same lane wrote them
                cur = pitch_window_mean(left, right, [&](int r) { return g[(int64_t)r * n_lags + lag]; });
                g[(int64_t)i * n_lags + lag] = cur;
            }
            pitch_argmax_combine(bv, bi, cur, lag);
        }
        if (flags & 2) {
            pitch_wave_argmax(bv, bi);
            if (lane == 0) out[i] = pitch_hz(bias, bi);
        }
    }
    if ((flags & 4) && lane == 0) pitch_octave_repair([&](int i) { return out[i]; }, [&](int i, double v) { out[i] = v; }, T);
}
