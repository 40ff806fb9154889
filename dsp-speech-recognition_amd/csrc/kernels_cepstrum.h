// Cepstral pitch path of the reference: pitch.pitch_detect (pitch.py:83-94) and pitch.pitch_feature (pitch.py:26-81,
// 227-279), batched.  Three launches behind the decimation to 10 kHz:
//   pitch_cepstrum_kernel        per frame: centre clip, complex band-pass FIR, FFT, log|.|, inverse FFT, |.|
//   pitch_cepstrum_track_kernel  per utterance: smoothing in place, peak-width scores, arg-max, octave repair
//   pitch_feature_kernel         per utterance: sub-endpoint, the two smooth subsequences, slopes, quadratic terms, shift
#pragma once

#include "pitch_common.h"

#define PITCH_CEP_MIN_I 20        // pitch.py:232: candidates 20 .. 99 on the 10 kHz quefrency grid
#define PITCH_CEP_NSCORE 80

// One wavefront per rectangular frame of L samples (L = 128 .. 1024, a power of two), zero padded as to_frames does.
//   1. centre clip at the median of the non-negative samples, non-binary form      pitch.py:145-155
//   2. y = convolve(clipped, taps)[:L], kept complex                                sigproc.py:22-46 as pitch.py:137 calls it
//   3. row = |IFFT_L(log|FFT_L(y)|)|                                                pitch.py:138-143
//   4. amp = sum |x| of the unclipped frame (fp64)                                  pitch.py:65
// Lane q owns W = L / 128 consecutive FIR outputs at the bottom of the frame and W at the top, so every lane does the
// same L + W tap products per output pair.  The transforms run in place in LDS on the buffer the clipped frame used:
// the forward pass leaves the spectrum bit-reversed, log|.| is pointwise, and the inverse pass takes bit-reversed
// input back to natural order, so nothing is ever permuted.  Only rows and amp reach global memory.
template <int L>
__global__ __launch_bounds__(64) void pitch_cepstrum_kernel(
    const float* __restrict__ sig, BatchGeom bg, int32_t S, const float2* __restrict__ taps, int32_t do_clip,
    float* __restrict__ rows, double* __restrict__ amp) {
    static_assert(L >= 128 && L <= 1024 && (L & (L - 1)) == 0, "frame length: a power of two in [128, 1024]");
    constexpr int W = L / 128, NR = L / 64;
    __shared__ __attribute__((aligned(16))) float s_cl0[2 * L];   // [L zeros][L samples]; later the L complex points
    __shared__ __attribute__((aligned(16))) float2 s_h[L];        // taps; later the L / 2 twiddles
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x;
    int64_t first, s0, nsamp;
    if (!pitch_frame_locate(bg, g, S, first, s0, nsamp)) return;
    float* cl = s_cl0 + L;
    // lane owns samples lane + 64 r
    float xr[NR];
    uint32_t kb[NR];
    double asum = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int i = lane + 64 * r;
        float x = 0.f;
        if (first + i < nsamp) x = sig[s0 + first + i];
        xr[r] = x;
        asum += (double)fabsf(x);
        kb[r] = pitch_clip_key(x);
        s_cl0[i] = 0.f;                                                  // guard band: samples before the frame
        s_h[i] = taps[i];
    }
    if (amp) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) asum += __shfl_xor(asum, o, 64);
        if (lane == 0) amp[g] = asum;
    }
    const float med = do_clip ? pitch_clip_level(kb) : 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const float x = xr[r];
        cl[lane + 64 * r] = do_clip ? pitch_center_clip(x, med) : x;
    }
    __syncthreads();
    // ---- FIR: y[k] = sum_m h[m] c[k - m]; lane q owns outputs [W q, W q + W) and [L - W q - W, L - W q) ----
    const int kl = W * lane, kh = L - W * (lane + 1);
    float alr[W], ali[W], ahr[W], ahi[W];
    pitch_fir_pair<W>(cl, s_h, kl, kh, L, alr, ali, ahr, ahi);
    __syncthreads();                                       // the clipped frame and the taps are dead from here
    float2* buf = reinterpret_cast<float2*>(s_cl0);        // [L] complex points
    float2* tw = s_h;                                      // [L / 2] exp(-2 pi i k / L)
#pragma unroll
    for (int e = 0; e < W; ++e) {
        buf[kl + e] = make_float2(alr[e], ali[e]);
        buf[kh + e] = make_float2(ahr[e], ahi[e]);
    }
    for (int k = lane; k < L / 2; k += 64) {
        float sn, cs;
        sincospif((float)(2 * k) / (float)L, &sn, &cs);
        tw[k] = make_float2(cs, -sn);
    }
    __syncthreads();
    pitch_fft_dif<L>(buf, tw, lane);
    for (int i = lane; i < L; i += 64) {                   // log|X|; a zero bin is -inf, as NumPy
        const float2 v = buf[i];
        buf[i] = make_float2(logf(sqrtf(fmaf(v.x, v.x, v.y * v.y))), 0.f);
    }
    __syncthreads();
    pitch_ifft_dit<L>(buf, tw, lane);
    float* out = rows + g * (int64_t)L;
    for (int i = lane; i < L; i += 64) {
        const float2 v = buf[i];
        out[i] = sqrtf(fmaf(v.x, v.x, v.y * v.y)) * (1.0f / (float)L);
    }
}

// The tracker behind the cepstrum rows, one wavefront per utterance, fp64, sequential over the frames:
//   flags bit 0  pitch.smooth(rows, 2); the smoothed rows below i are carried in registers, d_rows is not written
//                                                                                        pitch.py:157-164
//   always       pitch.peak_score of the (smoothed) row: for i in [20, 100) p walks down from i while p > 0 and
//                row[p] <= row[i], q walks up while q < L and row[q] <= row[i]; score = min(i - p, q - i).  row[0] is
//                never compared; a NaN row scores 0 everywhere.  i - p <= 99 and a walk up longer than the walk down
//                cannot change the minimum, so positions 1 .. 198 decide every score       pitch.py:227-242
//   flags bit 1  first arg-max of the 80 integers -> 1 / (1e-4 (20 + idx)), then the two octave-repair sweeps
//                                                                                        pitch.py:166-172,191-206
template <typename RT, int L>
__global__ __launch_bounds__(64) void pitch_cepstrum_track_kernel(const RT* __restrict__ rows,
                                                                  const int64_t* __restrict__ frame_off, int32_t flags,
                                                                  double* __restrict__ pitch, int32_t* __restrict__ scores) {
    constexpr int NR = L / 64;
    __shared__ double s_pitch[PITCH_LDS_FRAMES];
    const int u = blockIdx.x, lane = threadIdx.x;
    const int64_t base = frame_off[u];
    const int T = (int)(frame_off[u + 1] - base);
    if (T <= 0) return;
    const RT* rw = rows + base * L;
    const PitchTrackStore<double> track{s_pitch, (flags & 2) ? pitch + base : nullptr};
    double p2[NR], p1[NR];                  // smoothed rows i - 2 and i - 1 (columns lane, lane + 64, ...)
#pragma unroll
    for (int k = 0; k < NR; ++k) p2[k] = p1[k] = 0.0;
    // raw rows i and i + 1 live in registers and row i + 2 is fetched while frame i is scored: one batch of loads per
    // frame, off the critical path (a load per window row and column inside the sum costs a memory round trip each)
    double ra[NR], rb[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        ra[k] = (double)rw[lane + 64 * k];
        rb[k] = T > 1 ? (double)rw[(int64_t)L + lane + 64 * k] : 0.0;
    }
    for (int i = 0; i < T; ++i) {
        double cur[NR], rc[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) rc[k] = i + 2 < T ? (double)rw[(int64_t)(i + 2) * L + lane + 64 * k] : 0.0;
        if (flags & 1) {
            int left, right;                                      // right <= i + 2
            pitch_window_bounds(i, 2, T, left, right);
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                cur[k] = pitch_window_mean(left, right, [&](int r) {
                    return r == i - 2 ? p2[k] : (r == i - 1 ? p1[k] : (r == i ? ra[k] : rb[k]));
                });
            }
        } else {
#pragma unroll
            for (int k = 0; k < NR; ++k) cur[k] = ra[k];
        }
        // peak widths.  Only positions 1 .. 198 can matter (i <= 99, and a walk up longer than the walk down cannot change
        // the minimum), and lane l already holds positions l, l + 64, l + 128, l + 192 of the row in registers.  The
        // candidate is uniform: its value is read from its lane, one compare per register gives a 64-bit mask of the
        // positions that end a walk, and the nearest one either side is a count of leading / trailing zeros.  No LDS,
        // no barrier.  Positions at and beyond L end the walk up.
        constexpr int NW = NR < 4 ? NR : 4;
        int bv = -1, bi = 0, mine[2] = {0, 0};
#pragma unroll 4
        for (int c = 0; c < PITCH_CEP_NSCORE; ++c) {
            const int ii = PITCH_CEP_MIN_I + c, w = ii >> 6, bit = ii & 63;
            const double src = w == 0 ? cur[0] : cur[1];
            const double vi = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(src), bit),
                                               __builtin_amdgcn_readlane(__double2loint(src), bit));
            uint64_t m[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = k < NW ? __ballot(!(cur[k < NW ? k : 0] <= vi)) : ~0ull;
            const uint64_t below = (1ull << bit) - 1;                           // positions of word w below the candidate
            const uint64_t l0 = (w == 0 ? m[0] & below : m[0]) & ~1ull;            // position 0 is never compared
            const uint64_t l1 = w == 0 ? 0ull : m[1] & below;
            const int p = l1 ? 127 - __builtin_clzll(l1) : (l0 ? 63 - __builtin_clzll(l0) : 0);
            const int dl = !(vi <= vi) ? 0 : ii - p;
            const uint64_t above = bit == 63 ? 0ull : ~0ull << (bit + 1);
            const uint64_t r0 = (w == 0 ? m[0] : m[1]) & above, r1 = w == 0 ? m[1] : m[2], r2 = w == 0 ? m[2] : m[3];
            const int q = r0 ? 64 * w + __builtin_ctzll(r0)
                             : (r1 ? 64 * (w + 1) + __builtin_ctzll(r1) : (r2 ? 64 * (w + 2) + __builtin_ctzll(r2) : ii + 129));
            const int sc = min(dl, q - ii);
            if (lane == (c & 63)) mine[c >> 6] = sc;
            if (sc > bv) { bv = sc; bi = c; }                      // c ascends: the first maximum stays
        }
        if (scores) {
            scores[(base + i) * PITCH_CEP_NSCORE + lane] = mine[0];
            if (lane + 64 < PITCH_CEP_NSCORE) scores[(base + i) * PITCH_CEP_NSCORE + 64 + lane] = mine[1];
        }
        if ((flags & 2) && lane == 0) track.put(i, pitch_hz(PITCH_CEP_MIN_I, bi));
#pragma unroll
        for (int k = 0; k < NR; ++k) { p2[k] = p1[k]; p1[k] = cur[k]; ra[k] = rb[k]; rb[k] = rc[k]; }
    }
    if (!(flags & 2)) return;
    if (lane == 0) pitch_octave_repair([&](int i) { return track.get(i); }, [&](int i, double v) { track.put(i, v); }, T);
    __syncthreads();
    track.flush(T, lane);
}

// ------------------------------------------------------------------------------------------------
// pitch.find_smooth_subsequence (pitch.py:245-279): from every start i collect the values that stay within `thres` of
// the last accepted one, until `tor` values were rejected (the segment is then (i, j), j the index of the last
// rejection, and the next start is j - tor + 1) or the sequence ends (segment (i, n), the search stops).  Returned is
// the longest collected segment, the first one on a tie.  A comparison against a NaN accepts, as in the reference.
// ------------------------------------------------------------------------------------------------
struct PitchSubseq {
    int start, end, count;
};

template <typename Get>
__device__ __forceinline__ PitchSubseq pitch_subseq_best(Get get, int n, int tor, double thres) {
    PitchSubseq best = {0, 0, 0};
    int i = 0;
    while (i < n) {
        int j = i + 1, k = tor, cnt = 1;
        double prev = get(i);
        while (j < n) {
            const double v = get(j);
            if (fabs(v - prev) > thres) --k; else { ++cnt; prev = v; }
            if (!k) break;
            ++j;
        }
        if (cnt > best.count) best = {i, j, cnt};
        if (j == n) break;
        i = j - tor + 1;
    }
    return best;
}

// the accepted values of the segment that starts at s.start, in order, handed to put(idx, value)
template <typename Get, typename Put>
__device__ __forceinline__ void pitch_subseq_collect(Get get, PitchSubseq s, double thres, Put put) {
    if (s.count <= 0) return;
    double prev = get(s.start);
    int idx = 0;
    put(idx++, prev);
    for (int j = s.start + 1; j < s.end && idx < s.count; ++j) {
        const double v = get(j);
        if (!(fabs(v - prev) > thres)) { put(idx++, v); prev = v; }
    }
}

// values [sum n_b] fp64 -> accepted values at seg[off[b] ..], info[b] = (start, end, count).  One wave per sequence; the
// search is one dependency chain, so lane 0 walks it.
__global__ __launch_bounds__(64) void pitch_subseq_kernel(const double* __restrict__ values, const int64_t* __restrict__ off,
                                                          int32_t tor, double thres, double* __restrict__ seg,
                                                          int32_t* __restrict__ info) {
    if (threadIdx.x != 0) return;
    const int u = blockIdx.x;
    const int64_t base = off[u];
    const int n = (int)(off[u + 1] - base);
    const double* v = values + base;
    auto get = [&](int i) { return v[i]; };
    const PitchSubseq s = pitch_subseq_best(get, n, tor, thres);
    pitch_subseq_collect(get, s, thres, [&](int idx, double x) { seg[base + idx] = x; });
    info[3 * u + 0] = s.start;
    info[3 * u + 1] = s.end;
    info[3 * u + 2] = s.count;
}

// Median of m values (m >= 1, none NaN) by rank counting across the wave: the k-th order statistic is the value with
// at most k values below it and more than k values not above it.  numpy.median: mean of the two middle ones.
__device__ __forceinline__ double pitch_wave_median(const double* __restrict__ v, int m, double* s_two) {
    const int lane = threadIdx.x, k1 = (m - 1) >> 1, k2 = m >> 1;
    for (int e = lane; e < m; e += 64) {
        const double x = v[e];
        int lt = 0, eq = 0;
        for (int r = 0; r < m; ++r) {
            const double y = v[r];
            lt += y < x ? 1 : 0;
            eq += y == x ? 1 : 0;
        }
        if (lt <= k1 && k1 < lt + eq) s_two[0] = x;
        if (lt <= k2 && k2 < lt + eq) s_two[1] = x;
    }
    __syncthreads();
    const double r = (s_two[0] + s_two[1]) / 2.0;
    __syncthreads();
    return r;
}

// The tail of pitch.pitch_feature (pitch.py:26-81), one wavefront per utterance, fp64:
//   p      = sub_endpoint_detect: among i in [10, T - 10) with no amp[i-2 .. i+2] below amp[i], the first i with the
//            largest sum_{j = i-10 .. i+10} (amp[j] - amp[i]) (strictly greater, from -1000); none: T // 2   pitch.py:64-81
//   p_bias = 5 if p > 15 else 0                                                                              pitch.py:36
//   seg1, seg2 = find_smooth_subsequence(pitch[p_bias:p]), (pitch[p:]), tor 3, thres 30                      pitch.py:39-40
//   feat   = slope(seg1), slope(seg2), quad(seg1), quad(seg2), median(seg2) - median(seg1)                   pitch.py:44-62
// The least-squares leading coefficients over x = 0 .. m - 1 use the centred orthogonal basis: sum (x - xm) y /
// sum (x - xm)^2 and sum q y / sum q^2 with q = (x - xm)^2 - (m^2 - 1) / 12.  The reference raises for an empty slice
// and for m < 2, and is rank deficient for m = 2 at degree 2: any segment with m < 3 gives valid = 0 and a NaN row.
// aux[b] = (p, p_bias, start1, end1, start2, end2, m1, m2, valid), indices counted from the utterance's first frame.
// seg receives the accepted values: seg1 at seg[base + p_bias ..], seg2 at seg[base + p ..].  pitch == NULL: only p.
__global__ __launch_bounds__(64) void pitch_feature_kernel(const double* __restrict__ pitch, const double* __restrict__ amp,
                                                           const int64_t* __restrict__ frame_off, double* __restrict__ seg,
                                                           double* __restrict__ feat, int32_t* __restrict__ aux) {
    __shared__ double s_pitch[PITCH_LDS_FRAMES];
    __shared__ double s_fit[4], s_two[2];
    __shared__ int s_seg[6];
    const int u = blockIdx.x, lane = threadIdx.x;
    const int64_t base = frame_off[u];
    const int T = (int)(frame_off[u + 1] - base);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double* a = amp + base;
    double bs = -1000.0;
    int bi = 0x7fffffff;
    for (int i = 10 + lane; i < T - 10; i += 64) {
        const double ai = a[i];
        bool low = true;
#pragma unroll
        for (int d = -2; d <= 2; ++d) low = low && !(a[i + d] < ai);
        if (!low) continue;
        double s = 0.0;
        for (int j = i - 10; j <= i + 10; ++j) s += a[j] - ai;     // in order, as Python's sum
        if (s > bs) { bs = s; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(bs, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
    }
    const int p = bi == 0x7fffffff ? (T > 0 ? T / 2 : 0) : bi;
    int32_t* ax = aux + 9 * (int64_t)u;
    if (!pitch) {
        if (lane == 0) ax[0] = p;
        return;
    }
    const int p_bias = p > 15 ? 5 : 0;
    const PitchTrackStore<const double> track{s_pitch, pitch + base};
    track.load(T, lane);
    __syncthreads();
    if (lane == 0) {
        for (int h = 0; h < 2; ++h) {
            const int lo = h == 0 ? p_bias : p, n = h == 0 ? p - p_bias : T - p;
            auto get = [&](int i) { return track.get(lo + i); };
            const PitchSubseq s = pitch_subseq_best(get, n > 0 ? n : 0, 3, 30.0);
            const int m = s.count;
            const double xm = 0.5 * (double)(m - 1), c2 = ((double)m * (double)m - 1.0) / 12.0;
            double n1 = 0.0, d1 = 0.0, n2 = 0.0, d2 = 0.0;
            pitch_subseq_collect(get, s, 30.0, [&](int idx, double y) {
                seg[base + lo + idx] = y;
                const double x = (double)idx - xm, q = x * x - c2;
                n1 += x * y; d1 += x * x;
                n2 += q * y; d2 += q * q;
            });
            s_fit[h] = m >= 3 ? n1 / d1 : qnan;
            s_fit[2 + h] = m >= 3 ? n2 / d2 : qnan;
            s_seg[3 * h + 0] = lo + s.start;
            s_seg[3 * h + 1] = lo + s.end;
            s_seg[3 * h + 2] = m;
        }
    }
    __syncthreads();                                               // seg[] written by lane 0 is read by the whole wave below
    const int m1 = s_seg[2], m2 = s_seg[5];
    const bool valid = m1 >= 3 && m2 >= 3;
    double shift = qnan;
    if (valid) {
        const double med1 = pitch_wave_median(seg + base + p_bias, m1, s_two);
        const double med2 = pitch_wave_median(seg + base + p, m2, s_two);
        shift = med2 - med1;
    }
    if (lane == 0) {
        double* f = feat + 5 * (int64_t)u;
        f[0] = valid ? s_fit[0] : qnan;
        f[1] = valid ? s_fit[1] : qnan;
        f[2] = valid ? s_fit[2] : qnan;
        f[3] = valid ? s_fit[3] : qnan;
        f[4] = shift;
        ax[0] = p; ax[1] = p_bias;
        ax[2] = s_seg[0]; ax[3] = s_seg[1]; ax[4] = s_seg[3]; ax[5] = s_seg[4];
        ax[6] = m1; ax[7] = m2; ax[8] = valid ? 1 : 0;
    }
}
