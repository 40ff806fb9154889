// Generic (table-driven, any supported NFFT / L / S / M / C) kernels of the feature path.
// One wavefront owns one frame: frame samples -> LDS, mixed-radix Stockham FFT of NFFT/2 complex
// points in LDS (radices 4/2 plus one optional 3 for NFFT = 3*2^k, e.g. model.py:74's 1536),
// real-spectrum untangle, |X|^2/NFFT, CSR mel triangles, log, DCT*lifter, energy swap.
// This is the correctness workhorse and the fallback for every configuration the specialised
// NFFT=512 kernel (kernels_fast512.h) does not cover.
//
// The transform is a template parameter (ROUTE, dsp_plan_transform reports it); everything behind the spectrum is shared:
//   0  the pass list of the 17 sizes 2^k and 3*2^k, radices 4 / 2 / 3: this instantiation is the one the parent had
//   1  any even NFFT whose half is 2^a 3^b 5^c: the same packed transform with radix-5 passes and any number of 3s
//   2  every other NFFT (odd, or a prime factor above 5 in its half): chirp-z (Bluestein), see chirp_spectrum below
#pragma once

#include "dsp_common.h"
#include "kernels_repair.h"

#define DSP_GEN_WAVES 4
#define DSP_MAX_RADIX_PASSES 12

struct GenericParams {
    int32_t L, S, nfft, K, M, C, lfft, append_energy;
    float preemph;
    const float* window;
    const float2* tw;  // [nfft] exp(-2 pi i k / nfft)
    const int32_t* mel_start;
    const int32_t* mel_count;
    const int32_t* mel_off;
    const float* mel_w;
    const float* dct;
    const DspRepairTab* repair;  // fp64 tables for cancelled mel filters (kernels_repair.h)
    int32_t n_pass;
    int32_t radix[DSP_MAX_RADIX_PASSES];   // route 2: the passes of the convolution transform of conv_len points
    // the chirp-z route only (NULL / 0 otherwise)
    int32_t conv_len;        // 2^k or 3*2^k >= lfft + K - 1
    const float2* cz_w;      // [nfft]      w[n] = exp(-i pi n^2 / nfft)
    const float2* cz_spec;   // [conv_len]  transform of conj(w) laid out circularly, in the order dif_pass leaves it, / conv_len
    const float2* cz_tw;     // [conv_len]  exp(-2 pi i k / conv_len)
};

// One Stockham pass of radix R over n complex points held in LDS (in -> out), executed by one wave.
// p = product of the radices of the previous passes.  Thread j handles inputs j + r*n/R.
template <int R>
__device__ __forceinline__ void stockham_pass(const float2* __restrict__ in, float2* __restrict__ out, int n,
                                              int p, int lane, const float2* __restrict__ tw, int nfft) {
    const int T = n / R;
    const int twstep = nfft / (p * R);  // exp(-2 pi i r k /(p R)) = tw[r * k * twstep]
    for (int j = lane; j < T; j += 64) {
        const int k = j % p;
        float2 u[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float2 v = in[j + r * T];
            if (r > 0 && k > 0) v = cmul(v, tw[r * k * twstep]);
            u[r] = v;
        }
        const int j0 = (j - k) * R + k;
        if constexpr (R == 2) {
            out[j0] = make_float2(u[0].x + u[1].x, u[0].y + u[1].y);
            out[j0 + p] = make_float2(u[0].x - u[1].x, u[0].y - u[1].y);
        } else if constexpr (R == 3) {
            const float h = 0.86602540378443864676f;  // sqrt(3)/2
            float2 t1 = make_float2(u[1].x + u[2].x, u[1].y + u[2].y);
            float2 t2 = make_float2(fmaf(-0.5f, t1.x, u[0].x), fmaf(-0.5f, t1.y, u[0].y));
            float2 t3 = make_float2(h * (u[1].x - u[2].x), h * (u[1].y - u[2].y));
            out[j0] = make_float2(u[0].x + t1.x, u[0].y + t1.y);
            out[j0 + p] = make_float2(t2.x + t3.y, t2.y - t3.x);
            out[j0 + 2 * p] = make_float2(t2.x - t3.y, t2.y + t3.x);
        } else if constexpr (R == 4) {  // forward: W4 = -i
            float2 a = make_float2(u[0].x + u[2].x, u[0].y + u[2].y);
            float2 b = make_float2(u[0].x - u[2].x, u[0].y - u[2].y);
            float2 c = make_float2(u[1].x + u[3].x, u[1].y + u[3].y);
            float2 d = make_float2(u[1].x - u[3].x, u[1].y - u[3].y);
            out[j0] = make_float2(a.x + c.x, a.y + c.y);
            out[j0 + p] = make_float2(b.x + d.y, b.y - d.x);      // b - i d
            out[j0 + 2 * p] = make_float2(a.x - c.x, a.y - c.y);
            out[j0 + 3 * p] = make_float2(b.x - d.y, b.y + d.x);  // b + i d
        } else {  // R == 5 (route 1 only)
            static_assert(R == 5, "radices 2, 3, 4, 5");
            const float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;   // cos(2 pi / 5), cos(4 pi / 5)
            const float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;    // sin(2 pi / 5), sin(4 pi / 5)
            float2 a1 = make_float2(u[1].x + u[4].x, u[1].y + u[4].y), b1 = make_float2(u[1].x - u[4].x, u[1].y - u[4].y);
            float2 a2 = make_float2(u[2].x + u[3].x, u[2].y + u[3].y), b2 = make_float2(u[2].x - u[3].x, u[2].y - u[3].y);
            float2 m1 = make_float2(fmaf(c1, a1.x, fmaf(c2, a2.x, u[0].x)), fmaf(c1, a1.y, fmaf(c2, a2.y, u[0].y)));
            float2 m2 = make_float2(fmaf(c2, a1.x, fmaf(c1, a2.x, u[0].x)), fmaf(c2, a1.y, fmaf(c1, a2.y, u[0].y)));
            float2 n1 = make_float2(fmaf(s1, b1.x, s2 * b2.x), fmaf(s1, b1.y, s2 * b2.y));
            float2 n2 = make_float2(fmaf(s2, b1.x, -s1 * b2.x), fmaf(s2, b1.y, -s1 * b2.y));
            out[j0] = make_float2(u[0].x + a1.x + a2.x, u[0].y + a1.y + a2.y);
            out[j0 + p] = make_float2(m1.x + n1.y, m1.y - n1.x);      // m1 - i n1
            out[j0 + 2 * p] = make_float2(m2.x + n2.y, m2.y - n2.x);  // m2 - i n2
            out[j0 + 3 * p] = make_float2(m2.x - n2.y, m2.y + n2.x);  // m2 + i n2
            out[j0 + 4 * p] = make_float2(m1.x - n1.y, m1.y + n1.x);  // m1 + i n1
        }
    }
}

// ---- the chirp-z route: in-place passes over n complex points of one wave's LDS buffer ----
// X[k] = w[k] sum_n (x[n] w[n]) conj(w)[k - n]: a circular convolution of conv_len >= lfft + K - 1 points, done as a forward
// transform, a pointwise product with the stored transform of conj(w), and an inverse transform.  The forward passes are
// decimation in frequency (natural order in, digit-reversed out), the inverse passes their conjugate transposes in the
// opposite order (digit-reversed in, natural out), so nothing is permuted and one buffer serves; the stored spectrum lies in
// the order the forward passes leave theirs (the host runs the same passes in fp64 to build it).

// R-point DFT of u[] in place; INV: conjugate roots
template <int R, bool INV>
__device__ __forceinline__ void cz_butterfly(float2 (&u)[R]) {
    if constexpr (R == 2) {
        const float2 a = u[0], b = u[1];
        u[0] = make_float2(a.x + b.x, a.y + b.y);
        u[1] = make_float2(a.x - b.x, a.y - b.y);
    } else if constexpr (R == 3) {
        const float h = INV ? -0.86602540378443864676f : 0.86602540378443864676f;
        const float2 t1 = make_float2(u[1].x + u[2].x, u[1].y + u[2].y);
        const float2 t2 = make_float2(fmaf(-0.5f, t1.x, u[0].x), fmaf(-0.5f, t1.y, u[0].y));
        const float2 t3 = make_float2(h * (u[1].x - u[2].x), h * (u[1].y - u[2].y));
        u[0] = make_float2(u[0].x + t1.x, u[0].y + t1.y);
        u[1] = make_float2(t2.x + t3.y, t2.y - t3.x);
        u[2] = make_float2(t2.x - t3.y, t2.y + t3.x);
    } else {
        static_assert(R == 4, "radices 2, 3, 4");
        const float2 a = make_float2(u[0].x + u[2].x, u[0].y + u[2].y), b = make_float2(u[0].x - u[2].x, u[0].y - u[2].y);
        const float2 c = make_float2(u[1].x + u[3].x, u[1].y + u[3].y);
        float2 d = make_float2(u[1].x - u[3].x, u[1].y - u[3].y);
        if (INV) d = make_float2(-d.x, -d.y);
        u[0] = make_float2(a.x + c.x, a.y + c.y);
        u[1] = make_float2(b.x + d.y, b.y - d.x);
        u[2] = make_float2(a.x - c.x, a.y - c.y);
        u[3] = make_float2(b.x - d.y, b.y + d.x);
    }
}

// forward pass of radix R over blocks of `blk` points (blk = n, n / R0, ... down the pass list): butterfly over the R points
// j + q blk / R of a block, then output q times exp(-2 pi i j q / blk).  A butterfly reads and writes its own R points only.
template <int R>
__device__ __forceinline__ void dif_pass(float2* __restrict__ buf, int n, int blk, int lane, const float2* __restrict__ tw) {
    const int sub = blk / R, twstep = n / blk;
    for (int b = lane; b < n / R; b += 64) {
        const int j = b % sub, base = (b - j) * R + j;
        float2 u[R];
#pragma unroll
        for (int q = 0; q < R; ++q) u[q] = buf[base + q * sub];
        cz_butterfly<R, false>(u);
        buf[base] = u[0];
#pragma unroll
        for (int q = 1; q < R; ++q) buf[base + q * sub] = j ? cmul(u[q], tw[j * q * twstep]) : u[q];
    }
}

// its conjugate transpose (an inverse pass, not scaled): conjugate twiddles first, then the conjugate butterfly
template <int R>
__device__ __forceinline__ void dit_pass(float2* __restrict__ buf, int n, int blk, int lane, const float2* __restrict__ tw) {
    const int sub = blk / R, twstep = n / blk;
    for (int b = lane; b < n / R; b += 64) {
        const int j = b % sub, base = (b - j) * R + j;
        float2 u[R];
        u[0] = buf[base];
#pragma unroll
        for (int q = 1; q < R; ++q) {
            float2 v = buf[base + q * sub];
            if (j) {
                const float2 w = tw[j * q * twstep];
                v = cmul(v, make_float2(w.x, -w.y));
            }
            u[q] = v;
        }
        cz_butterfly<R, true>(u);
#pragma unroll
        for (int q = 0; q < R; ++q) buf[base + q * sub] = u[q];
    }
}

// buf[0 .. conv_len) holds x[n] w[n] (zeros from lfft on) -> buf[k] = sum_n x[n] w[n] conj(w)[k - n], k < K
__device__ __forceinline__ void chirp_spectrum(float2* __restrict__ buf, const GenericParams& P, int lane) {
    const int n = P.conv_len;
    int blk = n;
    for (int s = 0; s < P.n_pass; ++s) {
        const int R = P.radix[s];
        if (R == 4) dif_pass<4>(buf, n, blk, lane, P.cz_tw);
        else if (R == 2) dif_pass<2>(buf, n, blk, lane, P.cz_tw);
        else dif_pass<3>(buf, n, blk, lane, P.cz_tw);
        blk /= R;
        __syncthreads();
    }
    for (int i = lane; i < n; i += 64) buf[i] = cmul(buf[i], P.cz_spec[i]);
    __syncthreads();
    for (int s = P.n_pass - 1; s >= 0; --s) {
        const int R = P.radix[s];
        blk *= R;
        if (R == 4) dit_pass<4>(buf, n, blk, lane, P.cz_tw);
        else if (R == 2) dit_pass<2>(buf, n, blk, lane, P.cz_tw);
        else dit_pass<3>(buf, n, blk, lane, P.cz_tw);
        __syncthreads();
    }
}

// LDS of one wave's frame on the chirp-z route, in float2 units: the convolution buffer and K floats of power spectrum
__host__ __device__ __forceinline__ int dsp_chirp_frame_lds(int conv_len, int K) { return conv_len + (K + 1) / 2; }

template <int DTYPE, int ROUTE = 0>
__global__ __launch_bounds__(64 * DSP_GEN_WAVES) void features_generic_kernel(
    GenericParams P, BatchGeom bg, const void* __restrict__ wave, int out_kind, float* __restrict__ out,
    int64_t ld_out, float* __restrict__ out2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int N2 = P.nfft >> 1;
    // routes 0 and 1: two buffers of NFFT / 2 points per wave; route 2: one of conv_len points and the power spectrum behind it
    float2* bufA = reinterpret_cast<float2*>(smem) + (ROUTE == 2 ? (size_t)wid * dsp_chirp_frame_lds(P.conv_len, N2 + 1) : (size_t)wid * 2 * N2);
    float2* bufB = bufA + (ROUTE == 2 ? P.conv_len : N2);
    const float repair_thr = dsp_repair_threshold(N2 + 1);   // by the plan's bin count (kernels_repair.h)
    // frames of a workgroup: route 2 launches as many waves as its LDS allows (1 .. DSP_GEN_WAVES)
    const int waves = ROUTE == 2 ? (int)(blockDim.x >> 6) : DSP_GEN_WAVES;

    // ragged batches: bg.total_frames may be an upper bound (device-built layouts), the table holds the truth
    const int64_t total_frames = bg.uniform_frames > 0 ? bg.total_frames : bg.frame_off[bg.n_utt];   // the table is read for ragged geometry only
    const int64_t n_tiles = (total_frames + waves - 1) / waves;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int64_t g = tile * waves + wid;
        const bool active = g < total_frames;
        if (!active) g = total_frames - 1;  // keep the wave in step with the barriers
        int32_t utt;
        int64_t t, s0, nsamp;
        dsp_locate(bg, g, utt, t, s0, nsamp);
        const int64_t first = t * (int64_t)P.S;

        // ---- pre-emphasis + framing + window (sigproc.py:66-98,178-185) ----
        float* fr = reinterpret_cast<float*>(bufA);
        for (int n = lane; n < P.L; n += 64) {
            const int64_t pos = first + n;
            float v = 0.f;
            if (pos < nsamp) {
                v = dsp_load_sample<DTYPE>(wave, s0 + pos);
                if (P.preemph != 0.f && pos > 0)
                    v = fmaf(-P.preemph, dsp_load_sample<DTYPE>(wave, s0 + pos - 1), v);
            }
            v *= P.window[n];
            if (out_kind == DSP_OUT_FRAMES) {
                if (active) out[g * ld_out + n] = v;
            } else if (n < P.lfft) {
                if constexpr (ROUTE == 2) {
                    const float2 w = P.cz_w[n];
                    bufA[n] = make_float2(v * w.x, v * w.y);
                } else {
                    fr[n] = v;
                }
            }
        }
        if (out_kind == DSP_OUT_FRAMES) continue;  // uniform over the block
        if constexpr (ROUTE == 2) {
            for (int n = P.lfft + lane; n < P.conv_len; n += 64) bufA[n] = make_float2(0.f, 0.f);
        } else {
            for (int n = P.lfft + lane; n < P.nfft; n += 64) fr[n] = 0.f;
        }
        __syncthreads();

        float2* src = bufA;
        float2* dst = bufB;
        if constexpr (ROUTE == 2) {
            // ---- chirp-z: src[k] w[k] = X[k], k <= NFFT/2 ----
            chirp_spectrum(bufA, P, lane);
        } else {
            // ---- complex FFT of z[m] = x[2m] + i x[2m+1], m < NFFT/2 ----
            int p = 1;
            for (int s = 0; s < P.n_pass; ++s) {
                const int R = P.radix[s];
                if (R == 4) stockham_pass<4>(src, dst, N2, p, lane, P.tw, P.nfft);
                else if (R == 2) stockham_pass<2>(src, dst, N2, p, lane, P.tw, P.nfft);
                else if (ROUTE == 0 || R == 3) stockham_pass<3>(src, dst, N2, p, lane, P.tw, P.nfft);
                else stockham_pass<5>(src, dst, N2, p, lane, P.tw, P.nfft);
                p *= R;
                float2* tmp = src; src = dst; dst = tmp;
                __syncthreads();
            }
        }
        // ---- untangle to the real-input spectrum, |X|^2 / NFFT (sigproc.py:136-158) ----
        float* pspec = reinterpret_cast<float*>(dst);  // K = N2 + 1 <= 2*N2 floats
        const float inv_nfft = 1.0f / (float)P.nfft;
        float esum = 0.f;
        for (int k = lane; k <= N2; k += 64) {
            float2 x;
            if constexpr (ROUTE == 2) {
                x = cmul(src[k], P.cz_w[k]);
            } else {
                const float2 zk = src[k == N2 ? 0 : k];
                const float2 zc = src[k == 0 ? 0 : N2 - k];
                const float2 e = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));
                const float2 o = make_float2(0.5f * (zk.y + zc.y), -0.5f * (zk.x - zc.x));
                const float2 w = P.tw[k];
                x = make_float2(e.x + fmaf(w.x, o.x, -w.y * o.y), e.y + fmaf(w.x, o.y, w.y * o.x));
            }
            const float m2 = fmaf(x.x, x.x, x.y * x.y);
            if (out_kind == DSP_OUT_MAGSPEC) {
                if (active) out[g * ld_out + k] = sqrtf(m2);
            } else {
                const float pw = m2 * inv_nfft;
                if (out_kind == DSP_OUT_POWSPEC) {
                    if (active) out[g * ld_out + k] = pw;
                } else {
                    pspec[k] = pw;
                    esum += pw;
                }
            }
        }
        if (out_kind == DSP_OUT_MAGSPEC || out_kind == DSP_OUT_POWSPEC) {
            __syncthreads();
            continue;
        }
        esum = dsp_wave_sum(esum);
        if (esum == 0.f) esum = DSP_EPS_F32;  // base.py:26
        __syncthreads();

        // ---- mel filterbank (base.py:28-30), log (base.py:12) ----
        float* logmel = reinterpret_cast<float*>(src);  // spectrum Z is dead now
        for (int j0 = 0; j0 < P.M; j0 += 64) {
            const int j = j0 + lane;
            float acc = 0.f;
            if (j < P.M) {
                const int b0 = P.mel_start[j], cnt = P.mel_count[j];
                const float* w = P.mel_w + P.mel_off[j];
                for (int i = 0; i < cnt; ++i) acc = fmaf(w[i], pspec[b0 + i], acc);
            }
            float lg = logf(acc == 0.f ? DSP_EPS_F32 : acc);  // base.py:30
            if (out_kind == DSP_OUT_MFCC) {
                // a filter the fp32 spectrum cannot carry: its bins again in fp64 (kernels_repair.h); rare and wave-uniform
                unsigned long long m = __ballot(j < P.M && acc > 0.f && acc < repair_thr * esum);
                while (m != 0) {
                    const int src_lane = __builtin_ctzll(m);
                    m &= m - 1;
                    const double a = dsp_repair_mel_f64<DTYPE>(P.repair, wave, s0, nsamp, first, j0 + src_lane, lane);
                    if (lane == src_lane) lg = (float)log(a == 0.0 ? (double)DSP_EPS_F32 : a);
                }
            }
            if (j < P.M) {
                if (out_kind == DSP_OUT_FBANK) {
                    if (acc == 0.f) acc = DSP_EPS_F32;
                    if (active) out[g * ld_out + j] = acc;
                } else {
                    logmel[j] = lg;
                }
            }
        }
        if (out_kind == DSP_OUT_FBANK) {
            if (active && lane == 0) out2[g] = esum;
            __syncthreads();
            continue;
        }
        __syncthreads();
        // ---- DCT-II (ortho) * lifter, first C outputs; energy swap (base.py:13-15) ----
        for (int c = lane; c < P.C; c += 64) {
            const float* d = P.dct + (size_t)c * P.M;
            float acc = 0.f;
            for (int j = 0; j < P.M; ++j) acc = fmaf(d[j], logmel[j], acc);
            if (c == 0 && P.append_energy) acc = logf(esum);
            if (active) out[g * ld_out + c] = acc;
        }
        __syncthreads();
    }
}

// base.delta (base.py:70-79) and, optionally, delta-of-delta in the same pass.
__global__ __launch_bounds__(256) void delta_kernel(const float* __restrict__ in, int64_t ld_in, BatchGeom bg,
                                                    int32_t D, int32_t N, float inv_den, float* __restrict__ out,
                                                    int64_t ld_out, float* __restrict__ out_dd, int64_t ld_dd) {
    const int64_t total = (bg.uniform_frames > 0 ? bg.total_frames : bg.frame_off[bg.n_utt]) * D;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = idx / D;
        const int32_t d = (int32_t)(idx - g * D);
        int64_t t, T, base;
        if (bg.uniform_frames > 0) {
            const int64_t u = g / bg.uniform_frames;
            base = u * bg.uniform_frames;
            T = bg.uniform_frames;
        } else {
            const int32_t u = dsp_find_utt(bg.frame_off, bg.n_utt, g);
            base = bg.frame_off[u];
            T = bg.frame_off[u + 1] - base;
        }
        t = g - base;
        auto x = [&](int64_t tt) -> float {
            tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
            return in[(base + tt) * ld_in + d];
        };
        auto d1 = [&](int64_t tt) -> float {
            tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);  // edge-replicated Delta for the second pass
            float acc = 0.f;
            for (int n = 1; n <= N; ++n) acc = fmaf((float)n, x(tt + n) - x(tt - n), acc);
            return acc * inv_den;
        };
        out[g * ld_out + d] = d1(t);
        if (out_dd != nullptr) {
            float acc = 0.f;
            for (int n = 1; n <= N; ++n) acc = fmaf((float)n, d1(t + n) - d1(t - n), acc);
            out_dd[g * ld_dd + d] = acc * inv_den;
        }
    }
}

// Tiled delta + delta-delta: one workgroup owns DT_TILE consecutive frames of one utterance.
// The tile's rows (plus a halo of 2N, edge-replicated at the utterance ends exactly like
// numpy.pad(mode='edge') in base.py:75) go to LDS once; delta is formed in LDS for tile + halo N,
// delta-delta from that, so every input value is read from HBM/L2 once instead of (2N+1)^2 times.
#ifndef DT_TILE
#define DT_TILE 128
#define DT_SHIFT 7
#endif
// tile_off[b] = sum_{i<b} ceil(T_i / 2^shift), tile_off[n] = total (single block).
__global__ __launch_bounds__(1024) void prefix_ceil_kernel(const int64_t* __restrict__ frame_off, int32_t n_utt,
                                                           int shift, int64_t* __restrict__ tile_off) {
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    const int per = (n_utt + 1023) / 1024;
    const int lo = tid * per, hi = min(lo + per, n_utt);
    const int64_t rnd = ((int64_t)1 << shift) - 1;
    int64_t sum = 0;
    for (int b = lo; b < hi; ++b) sum += (frame_off[b + 1] - frame_off[b] + rnd) >> shift;
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = part[tid] - sum;
    for (int b = lo; b < hi; ++b) {
        tile_off[b] = run;
        run += (frame_off[b + 1] - frame_off[b] + rnd) >> shift;
    }
    if (tid == 1023) tile_off[n_utt] = part[1023];
}

template <int DC>  // DC > 0: feature width known at compile time (division by a constant); 0: runtime D
__global__ __launch_bounds__(256) void delta_tiled_kernel(const float* __restrict__ in, int64_t ld_in, BatchGeom bg,
                                                          int32_t D_rt, int32_t N, float inv_den,
                                                          float* __restrict__ out, int64_t ld_out,
                                                          float* __restrict__ out_dd, int64_t ld_dd,
                                                          int32_t tiles_per_utt_uniform,
                                                          const int64_t* __restrict__ tile_off) {
    extern __shared__ __attribute__((aligned(16))) float smem_d[];
    const int D = DC > 0 ? DC : D_rt;
    // locate (utterance, tile): wave-uniform scalars
    int64_t base;
    int T, tile;
    if (bg.uniform_frames > 0) {
        const int u = (int)blockIdx.x / tiles_per_utt_uniform;
        tile = (int)blockIdx.x - u * tiles_per_utt_uniform;
        base = (int64_t)u * bg.uniform_frames;
        T = (int)bg.uniform_frames;
    } else {
        if ((int64_t)blockIdx.x >= tile_off[bg.n_utt]) return;  // grid is sized by an upper bound
        const int32_t u = dsp_find_utt(tile_off, bg.n_utt, (int64_t)blockIdx.x);
        tile = (int32_t)(blockIdx.x - tile_off[u]);
        base = bg.frame_off[u];
        T = (int)(bg.frame_off[u + 1] - base);
    }
    const int t0 = tile * DT_TILE;
    const int nt = (T - t0) < DT_TILE ? (T - t0) : DT_TILE;  // frames of this tile
    const int rows_x = nt + 4 * N, rows_d = nt + 2 * N;
    const int ldi = (int)ld_in, ldo = (int)ld_out, ldd = (int)ld_dd;
    const float* in_u = in + base * ld_in;        // utterance-relative 32-bit offsets from here on
    float* out_u = out + (base + t0) * ld_out;
    float* dd_u = out_dd ? out_dd + (base + t0) * ld_dd : nullptr;
    float* sx = smem_d;                           // [rows_x][D]  x[clamp(t0 - 2N + r)]
    float* sd = smem_d + (DT_TILE + 4 * N) * D;   // [rows_d][D]  delta[clamp(t0 - N + r)]
    for (int i = threadIdx.x; i < rows_x * D; i += 256) {
        const int r = i / D, d = i - r * D;
        int tt = t0 - 2 * N + r;
        tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
        sx[i] = in_u[tt * ldi + d];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows_d * D; i += 256) {
        const int r = i / D, d = i - r * D;
        int tt = t0 - N + r;                       // requested frame; delta is evaluated at clamp(tt)
        tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
        const int rc = tt - t0 + 2 * N;            // row of x[tt] in sx
        float acc = 0.f;
        for (int n = 1; n <= N; ++n) acc = fmaf((float)n, sx[(rc + n) * D + d] - sx[(rc - n) * D + d], acc);
        sd[i] = acc * inv_den;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt * D; i += 256) {
        const int r = i / D, d = i - r * D;
        out_u[r * ldo + d] = sd[(r + N) * D + d];
        if (dd_u != nullptr) {
            float acc = 0.f;
            for (int n = 1; n <= N; ++n) acc = fmaf((float)n, sd[(r + N + n) * D + d] - sd[(r + N - n) * D + d], acc);
            dd_u[r * ldd + d] = acc * inv_den;
        }
    }
}

// MFCC + delta + delta-delta rows in one pass: reads the DENSE cepstra [sum T, D] the fused MFCC kernels
// write (full 128-byte lines, no partial-row writes) and emits whole [x | delta | delta2] rows of 3 D
// floats, contiguous per tile, so every output line is written once and completely (base.py:70-79 twice).
template <int DC>
__global__ __launch_bounds__(256) void delta_rows_kernel(const float* __restrict__ in, BatchGeom bg, int32_t D_rt,
                                                         int32_t N, float inv_den, float* __restrict__ out,
                                                         int32_t tiles_per_utt_uniform,
                                                         const int64_t* __restrict__ tile_off,
                                                         const int64_t* __restrict__ seg = nullptr,
                                                         const double* __restrict__ stats = nullptr,
                                                         const int32_t* __restrict__ tile_utt = nullptr) {
    extern __shared__ __attribute__((aligned(16))) float smem_d[];
    __shared__ float s_shift;
    const int D = DC > 0 ? DC : D_rt;
    int64_t base;
    int T, tile;
    int32_t utt_ = 0;
    if (threadIdx.x == 0) s_shift = 0.f;
    if (bg.uniform_frames > 0) {
        const int u = (int)blockIdx.x / tiles_per_utt_uniform;
        tile = (int)blockIdx.x - u * tiles_per_utt_uniform;
        base = (int64_t)u * bg.uniform_frames;
        T = (int)bg.uniform_frames;
    } else {
        if ((int64_t)blockIdx.x >= tile_off[bg.n_utt]) return;  // grid is sized by an upper bound
        // (a table spares the binary search: ten dependent loads are most of this kernel's latency on small tiles)
        const int32_t u = tile_utt != nullptr ? tile_utt[blockIdx.x] : dsp_find_utt(tile_off, bg.n_utt, (int64_t)blockIdx.x);
        tile = (int32_t)(blockIdx.x - tile_off[u]);
        base = bg.frame_off[u];
        T = (int)(bg.frame_off[u + 1] - base);
        // Segments read in place (dsp_mfcc_delta_segments_batch, unit variance): the cepstra are those of the UNSCALED
        // clip.  Dividing the clip by its standard deviation sd scales every power by 1 / sd^2, i.e. adds -ln sd^2 to
        // every log: the cepstra k >= 1 do not move (their DCT rows sum to zero), c0 = log(energy) loses ln(var) --
        // unless the frame's energy was exactly zero (then it is ln(eps) either way, base.py:26).  model.py:62-63.
        utt_ = u;
    }
    // the statistics: loaded here, next to the tile's own loads, turned into the shift (a logarithm) behind them
    double st_n = 0.0, st_s = 0.0, st_q = 0.0;
    if (stats != nullptr && threadIdx.x == 0) {
        st_n = (double)(seg[2 * utt_ + 1] - seg[2 * utt_]);
        st_s = stats[2 * utt_];
        st_q = stats[2 * utt_ + 1];
    }
    const int t0 = tile * DT_TILE;
    const int nt = (T - t0) < DT_TILE ? (T - t0) : DT_TILE;
    const int rows_x = nt + 4 * N, rows_d = nt + 2 * N;
    const float* in_u = in + base * D;
    float* out_u = out + (base + t0) * 3 * D;
    float* sx = smem_d;                           // [rows_x][D]  x[clamp(t0 - 2N + r)]
    float* sd = smem_d + (DT_TILE + 4 * N) * D;   // [rows_d][D]  delta[clamp(t0 - N + r)]
    // all of a thread's loads are issued before the first one is used (eight in flight per thread: the tile
    // is a few KB, the pass is latency bound otherwise)
    for (int i0 = threadIdx.x; i0 < rows_x * D; i0 += 8 * 256) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = i0 + 256 * k;
            const int r = i / D, d = i - r * D;
            int tt = t0 - 2 * N + r;
            tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
            v[k] = i < rows_x * D ? in_u[tt * D + d] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + 256 * k < rows_x * D) sx[i0 + 256 * k] = v[k];
    }
    if (stats != nullptr && threadIdx.x == 0 && st_n > 0.0) {
        const double mean = st_s / st_n;
        const double var = st_q / st_n - mean * mean;
        s_shift = var > 0.0 ? (float)log(var) : 0.f;       // zero variance: sklearn scales by 1
    }
    __syncthreads();
    if (stats != nullptr) {
        // the shift of c0 goes into the window BEFORE the deltas: a frame of exactly zero energy keeps ln(eps) while its
        // neighbours move, so delta and delta-delta of c0 around digital silence see the shifted values, as when the
        // clip is scaled first (model.py:62-63, then base.py:26 and :70-79)
        const float shift = s_shift;
        for (int r = threadIdx.x; r < rows_x; r += 256) {
            const float x0 = sx[r * D];
            if (x0 != -36.04365338911715f) sx[r * D] = x0 - shift;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < rows_d * D; i += 256) {
        const int r = i / D, d = i - r * D;
        int tt = t0 - N + r;
        tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
        const int rc = tt - t0 + 2 * N;
        float acc = 0.f;
        for (int n = 1; n <= N; ++n) acc = fmaf((float)n, sx[(rc + n) * D + d] - sx[(rc - n) * D + d], acc);
        sd[i] = acc * inv_den;
    }
    __syncthreads();
    // thread (r, d) writes x, delta and delta2 of its element: the three stores of a wave cover the same
    // rows back to back, so L2 merges them into whole lines before they leave for HBM
    for (int i = threadIdx.x; i < nt * D; i += 256) {
        const int r = i / D, d = i - r * D;
        float acc = 0.f;
        for (int n = 1; n <= N; ++n) acc = fmaf((float)n, sd[(r + N + n) * D + d] - sd[(r + N - n) * D + d], acc);
        float* o = out_u + r * 3 * D + d;
        o[0] = sx[(r + 2 * N) * D + d];
        o[D] = sd[(r + N) * D + d];
        o[2 * D] = acc * inv_den;
    }
}

template <int DTYPE>
__global__ __launch_bounds__(256) void preemphasis_kernel(const void* __restrict__ wave, const int64_t* __restrict__ off,
                                                          int32_t n_utt, int64_t total, float coeff,
                                                          float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = dsp_find_utt(off, n_utt, i);
        float v = dsp_load_sample<DTYPE>(wave, i);
        if (i > off[u]) v = fmaf(-coeff, dsp_load_sample<DTYPE>(wave, i - 1), v);
        out[i] = v;
    }
}

__global__ __launch_bounds__(256) void scale_columns_kernel(float* __restrict__ x, int64_t rows, int32_t cols,
                                                            const float* __restrict__ scale) {
    const int64_t total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x)
        x[i] *= scale[i % cols];
}

// endpoint.get_amplitude / get_zcr (endpoint.py:109-126,182-198) on rectangular frames
// (sigproc.to_frames, sigproc.py:11-19).  One wavefront per frame, fp64 accumulation.
template <int DTYPE>
__global__ __launch_bounds__(256) void vad_features_kernel(const void* __restrict__ wave, BatchGeom bg, int32_t L,
                                                           int32_t S, int32_t use_sq, double* __restrict__ amp_sum,
                                                           int32_t* __restrict__ zcr) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t total_frames = bg.uniform_frames > 0 ? bg.total_frames : bg.frame_off[bg.n_utt];   // ragged: the table is the truth
    const int64_t n_tiles = (total_frames + 3) / 4;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t g = tile * 4 + wid;
        if (g >= total_frames) continue;
        int32_t utt;
        int64_t t, s0, nsamp;
        dsp_locate(bg, g, utt, t, s0, nsamp);
        const int64_t first = t * (int64_t)S;
        double acc = 0.0;
        int32_t cnt = 0;
        for (int n = lane; n < L; n += 64) {
            const int64_t pos = first + n;
            const float a = pos < nsamp ? dsp_load_sample<DTYPE>(wave, s0 + pos) : 0.f;
            acc += use_sq ? (double)a * (double)a : (double)fabsf(a);
            if (n + 1 < L) {
                const float b = pos + 1 < nsamp ? dsp_load_sample<DTYPE>(wave, s0 + pos + 1) : 0.f;
                cnt += ((a > 0.f && b < 0.f) || (a < 0.f && b > 0.f)) ? 1 : 0;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            acc += __shfl_xor(acc, o, 64);
            cnt += __shfl_xor(cnt, o, 64);
        }
        if (lane == 0) {
            amp_sum[g] = acc;
            zcr[g] = cnt;
        }
    }
}

#define DSP_MAX_SIL 128

// endpoint.amplitude_rule (endpoint.py:133-179, use_acr=False): only the first segment's start and
// the last segment's end are consumed by basic_endpoint_detection (endpoint.py:43,49).
// `voiced` (robust_endpoint_detection, endpoint.py:168-170): a segment only grows over frames whose bit is set.
template <typename AmpT, typename SilT>
__device__ __forceinline__ void amplitude_rule_dev(AmpT amp, int64_t T, double inv_L, double mh,
                                                   double th, int n_l, int n_r, double sigma, double cfg_frame,
                                                   SilT sil, int64_t& left, int64_t& right,
                                                   const uint8_t* __restrict__ voiced = nullptr) {
    int ns = 0;
    const int64_t cl = n_l < T ? n_l : T;                   // amp[:n_l]
    for (int64_t i = 0; i < cl; ++i) sil[ns++] = amp[i] * inv_L;
    const int64_t cr = (n_r == 0 || n_r > T) ? T : n_r;     // amp[-n_r:]  (-0 slices the whole list)
    for (int64_t i = T - cr; i < T; ++i) sil[ns++] = amp[i] * inv_L;
    for (int i = 1; i < ns; ++i) {                          // insertion sort, ns <= 128
        double v = sil[i];
        int j = i - 1;
        while (j >= 0 && sil[j] > v) { sil[j + 1] = sil[j]; --j; }
        sil[j + 1] = v;
    }
    const int m = ns - 2 > 0 ? ns - 2 : 0;                  // sorted(sil)[:-2]
    double mean = 0.0, var = 0.0;
    for (int i = 0; i < m; ++i) mean += sil[i];
    mean = m > 0 ? mean / m : __longlong_as_double(0x7ff8000000000000LL);
    for (int i = 0; i < m; ++i) var += (sil[i] - mean) * (sil[i] - mean);
    const double sd = m > 0 ? sqrt(var / m) : mean;
    double amax = amp[0] * inv_L;
    for (int64_t i = 1; i < T; ++i) { double v = amp[i] * inv_L; amax = v > amax ? v : amax; }
    const double T_H = th / cfg_frame;
    const double M_L = mean + sigma * sd;
    const double a = amax * mh;
    const double M_H = (M_L > a) ? M_L : a;                 // python max(a, M_L): NaN M_L loses
    bool any = false;
    int64_t i = 0;
    while (i < T) {
        if (amp[i] * inv_L >= M_H) {
            int64_t j = i, k = i;
            while (k < T && amp[k] * inv_L > M_H) ++k;
            if ((double)(k - j) < T_H) {
                i = k;
            } else {
                while (j > 0 && amp[j] * inv_L > M_L && (!voiced || voiced[j])) --j;
                while (k < T && amp[k] * inv_L > M_L && (!voiced || voiced[k])) ++k;
                if (!any) { left = j; any = true; }
                right = k;
                i = k;
            }
        }
        ++i;
    }
    if (!any) { left = 0; right = T; }
}

// endpoint.zcr_rule (endpoint.py:201-220; l_sil = 0 -> front slice empty, r_sil = 0.1) and the
// <50-frame fallback of endpoint.py:60-62.
template <typename ZcrT>
__device__ __forceinline__ void endpoint_zcr_rule(ZcrT z, int64_t T, int64_t left, int64_t right, int n_sil,
                                                  double cfg_frame, int32_t* __restrict__ out2) {
    const double max_shift = 0.400 / cfg_frame;
    const int64_t cr = (n_sil == 0 || n_sil > T) ? T : n_sil;
    double mu = 0.0, var = 0.0;
    for (int64_t i = T - cr; i < T; ++i) mu += (double)z[i];
    mu /= (double)cr;
    for (int64_t i = T - cr; i < T; ++i) var += ((double)z[i] - mu) * ((double)z[i] - mu);
    const double thres = mu + 3.0 * sqrt(var / (double)cr);
    int64_t j = left;
    while (j > 0 && (double)(left - j) <= max_shift && (double)z[j] > thres) --j;
    int64_t k = right;
    while (k < T && (double)(k - right) <= max_shift && (double)z[k] > thres) ++k;
    if (k - j < 50) { j = 0; k = T; }                       // endpoint.py:60-62
    out2[0] = (int32_t)j;
    out2[1] = (int32_t)k;
}

template <typename AmpT, typename ZcrT, typename SilT>
__device__ __forceinline__ void endpoint_rule_body(AmpT amp, ZcrT z, SilT sil, int64_t T, double inv_L,
                                                   double cfg_frame, double cfg_step, int32_t* __restrict__ out2,
                                                   const uint8_t* __restrict__ voiced = nullptr) {
    const int n_sil = (int)(0.100 / cfg_step);              // int(l_sil / cfg.step), endpoint.py:151
    int64_t left = 0, right = T;
    if (voiced) {                                           // robust_endpoint_detection: one pass, mh = 0.5 (endpoint.py:73)
        amplitude_rule_dev(amp, T, inv_L, 0.5, 0.100, n_sil, n_sil, 3.0, cfg_frame, sil, left, right, voiced);
    } else {
        amplitude_rule_dev(amp, T, inv_L, 0.25, 0.100, n_sil, n_sil, 3.0, cfg_frame, sil, left, right);
        if (right - left < 50)                              // endpoint.py:44-45
            amplitude_rule_dev(amp, T, inv_L, 0.125, 0.100, n_sil, n_sil, 3.0, cfg_frame, sil, left, right);
    }
    endpoint_zcr_rule(z, T, left, right, n_sil, cfg_frame, out2);
}

#define DSP_RULE_LDS_FRAMES 2048   // utterances up to this many frames are scanned out of LDS

// One wavefront per utterance: the wave copies the utterance's amp / zcr rows into LDS (coalesced),
// then lane 0 runs the sequential state machines against LDS instead of HBM (the scan is a chain of
// dependent loads: ~1 us each from HBM, ~0.05 us from LDS).
__global__ __launch_bounds__(64) void endpoint_rule_kernel(const double* __restrict__ amp_sum,
                                                           const int32_t* __restrict__ zcr,
                                                           const int64_t* __restrict__ frame_off, int32_t n_utt,
                                                           int32_t L, double cfg_frame, double cfg_step,
                                                           int32_t* __restrict__ endpoints,
                                                           // robust_endpoint_detection (endpoint.py:68-92): one bit per frame from
                                                           // acr_gate_kernel; mh = 0.5, a single pass, growth gated by the bit
                                                           const uint8_t* __restrict__ voiced = nullptr) {
    __shared__ double s_amp[DSP_RULE_LDS_FRAMES];
    __shared__ int32_t s_zcr[DSP_RULE_LDS_FRAMES];
    __shared__ double s_sil[DSP_MAX_SIL];
    __shared__ double s_sorted[DSP_MAX_SIL];
    __shared__ double s_thr[3];
    __shared__ unsigned long long s_bits[5][DSP_RULE_LDS_FRAMES / 64];
    const int32_t b = blockIdx.x;
    if (b >= n_utt) return;
    const int64_t base = frame_off[b];
    const int64_t T = frame_off[b + 1] - base;
    const double* amp = amp_sum + base;
    const int32_t* z = zcr + base;
    const double inv_L = 1.0 / (double)L;
    if (T <= DSP_RULE_LDS_FRAMES) {
        // (1) whole wave: copy the rows, running maximum
        const int lane = threadIdx.x;
        double mx = amp[0] * inv_L;
        for (int i = lane; i < (int)T; i += 64) {
            const double v = amp[i] * inv_L;   // the per-frame mean, scaled once instead of at every use
            s_amp[i] = v;
            s_zcr[i] = z[i];
            mx = v > mx ? v : mx;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_xor(mx, o, 64);
            mx = other > mx ? other : mx;
        }
        __syncthreads();
        // (2) silence window amp[:n] + amp[-n:] (endpoint.py:151-153), rank sort (stable: equal keys keep order)
        const int n_sil = (int)(0.100 / cfg_step);
        const int cl = n_sil < (int)T ? n_sil : (int)T;
        const int cr = (n_sil == 0 || n_sil > (int)T) ? (int)T : n_sil;
        const int ns = cl + cr;
        for (int k = lane; k < ns; k += 64) s_sil[k] = k < cl ? s_amp[k] : s_amp[(int)T - cr + (k - cl)];
        __syncthreads();
        for (int k = lane; k < ns; k += 64) {
            const double v = s_sil[k];
            int rank = 0;
            for (int j = 0; j < ns; ++j) {
                const double w = s_sil[j];
                rank += (w < v || (w == v && j < k)) ? 1 : 0;
            }
            s_sorted[rank] = v;
        }
        __syncthreads();
        // (3) lane 0: statistics of sorted(sil)[:-2] in the reference's order, the two thresholds
        if (lane == 0) {
            const int m = ns - 2 > 0 ? ns - 2 : 0;
            double mean = 0.0, var = 0.0;
            for (int i = 0; i < m; ++i) mean += s_sorted[i];
            mean = m > 0 ? mean / m : __longlong_as_double(0x7ff8000000000000LL);
            for (int i = 0; i < m; ++i) var += (s_sorted[i] - mean) * (s_sorted[i] - mean);
            const double sd = m > 0 ? sqrt(var / m) : mean;
            const double M_L = mean + 3.0 * sd;
            const double a1 = mx * (voiced ? 0.5 : 0.25), a2 = mx * 0.125;   // mh (endpoint.py:73: 0.5 with the gate), and the retry of endpoint.py:44-45
            s_thr[0] = M_L;
            s_thr[1] = (M_L > a1) ? M_L : a1;                         // python max(a, M_L): NaN M_L loses
            s_thr[2] = (M_L > a2) ? M_L : a2;
        }
        __syncthreads();
        // (4) whole wave: every comparison the scans can ask for, as one bit per frame in 64-frame ballot
        //     words (bits at and beyond T are clear, so "first clear bit" never runs past T)
        const int words = ((int)T + 63) >> 6;
        {
            const double M_L = s_thr[0], M_H1 = s_thr[1], M_H2 = s_thr[2];
            for (int w = 0; w < words; ++w) {
                const int i = 64 * w + lane;
                const bool ok = i < (int)T;
                const double v = ok ? s_amp[i] : 0.0;
                // with the gate, "amp > M_L" only ever appears as "amp > M_L and voiced" (endpoint.py:168-170)
                const bool vc = voiced == nullptr || (ok && voiced[base + i] != 0);
                const unsigned long long m0 = __ballot(ok && v > M_L && vc), m1 = __ballot(ok && v > M_H1),
                                         m2 = __ballot(ok && v >= M_H1), m3 = __ballot(ok && v > M_H2),
                                         m4 = __ballot(ok && v >= M_H2);
                if (lane == 0) {
                    s_bits[0][w] = m0; s_bits[1][w] = m1; s_bits[2][w] = m2; s_bits[3][w] = m3; s_bits[4][w] = m4;
                }
            }
        }
        __syncthreads();
        if (lane != 0) return;
        // (5) lane 0: the two-threshold scan (endpoint.py:155-179), a word at a time: O(runs), not O(frames)
        auto next_set = [&](const unsigned long long* m, int64_t i) -> int64_t {     // first set bit at >= i, else T
            int w = (int)(i >> 6);
            if (w >= words) return T;
            unsigned long long x = m[w] & (~0ull << (i & 63));
            while (x == 0) {
                if (++w >= words) return T;
                x = m[w];
            }
            return 64 * (int64_t)w + __builtin_ctzll(x);
        };
        auto next_clear = [&](const unsigned long long* m, int64_t i) -> int64_t {   // first clear bit at >= i (<= T)
            int w = (int)(i >> 6);
            if (w >= words) return T;
            unsigned long long x = ~m[w] & (~0ull << (i & 63));
            while (x == 0) {
                if (++w >= words) return T;
                x = ~m[w];
            }
            const int64_t r = 64 * (int64_t)w + __builtin_ctzll(x);
            return r < T ? r : T;
        };
        auto prev_clear = [&](const unsigned long long* m, int64_t i) -> int64_t {   // last clear bit at <= i, else 0
            int w = (int)(i >> 6);
            const int sh = 63 - (int)(i & 63);
            unsigned long long x = (~m[w] << sh) >> sh;                               // bits 0 .. (i & 63)
            while (x == 0) {
                if (--w < 0) return 0;
                x = ~m[w];
            }
            return 64 * (int64_t)w + 63 - __builtin_clzll(x);
        };
        const double T_H = 0.100 / cfg_frame;
        int64_t left = 0, right = T;
        for (int pass = 0; pass < 2; ++pass) {
            const unsigned long long* hi = s_bits[pass == 0 ? 1 : 3];
            const unsigned long long* ge = s_bits[pass == 0 ? 2 : 4];
            const unsigned long long* ml = s_bits[0];
            bool any = false;
            int64_t i = 0;
            while (i < T) {
                i = next_set(ge, i);                      // frames below the entry threshold are stepped over
                if (i >= T) break;
                int64_t j = i, k = next_clear(hi, i);     // while (k < T && amp[k] > M_H) ++k
                if ((double)(k - j) < T_H) {
                    i = k;
                } else {
                    j = prev_clear(ml, j);                // while (j > 0 && amp[j] > M_L) --j
                    k = next_clear(ml, k);                // while (k < T && amp[k] > M_L) ++k
                    if (!any) { left = j; any = true; }
                    right = k;
                    i = k;
                }
                ++i;
            }
            if (!any) { left = 0; right = T; }
            if (right - left >= 50 || voiced != nullptr) break;        // endpoint.py:44-45 (no retry in the robust form)
        }
        endpoint_zcr_rule(s_zcr, T, left, right, n_sil, cfg_frame, endpoints + 2 * b);
    } else {
        if (threadIdx.x != 0) return;
        endpoint_rule_body(amp, z, s_sil, T, inv_L, cfg_frame, cfg_step, endpoints + 2 * b, voiced ? voiced + base : nullptr);
    }
}

// The autocorrelation gate of endpoint.robust_endpoint_detection (endpoint.py:142-144 with sigproc.acr,
// sigproc.py:48-53): frame g is "voiced" when  max_{n in [lag_lo, lag_hi)} (sum_i x[i] x[i+n] / (L - n))  /  (sum_i x[i]^2 / L)
// exceeds `thresh` (0.55), the frame being the rectangular to_frames frame (sigproc.py:11-19, zero padded).
// One wavefront per frame; the frame sits in LDS as fp64 (products of fp32 / int16 samples are exact in fp64, so the sums
// equal NumPy's to the last bits of the additions); lane l takes lags lag_lo + l, + 64, ...: x[i] is a broadcast read,
// x[i + n] a conflict-free one.  A quotient that is NaN (an all-zero frame: 0 / 0) compares false, as in the reference.
template <int DTYPE>
__global__ __launch_bounds__(256) void acr_gate_kernel(const void* __restrict__ wave, BatchGeom bg, int32_t L, int32_t S,
                                                       int32_t lag_lo, int32_t lag_hi, double thresh,
                                                       uint8_t* __restrict__ voiced) {
    extern __shared__ __attribute__((aligned(16))) double acr_smem[];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* const x = acr_smem + (size_t)wid * L;
    const int64_t total_frames = bg.uniform_frames > 0 ? bg.total_frames : bg.frame_off[bg.n_utt];
    const int64_t g = (int64_t)blockIdx.x * 4 + wid;
    if (g >= total_frames) return;                          // (wave-uniform; no barrier below)
    int32_t utt;
    int64_t t, s0, nsamp;
    dsp_locate(bg, g, utt, t, s0, nsamp);
    const int64_t first = t * (int64_t)S;
    double e0 = 0.0;
    for (int i = lane; i < L; i += 64) {
        const double v = first + i < nsamp ? (double)dsp_load_sample<DTYPE>(wave, s0 + first + i) : 0.0;
        x[i] = v;
        e0 = fma(v, v, e0);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e0 += __shfl_xor(e0, o, 64);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the wave's own LDS stores (one wave per frame: no barrier)
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double best = nan;                                      // python max(): the first value, then anything greater
    for (int n = lag_lo + lane; n < lag_hi; n += 64) {
        double a = nan;
        if (n < L) {
            double acc0 = 0.0, acc1 = 0.0;
            const int m = L - n;
            int i = 0;
            for (; i + 1 < m; i += 2) {
                acc0 = fma(x[i], x[i + n], acc0);
                acc1 = fma(x[i + 1], x[i + 1 + n], acc1);
            }
            if (i < m) acc0 = fma(x[i], x[i + n], acc0);
            a = (acc0 + acc1) / (double)m;
        } else if (n == L) {
            a = nan;                                        // numpy: the sum of an empty product is 0, divided by 0
        }
        // (lags beyond L wrap in numpy slicing; no caller's rate / frame length reaches them: rate // 50 < int(0.03 rate))
        if (a > best || !(best == best)) best = a;
    }
    // wave maximum; NaN lanes (no lag) lose to any number
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(best, o, 64);
        best = (other > best || !(best == best)) ? other : best;
    }
    if (lane == 0) voiced[g] = (best / (e0 / (double)L) > thresh) ? 1 : 0;
}

// Inclusive prefix sums over the 64 lanes of a wave without LDS: row_shr 1, 2, 4, 8 inside each row of 16 lanes, then
// row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3 (lanes without a source add zero).
__device__ __forceinline__ int32_t dsp_wave_scan_i32(int32_t v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return v;
}
__device__ __forceinline__ int64_t dsp_wave_scan_i64(int64_t v) {
#define DSP_SCAN64_STEP(CTRL, ROWS)                                                                           \
    {                                                                                                         \
        const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(uint64_t)v, CTRL, ROWS, 0xf, false); \
        const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)v >> 32), CTRL, ROWS, 0xf, false); \
        v += (int64_t)(((uint64_t)hi_ << 32) | lo_);                                                          \
    }
    DSP_SCAN64_STEP(0x111, 0xf)
    DSP_SCAN64_STEP(0x112, 0xf)
    DSP_SCAN64_STEP(0x114, 0xf)
    DSP_SCAN64_STEP(0x118, 0xf)
    DSP_SCAN64_STEP(0x142, 0xa)
    DSP_SCAN64_STEP(0x143, 0xc)
#undef DSP_SCAN64_STEP
    return v;
}

// configs[3] glue, all on the device: endpoint frame indices -> what the trim and feature kernels need.
//   seg[b]      = (int((left  * step) * rate), int((right * step) * rate)) clipped to the clip length
//                 (endpoint.py:64: fp64 products in that order, truncation; numpy slicing clips at the end;
//                 `jitter` adds model.py:54-60's per-utterance offsets first, clamped to [0, len])
//   dst_off[b]  = exclusive prefix of the trimmed lengths      (sample offsets of the trimmed batch)
//   frame_off[b]= exclusive prefix of their frame counts at (L, S)   (sigproc.py:79-82)
// One 1024-thread block; every thread owns a contiguous run of utterances, Hillis-Steele scan across threads.
__global__ __launch_bounds__(1024) void endpoint_layout_kernel(const int32_t* __restrict__ ep_frames,
                                                               const int64_t* __restrict__ src_off, int32_t n_utt,
                                                               double step, double rate, int32_t L, int32_t S,
                                                               const int64_t* __restrict__ jitter,
                                                               int64_t* __restrict__ seg, int64_t* __restrict__ dst_off,
                                                               int64_t* __restrict__ frame_off,
                                                               // optional (dsp_endpoint_layout_segments_batch): the tables
                                                               // dsp_mfcc_delta_segments_batch needs, in the same launch
                                                               int32_t group_shift = 0, int32_t* __restrict__ group_off = nullptr,
                                                               int32_t* __restrict__ group_utt = nullptr,
                                                               int64_t* __restrict__ tile_off = nullptr,
                                                               double* __restrict__ zero_stats = nullptr,
                                                               int32_t* __restrict__ tile_utt = nullptr) {
    __shared__ int64_t part_s[16], part_f[16];
    __shared__ int32_t part_g[16], part_t[16];
    const int64_t rnd_g = ((int64_t)1 << group_shift) - 1, rnd_t = ((int64_t)1 << DT_SHIFT) - 1;
    int32_t sum_g = 0, sum_t = 0;
    const int tid = threadIdx.x;
    const int per = (n_utt + 1023) / 1024;
    const int lo = tid * per, hi = min(lo + per, n_utt);
    int64_t sum_s = 0, sum_f = 0;
    for (int b = lo; b < hi; ++b) {
        const int64_t len = src_off[b + 1] - src_off[b];
        int64_t l = (int64_t)(((double)ep_frames[2 * b] * step) * rate);
        int64_t r = (int64_t)(((double)ep_frames[2 * b + 1] * step) * rate);
        if (jitter != nullptr) {           // model.py:54-60: left -= s_l; right += s_r; negatives -> 0
            l += jitter[2 * b];
            r += jitter[2 * b + 1];
            l = l < 0 ? 0 : l;
            r = r < 0 ? 0 : r;
        }
        l = l > len ? len : l;             // numpy slicing sig[left:right] clips at the end of the clip
        r = r > len ? len : r;
        if (r < l) r = l;
        seg[2 * b] = l;
        seg[2 * b + 1] = r;
        const int64_t n = r - l;
        sum_s += n;
        const int64_t nf = n <= L ? 1 : 1 + (n - L + S - 1) / S;
        sum_f += nf;
        sum_g += (int32_t)((nf + rnd_g) >> group_shift);
        sum_t += (int32_t)((nf + rnd_t) >> DT_SHIFT);
        if (zero_stats != nullptr) { zero_stats[2 * b] = 0.0; zero_stats[2 * b + 1] = 0.0; }
    }
    // inclusive scans of the four per-thread sums: inside each wave with shuffles, across the 16 waves through LDS
    // (two barriers in all; a Hillis-Steele scan over 1024 threads needs twenty)
    // (DPP row shifts + the two row broadcasts: 6 steps of a few VALU instructions; the __shfl_up form was 36
    // ds_bpermute round trips, 2 of this kernel's 8.5 us)
    const int64_t inc_s_ = dsp_wave_scan_i64(sum_s), inc_f_ = dsp_wave_scan_i64(sum_f);
    int64_t inc_s = inc_s_, inc_f = inc_f_;
    int32_t inc_g = dsp_wave_scan_i32(sum_g), inc_t = dsp_wave_scan_i32(sum_t);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 63) { part_s[wv] = inc_s; part_f[wv] = inc_f; part_g[wv] = inc_g; part_t[wv] = inc_t; }
    __syncthreads();
    int64_t tot_s = 0, tot_f = 0;
    int32_t tot_g = 0, tot_t = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int64_t as = part_s[k], af = part_f[k];
        const int32_t ag = part_g[k], at = part_t[k];
        if (k < wv) { inc_s += as; inc_f += af; inc_g += ag; inc_t += at; }
        tot_s += as; tot_f += af; tot_g += ag; tot_t += at;
    }
    int64_t run_s = inc_s - sum_s, run_f = inc_f - sum_f, run_t = (int64_t)(inc_t - sum_t);
    int32_t run_g = inc_g - sum_g;
    for (int b = lo; b < hi; ++b) {
        dst_off[b] = run_s;
        frame_off[b] = run_f;
        const int64_t n = seg[2 * b + 1] - seg[2 * b];
        const int64_t nf = n <= L ? 1 : 1 + (n - L + S - 1) / S;
        run_s += n;
        run_f += nf;
        if (group_off != nullptr) {
            group_off[b] = run_g;
            const int32_t ng = (int32_t)((nf + rnd_g) >> group_shift);
            for (int32_t g = 0; g < ng; ++g) group_utt[run_g + g] = b;
            run_g += ng;
        }
        if (tile_off != nullptr) {
            tile_off[b] = run_t;
            const int64_t nt = (nf + rnd_t) >> DT_SHIFT;
            if (tile_utt != nullptr)
                for (int64_t g = 0; g < nt; ++g) tile_utt[run_t + g] = b;
            run_t += nt;
        }
    }
    if (tid == 1023) {
        dst_off[n_utt] = tot_s;
        frame_off[n_utt] = tot_f;
        if (group_off != nullptr) group_off[n_utt] = tot_g;
        if (tile_off != nullptr) tile_off[n_utt] = (int64_t)tot_t;
    }
}

// Endpoint-trimmed copy of a ragged batch (model.py:52-64 without augmentation): utterance b keeps
// samples [lo_b, hi_b) and is divided by its population standard deviation when `unit_variance`
// (sklearn scale(with_mean=False), zero std -> 1).  One workgroup per utterance; fp64 statistics.
template <int DTYPE>
__global__ __launch_bounds__(256) void trim_scale_kernel(const void* __restrict__ wave, const int64_t* __restrict__ src_off,
                                                         const int64_t* __restrict__ seg, const int64_t* __restrict__ dst_off,
                                                         int32_t unit_variance, float* __restrict__ out) {
    __shared__ double red[2][4];
    const int b = blockIdx.x;
    const int64_t s0 = src_off[b] + seg[2 * b];
    const int64_t n = seg[2 * b + 1] - seg[2 * b];
    float* dst = out + dst_off[b];
    double inv = 1.0;
    if (unit_variance && n > 0) {
        double s = 0.0, q = 0.0;
        // eight independent loads in flight per thread (the loop is latency bound otherwise)
        int64_t i = threadIdx.x;
        for (; i + 7 * 256 < n; i += 8 * 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = dsp_load_sample<DTYPE>(wave, s0 + i + u * 256);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s += (double)v[u];
                q += (double)v[u] * (double)v[u];
            }
        }
        for (; i < n; i += 256) {
            const double v = (double)dsp_load_sample<DTYPE>(wave, s0 + i);
            s += v;
            q += v * v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o, 64);
            q += __shfl_xor(q, o, 64);
        }
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = q; }
        __syncthreads();
        s = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        q = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        const double mean = s / (double)n;
        double var = q / (double)n - mean * mean;
        if (var < 0.0) var = 0.0;
        const double sd = sqrt(var);
        inv = sd > 0.0 ? 1.0 / sd : 1.0;
    }
    int64_t i = threadIdx.x;
    for (; i + 7 * 256 < n; i += 8 * 256) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = dsp_load_sample<DTYPE>(wave, s0 + i + u * 256);
#pragma unroll
        for (int u = 0; u < 8; ++u) dst[i + u * 256] = (float)((double)v[u] * inv);
    }
    for (; i < n; i += 256)
        dst[i] = (float)((double)dsp_load_sample<DTYPE>(wave, s0 + i) * inv);
}

// Optional amplitude stream of model.py:97-101 (cfg.use_timefeat) for a whole batch: per utterance
//   a[t]  = amp_sum[t] / L                 get_amplitude of the trimmed, scaled clip (endpoint.py:109-131)
//   z     = (a - mean) / std               sklearn scale: population std, 0 -> 1
//   out[t, b, 0] = z[t], out[t, b, 1] = z[t + 1] - z[t]  (deviation, model.py:29-33: T - 1 rows),
// each zero padded / truncated to max_len rows (model.py:35-50), at the place `pl` names.  One wave per utterance, fp64.
__global__ __launch_bounds__(64) void timefeat_finalize_kernel(const double* __restrict__ amp_sum,
                                                               const int64_t* __restrict__ frame_off, int32_t n_utt,
                                                               int32_t L, int32_t max_len, float* __restrict__ out,
                                                               OutPlacement pl) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t base = frame_off[b];
    const int T = (int)(frame_off[b + 1] - base);
    const double* a = amp_sum + base;
    float* ob = pl.base(out, pl.col(b));
    const int64_t row = pl.stride();
    const double inv_L = 1.0 / (double)L;
    double s = 0.0;
    for (int t = lane; t < T; t += 64) s += a[t] * inv_L;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const double mu = T > 0 ? s / (double)T : 0.0;
    double v = 0.0;
    for (int t = lane; t < T; t += 64) {
        const double d = a[t] * inv_L - mu;
        v += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const double sd = T > 0 ? sqrt(v / (double)T) : 0.0;
    const double inv = sd == 0.0 ? 1.0 : 1.0 / sd;
    for (int t = lane; t < max_len; t += 64) {
        float z0 = 0.f, z1 = 0.f;
        if (t < T) {
            const double zt = (a[t] * inv_L - mu) * inv;
            z0 = (float)zt;
            if (t + 1 < T) z1 = (float)((a[t + 1] * inv_L - mu) * inv - zt);
        }
        float* o = ob + (int64_t)t * row;
        o[0] = z0;
        o[1] = z1;
    }
}

// model.py:66-88 after the MFCC call, plus the 200-frame layout of model.py:35-50,131-135, one
// workgroup per utterance:
//   x  = mfcc0 - mean(mfcc0)               scalar mean over the whole [T, C] block   (model.py:75)
//   d1 = delta(x, N), d2 = delta(d1, N)    edge replicated, base.py:70-79            (model.py:76-77)
//   z  = (x - mean_c) / std_c              per coefficient, population std, 0 -> 1   (model.py:78)
//   out[t, b, :] = z | d1 | d2 for t < min(T, max_len), zeros up to max_len          (model.py:35-50)
// `pl` says where (t, b, :) lies in `out` and which len0 entry is b's (OutPlacement, dsp_common.h).
// Statistics in fp64 over all T frames; only the first max_len (+ halo) rows are staged in LDS.
__global__ __launch_bounds__(256) void model_finalize_kernel(const float* __restrict__ mfcc, int64_t ld_in,
                                                             const int64_t* __restrict__ frame_off, int32_t n_utt,
                                                             int32_t C, int32_t N, int32_t max_len,
                                                             float* __restrict__ out, int32_t* __restrict__ len0,
                                                             OutPlacement pl,
                                                             // cepstra of segments read IN PLACE (dsp_mfcc_delta_segments_batch,
                                                             // delta_n = 0, unit variance): c0 still lacks the -ln(var) of
                                                             // model.py:62-63 -- applied here, at every read, from the sums
                                                             // the MFCC kernel left (frames of zero energy keep ln(eps))
                                                             const int64_t* __restrict__ seg = nullptr,
                                                             const double* __restrict__ stats = nullptr) {
    extern __shared__ __attribute__((aligned(16))) float fin_smem[];
    __shared__ double red[4];
    __shared__ double s_mu[32], s_inv[32];
    __shared__ double s_part[256];
    __shared__ double s_shift;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t col = pl.col(b);
    if (col < 0) return;             // a pad slot of a rate group (dsp_rate_groups_batch): no rows, no len0; the whole workgroup leaves
    const int64_t base = frame_off[b];
    const int T = (int)(frame_off[b + 1] - base);
    const int keep = T < max_len ? T : max_len;
    const float* in_raw = mfcc + base * ld_in;
    if (tid == 0) {
        double sh = 0.0;
        if (stats != nullptr) {
            const double n = (double)(seg[2 * b + 1] - seg[2 * b]);
            if (n > 0.0) {
                const double mean = stats[2 * b] / n;
                const double var = stats[2 * b + 1] / n - mean * mean;
                sh = var > 0.0 ? log(var) : 0.0;                      // zero variance: sklearn scales by 1
            }
        }
        s_shift = sh;
    }
    __syncthreads();
    const double shift = s_shift;
    auto in = [&](int64_t idx, int c) -> double {                      // element (row idx / ld_in, column c) with the shift of c0
        const float v = in_raw[idx];
        return (c == 0 && stats != nullptr && v != -36.04365338911715f) ? (double)v - shift : (double)v;
    };
    // scalar mean of the block
    double s = 0.0;
    for (int i = tid; i < T * C; i += 256) s += in((int64_t)(i / C) * ld_in + (i % C), i % C);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const double gmean = T > 0 ? (red[0] + red[1] + red[2] + red[3]) / ((double)T * (double)C) : 0.0;
    __syncthreads();
    // per-coefficient mean and population std of x = mfcc - gmean (two passes, like numpy).  All C coefficients at once:
    // thread (c, j) sums every J-th frame of coefficient c, the J partial sums of a coefficient meet in LDS -- two short
    // phases instead of ceil(C / 4) rounds of a wave per coefficient with two 64-lane fp64 butterflies each
    {
        const int J = 256 / C;                       // threads per coefficient (C <= 32: J >= 8)
        const int c = tid / J, j = tid - c * J;
        const bool mine = c < C;
        double a = 0.0;
        if (mine)
            for (int t = j; t < T; t += J) a += (double)(float)(in((int64_t)t * ld_in + c, c) - gmean);
        s_part[tid] = a;
        __syncthreads();
        if (mine && j == 0) {
            double tot = 0.0;
            for (int k = 0; k < J; ++k) tot += s_part[c * J + k];
            s_mu[c] = T > 0 ? tot / (double)T : 0.0;
        }
        __syncthreads();
        double v = 0.0;
        if (mine) {
            const double mu = s_mu[c];
            for (int t = j; t < T; t += J) {
                const double dlt = (double)(float)(in((int64_t)t * ld_in + c, c) - gmean) - mu;
                v += dlt * dlt;
            }
        }
        s_part[tid] = v;
        __syncthreads();
        if (mine && j == 0) {
            double tot = 0.0;
            for (int k = 0; k < J; ++k) tot += s_part[c * J + k];
            const double sd = T > 0 ? sqrt(tot / (double)T) : 0.0;
            s_inv[c] = sd == 0.0 ? 1.0 : 1.0 / sd;
        }
    }
    // stage x rows [0, nx) and d1 rows [0, nd): what the first `keep` output rows can reach
    const int nx = (keep + 2 * N < T) ? keep + 2 * N : T;
    const int nd = (keep + N < T) ? keep + N : T;
    float* sx = fin_smem;                       // [max_len + 2 N, C]
    float* sd1 = fin_smem + (size_t)(max_len + 2 * N) * C;   // [max_len + N, C]
    for (int i = tid; i < nx * C; i += 256)
        sx[i] = (float)(in((int64_t)(i / C) * ld_in + (i % C), i % C) - gmean);
    __syncthreads();
    double den = 0.0;
    for (int n = 1; n <= N; ++n) den += (double)n * n;
    const float inv_den = (float)(1.0 / (2.0 * den));
    auto xat = [&](int t, int c) { t = t < 0 ? 0 : (t >= T ? T - 1 : t); return sx[t * C + c]; };
    for (int i = tid; i < nd * C; i += 256) {
        const int t = i / C, c = i % C;
        float acc = 0.f;
        for (int n = 1; n <= N; ++n) acc = fmaf((float)n, xat(t + n, c) - xat(t - n, c), acc);
        sd1[i] = acc * inv_den;
    }
    __syncthreads();
    auto dat = [&](int t, int c) { t = t < 0 ? 0 : (t >= T ? T - 1 : t); return sd1[t * C + c]; };
    const int64_t row = pl.stride();
    float* ob = pl.base(out, col);
    for (int i = tid; i < max_len * C; i += 256) {
        const int t = i / C, c = i % C;
        float z = 0.f, d1 = 0.f, d2 = 0.f;
        if (t < keep) {
            z = (float)(((double)sx[i] - s_mu[c]) * s_inv[c]);
            d1 = sd1[i];
            float acc = 0.f;
            for (int n = 1; n <= N; ++n) acc = fmaf((float)n, dat(t + n, c) - dat(t - n, c), acc);
            d2 = acc * inv_den;
        }
        float* o = ob + (int64_t)t * row;
        o[c] = z;
        o[C + c] = d1;
        o[2 * C + c] = d2;
    }
    if (tid == 0) len0[col] = keep;
}


// Clip pick[i] of a batch copied, sample type kept, to out + dst_off[i] (dsp_gather_clips_batch): the clips of one sample
// rate of a mixed-rate batch (reader.mini_batch_iterator shuffles the file list, reader.py:80) made one contiguous run.
// GATHER_CHUNKS workgroups share a clip, each striding over it, so one long clip is not one workgroup's work alone.
// Where source and destination are equally misaligned against 16 bytes the body moves as 16-byte vectors with an
// element-wise head and tail; otherwise element by element.
constexpr int GATHER_CHUNKS = 8;
template <typename T>
__global__ __launch_bounds__(256) void gather_clips_kernel(const T* __restrict__ wave, const int64_t* __restrict__ src_off,
                                                           const int32_t* __restrict__ pick, const int64_t* __restrict__ dst_off,
                                                           T* __restrict__ out) {
    constexpr int V = 16 / (int)sizeof(T);
    const int i = blockIdx.y;
    const int32_t u = pick[i];
    const int64_t s0 = src_off[u], n = src_off[u + 1] - s0;
    const T* src = wave + s0;
    T* dst = out + dst_off[i];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    const uintptr_t mis_s = reinterpret_cast<uintptr_t>(src) & 15, mis_d = reinterpret_cast<uintptr_t>(dst) & 15;
    if (mis_s != mis_d) {
        for (int64_t k = tid; k < n; k += nthr) dst[k] = src[k];
        return;
    }
    int64_t head = (int64_t)(((16 - mis_d) & 15) / sizeof(T));
    if (head > n) head = n;
    const int64_t nvec = (n - head) / V;
    for (int64_t k = tid; k < head; k += nthr) dst[k] = src[k];
    const uint4* vs = reinterpret_cast<const uint4*>(src + head);
    uint4* vd = reinterpret_cast<uint4*>(dst + head);
    for (int64_t k = tid; k < nvec; k += nthr) vd[k] = vs[k];
    for (int64_t k = head + nvec * V + tid; k < n; k += nthr) dst[k] = src[k];
}

// dsp_gather_groups_batch: gather_clips_kernel for every rate group of a mixed-rate batch in ONE launch, grid (GATHER_CHUNKS,
// n_utt slots, n_groups).  Slot i of group g holds source clip pick_g[i], copied as above to out_g + offsets_g[i]; a pad slot
// (pick_g[i] < 0, dsp_rate_groups_batch) is filled with `pad` samples of DSP_GROUP_PAD_VALUE, so every sample below
// offsets_g[n_utt] of every group buffer is written by every launch.
struct GatherGroupsArgs {
    const int32_t* pick[DSP_MAX_RATE_GROUPS];
    const int64_t* offsets[DSP_MAX_RATE_GROUPS];
    void* out[DSP_MAX_RATE_GROUPS];
};

template <typename T>
__global__ __launch_bounds__(256) void gather_groups_kernel(const T* __restrict__ wave, const int64_t* __restrict__ src_off,
                                                            int64_t pad, GatherGroupsArgs A) {
    constexpr int V = 16 / (int)sizeof(T);
    const int i = blockIdx.y;
    const int32_t* pick = A.pick[0];
    const int64_t* dst_off = A.offsets[0];
    T* out = static_cast<T*>(A.out[0]);
#pragma unroll
    for (int g = 1; g < DSP_MAX_RATE_GROUPS; ++g)
        if ((int)blockIdx.z == g) { pick = A.pick[g]; dst_off = A.offsets[g]; out = static_cast<T*>(A.out[g]); }
    const int32_t u = pick[i];
    T* dst = out + dst_off[i];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    if (u < 0) {
        for (int64_t k = tid; k < pad; k += nthr) dst[k] = (T)DSP_GROUP_PAD_VALUE;
        return;
    }
    if (u >= (int32_t)gridDim.y) return;             // not a clip of this batch: nothing is read through it
    const int64_t s0 = src_off[u], n = src_off[u + 1] - s0;
    const T* src = wave + s0;
    const uintptr_t mis_s = reinterpret_cast<uintptr_t>(src) & 15, mis_d = reinterpret_cast<uintptr_t>(dst) & 15;
    if (mis_s != mis_d) {
        for (int64_t k = tid; k < n; k += nthr) dst[k] = src[k];
        return;
    }
    int64_t head = (int64_t)(((16 - mis_d) & 15) / sizeof(T));
    if (head > n) head = n;
    const int64_t nvec = (n - head) / V;
    for (int64_t k = tid; k < head; k += nthr) dst[k] = src[k];
    const uint4* vs = reinterpret_cast<const uint4*>(src + head);
    uint4* vd = reinterpret_cast<uint4*>(dst + head);
    for (int64_t k = tid; k < nvec; k += nthr) vd[k] = vs[k];
    for (int64_t k = head + nvec * V + tid; k < n; k += nthr) dst[k] = src[k];
}

// dsp_scatter_segments_batch: the [n_utt, 2] segment tables the groups' endpoint kernels wrote in slot order, brought back to
// batch order: endpoints[dst_col_g[k]] = seg_g[k] for every real slot, pad slots (dst_col_g[k] < 0) skipped.  The groups
// partition the batch, so every row of `endpoints` is written exactly once.  Grid (ceil(n_utt / 256), n_groups).
struct ScatterSegmentsArgs {
    const int64_t* seg[DSP_MAX_RATE_GROUPS];
    const int32_t* dst_col[DSP_MAX_RATE_GROUPS];
};

__global__ __launch_bounds__(256) void scatter_segments_kernel(ScatterSegmentsArgs A, int32_t n_utt, int64_t* __restrict__ endpoints) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_utt) return;
    const int64_t* seg = A.seg[0];
    const int32_t* dst_col = A.dst_col[0];
#pragma unroll
    for (int g = 1; g < DSP_MAX_RATE_GROUPS; ++g)
        if ((int)blockIdx.y == g) { seg = A.seg[g]; dst_col = A.dst_col[g]; }
    const int32_t col = dst_col[k];
    if (col < 0 || col >= n_utt) return;
    endpoints[2 * (int64_t)col] = seg[2 * (int64_t)k];
    endpoints[2 * (int64_t)col + 1] = seg[2 * (int64_t)k + 1];
}

// dsp_scatter_group_rows_batch: the same way back for rows of row_words 4-byte words (the pitch tail's [n_utt, 5] fp64 features
// and [n_utt, 9] int32 details, which each group computes over all its slots): out[dst_col_g[k]] = rows_g[k], a pad slot
// (dst_col_g[k] < 0) or a column that is no row of the batch skipped WITHOUT reading its row -- a pad slot's row may be NaN.
// One thread per word, so neighbouring lanes move neighbouring words; grid (ceil(n_utt * row_words / 256), n_groups).
struct ScatterRowsArgs {
    const uint32_t* rows[DSP_MAX_RATE_GROUPS];
    const int32_t* dst_col[DSP_MAX_RATE_GROUPS];
};

__global__ __launch_bounds__(256) void scatter_group_rows_kernel(ScatterRowsArgs A, int32_t n_utt, int32_t row_words,
                                                                 uint32_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t k = idx / row_words;
    if (k >= n_utt) return;
    const int64_t w = idx - k * row_words;
    const uint32_t* rows = A.rows[0];
    const int32_t* dst_col = A.dst_col[0];
#pragma unroll
    for (int g = 1; g < DSP_MAX_RATE_GROUPS; ++g)
        if ((int)blockIdx.y == g) { rows = A.rows[g]; dst_col = A.dst_col[g]; }
    const int32_t col = dst_col[k];
    if (col < 0 || col >= n_utt) return;
    out[(int64_t)col * row_words + w] = rows[k * row_words + w];
}
