// fp64 repair of cancelled mel filters (base.py:28-30 at frames where the fp32 spectrum cannot carry them).
//
// A mel filter made of one or two FFT bins (filter 0 of the 40-filter bank is bin 1 alone) can come out many orders of
// magnitude below the frame's energy when pre-emphasis and window nearly cancel those bins.  An fp32 transform has an
// absolute error of a few 1e-7 of the frame's RMS spectrum in EVERY bin, so the logarithm of such a filter -- and with
// it c1..c12 of the frame -- is lost, whatever the FFT.  The MFCC kernels therefore compare every filter output with the
// frame's energy; where it is below DSP_REPAIR_RATIO times the energy (rare: a wave-uniform branch behind one scalar test),
// the whole wave recomputes that filter's bins as direct DFT sums in fp64 from the samples, re-read from memory, with
// the fp64 window, the fp64 pre-emphasis coefficient and an exact fp64 twiddle table (cos / sin of 2 pi k / NFFT, indexed
// by k n mod NFFT), and the result replaces the fp32 one in front of the logarithm.  The criterion is on the filter's
// OUTPUT: the tap count does not enter.  No atomics, no allocation: the same input gives the same bits.
#pragma once

#include "dsp_common.h"

// filter output / frame energy below which a filter is recomputed.  DESIGN section 4 has the measured error per
// cancellation ratio without the repair and how this value follows from it: a one-bin filter at 5e-4 of the frame's
// median bin magnitude is 7e-10 of the frame's energy (257 bins); the first ratio at which the unrepaired kernels miss
// 5e-5 is 1e-4.  Every flagged filter costs its wave a few microseconds, so the margin is not made larger than that:
// at 7e-10 a white-noise batch flags one frame in 4 000.
// The value was derived at NFFT 512 (K = 257 bins) and holds as it is for every plan with at least that many bins (the
// NFFT = 512 and 1536 kernels use the constant itself; measured on the generic kernel without the repair, white noise at
// NFFT 256 .. 4096 never misses 5e-5 above it).  With fewer bins one bin is a larger share of the energy, the filterbank
// is smaller and so are the cepstra the error is held against.  profiles/generic_repair_sweep.txt has the generic kernel's
// error against the smallest filter / energy ratio of a frame per NFFT: no frame misses 5e-5 above 7e-7 at 9 bins, 2e-7 at
// 13, 7e-9 at 33, 65 and 97 bins, 7e-10 from 129 bins on -- steeper than 257 / K and, at 97 bins, than its square.
// dsp_repair_threshold is the constant times (257 / K)^3 below 257 bins: the same value at 257, never a smaller one, at
// least 1.9 times every figure above.  It flags a few per cent of all frames at the smallest sizes, where the fp64 sum
// over a frame of 16 .. 200 samples costs next to nothing.
// -DDSP_REPAIR_RATIO=0.f switches the repair off in every kernel (nothing is below zero): the build the "without the
// repair" figures were measured on.  -DDSP_REPAIR_BINS=0 keeps the constant at every size (the rule before the sweep).
#ifndef DSP_REPAIR_RATIO
#define DSP_REPAIR_RATIO 7e-10f
#endif
#ifndef DSP_REPAIR_BINS
#define DSP_REPAIR_BINS 257
#endif

// The threshold of a plan with K = NFFT / 2 + 1 bins (tests/generic_cases.py mirrors it operation by operation).
__host__ __device__ __forceinline__ float dsp_repair_threshold(int K) {
    if (K >= DSP_REPAIR_BINS) return DSP_REPAIR_RATIO;
    const float s = (float)DSP_REPAIR_BINS / (float)K;
    return DSP_REPAIR_RATIO * (s * s * s);
}

// One per plan with mel tables, in device memory (host memory under dsp_debug_host_dry_run).
struct DspRepairTab {
    double preemph;           // the coefficient in fp64 (dsp_plan_desc::preemph64)
    int32_t lfft, nfft;       // samples of a frame that reach the transform, its size
    const double* window;     // [lfft]  fp64 window (dsp_plan_desc::h_window64)
    const double* tw;         // [nfft][2]  cos, sin of 2 pi k / nfft
    const int32_t* mel_start; // the plan's CSR mel tables
    const int32_t* mel_count;
    const int32_t* mel_off;
    const float* mel_w;
};

// Output of mel filter j for the frame that starts at sample `first` of the utterance [s0, s0 + nsamp): sum_i w[i] |X[b0 + i]|^2 / nfft.
// Called by all 64 lanes of a wave with the same arguments; every lane returns the same value.
template <int DTYPE>
__device__ __forceinline__ double dsp_repair_mel_f64(const DspRepairTab* __restrict__ R, const void* __restrict__ wave,
                                                     int64_t s0, int64_t nsamp, int64_t first, int j, int lane) {
    const double pre = R->preemph;
    const int lfft = R->lfft, nfft = R->nfft;
    const double* __restrict__ win = R->window;
    const double* __restrict__ tw = R->tw;
    const int b0 = R->mel_start[j], cnt = R->mel_count[j];
    const float* __restrict__ w = R->mel_w + R->mel_off[j];
    const double inv_nfft = 1.0 / (double)nfft;
    double acc = 0.0;
    for (int i = 0; i < cnt; ++i) {
        const int k = b0 + i;
        double re = 0.0, im = 0.0;
        for (int n = lane; n < lfft; n += 64) {
            const int64_t pos = first + n;
            if (pos >= nsamp) break;                       // zero padding behind the utterance's end (sigproc.py:84-86)
            double v = (double)dsp_load_sample<DTYPE>(wave, s0 + pos);
            if (pre != 0.0 && pos > 0) v -= pre * (double)dsp_load_sample<DTYPE>(wave, s0 + pos - 1);   // sigproc.py:185
            v *= win[n];
            const int idx = (int)((uint32_t)(k * n) % (uint32_t)nfft);   // k <= nfft / 2, n < nfft <= 4096: the product fits
            re = fma(v, tw[2 * idx], re);
            im = fma(v, tw[2 * idx + 1], im);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            re += __shfl_xor(re, o, 64);
            im += __shfl_xor(im, o, 64);
        }
        acc = fma((double)w[i], fma(re, re, im * im) * inv_nfft, acc);
    }
    return acc;
}
