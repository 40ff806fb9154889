// C ABI of libdsp_frontend.so (see include/dsp_frontend.h).  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_generic.h"
#include "kernels_fast512.h"
#include "kernels_fast1536.h"
#include "kernels_mfma512.h"
#include "kernels_mfma512t.h"
#include "kernels_vad.h"
#include "kernels_pitch.h"
#include "kernels_cepstrum.h"

thread_local int g_host_dry_run = 0;   // dsp_debug_host_dry_run: plan tables in host memory (sanitizer build, no GPU)

// A batch shape's index tables, built once (include/dsp_frontend.h: dsp_layout).
struct dsp_layout {
    int32_t n_utt, frame_len, frame_step, shift;
    int64_t n_frames_total;
    int32_t* group_off;
    int32_t* group_utt;
    int32_t* group_off2;   // tables of the int16 VAD kernel's 8-frame groups, where it uses them (vad_scan_frames8)
    int32_t* group_utt2;
    int device;
    int capacity;          // dsp_layout_create_capacity: n_frames_total is a BOUND, the tables are rebuilt by dsp_layout_refresh
    int dry_run;           // tables in HOST memory (dsp_debug_host_dry_run): the handle can be destroyed, nothing else
};

static thread_local std::string g_err;  // dsp_last_error

int dsp_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {

thread_local int g_force_generic = 0;   // test switch, per calling thread: other threads' calls are unaffected

template <typename T>
int upload(T** d, const T* h, size_t n) {
    *d = nullptr;
    if (n == 0) return DSP_OK;
    HIP_TRY(dsp_table_alloc_copy(reinterpret_cast<void**>(d), h, n * sizeof(T)));
    return DSP_OK;
}

// the pass list of a transform of n2 = 2^a 3^b 5^c points: the 3s, the 5s, the 4s, a last 2.  For 2^k and 3 * 2^k (the
// sizes dsp_plan_create accepts, and every convolution length of the chirp-z route) that is one optional 3, 4s and a 2
bool factor_half_fft(int n2, std::vector<int>& radix) {
    radix.clear();
    while (n2 % 3 == 0) { radix.push_back(3); n2 /= 3; }
    while (n2 % 5 == 0) { radix.push_back(5); n2 /= 5; }
    while (n2 % 4 == 0) { radix.push_back(4); n2 /= 4; }
    if (n2 % 2 == 0) { radix.push_back(2); n2 /= 2; }
    return n2 == 1 && radix.size() <= DSP_MAX_RADIX_PASSES;
}

bool is_pow2_or_3pow2(int n) {
    if (n > 0 && n % 3 == 0) n /= 3;
    return n > 0 && (n & (n - 1)) == 0;
}

// smallest 2^k or 3 * 2^k that is >= n
int chirp_conv_len(int n) {
    int best = 1;
    while (best < n) best <<= 1;
    for (int m = 3; m < best; m <<= 1)
        if (m >= n) { best = m; break; }
    return best;
}

// dif_pass of kernels_generic.h in fp64 on the host, all passes: natural order in, the kernels' digit-reversed order out.
// O(n log n): the butterflies are direct R-point sums over an exact root table.
void host_dif_f64(std::vector<std::complex<double>>& a, const std::vector<int>& radix) {
    const int n = (int)a.size();
    std::vector<std::complex<double>> tw(n);
    for (int k = 0; k < n; ++k) {
        const double ang = -2.0 * M_PI * (double)k / (double)n;
        tw[k] = std::complex<double>(cos(ang), sin(ang));
    }
    int blk = n;
    for (int R : radix) {
        const int sub = blk / R, twstep = n / blk;
        for (int b = 0; b < n / R; ++b) {
            const int j = b % sub, base = (b - j) * R + j;
            std::complex<double> u[5], y[5];
            for (int q = 0; q < R; ++q) u[q] = a[base + q * sub];
            for (int q2 = 0; q2 < R; ++q2) {
                y[q2] = u[0];
                for (int q = 1; q < R; ++q) y[q2] += u[q] * tw[(size_t)((q * q2) % R) * (n / R)];
                y[q2] *= tw[(size_t)j * q2 * twstep];
            }
            for (int q = 0; q < R; ++q) a[base + q * sub] = y[q];
        }
        blk /= R;
    }
}

// The tables of the chirp-z route (GenericParams::cz_*), built in fp64 and rounded to fp32 once.
void chirp_tables(int nfft, int lfft, int K, int conv_len, const std::vector<int>& radix, std::vector<float2>& w,
                  std::vector<float2>& spec, std::vector<float2>& tw) {
    std::vector<std::complex<double>> w64(nfft);
    w.resize(nfft);
    for (int n = 0; n < nfft; ++n) {
        const int64_t r = ((int64_t)n * n) % (2 * (int64_t)nfft);       // the argument reduced in integers
        const double ang = -M_PI * (double)r / (double)nfft;
        w64[n] = std::complex<double>(cos(ang), sin(ang));
        w[n] = make_float2((float)w64[n].real(), (float)w64[n].imag());
    }
    // conj(w)[m], m = -(lfft - 1) .. K - 1, laid out circularly
    std::vector<std::complex<double>> h(conv_len, std::complex<double>(0.0, 0.0));
    for (int m = 0; m < K; ++m) h[m] = std::conj(w64[m]);
    for (int m = 1; m < lfft; ++m) h[conv_len - m] = std::conj(w64[m]);
    host_dif_f64(h, radix);
    spec.resize(conv_len);
    tw.resize(conv_len);
    const double inv = 1.0 / (double)conv_len;
    for (int i = 0; i < conv_len; ++i) {
        spec[i] = make_float2((float)(h[i].real() * inv), (float)(h[i].imag() * inv));
        const double ang = -2.0 * M_PI * (double)i / (double)conv_len;
        tw[i] = make_float2((float)cos(ang), (float)sin(ang));
    }
}

int check_geom(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
               const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total,
               int64_t uniform_samples) {
    if (!d_wave) return dsp_fail(DSP_EINVAL, "d_wave is NULL");
    if (wave_dtype != DSP_WAVE_F32 && wave_dtype != DSP_WAVE_I16)
        return dsp_fail(DSP_EINVAL, "unsupported wave_dtype %d", wave_dtype);
    if (n_utt <= 0 || n_frames_total <= 0) return dsp_fail(DSP_EINVAL, "empty batch (n_utt=%d, frames=%lld)", n_utt, (long long)n_frames_total);
    if (uniform_samples <= 0 && (!d_sample_offsets || !d_frame_offsets))
        return dsp_fail(DSP_EINVAL, "ragged batch needs d_sample_offsets and d_frame_offsets");
    return DSP_OK;
}

BatchGeom make_geom(const int64_t* d_sample_offsets, const int64_t* d_frame_offsets, int32_t n_utt,
                    int64_t n_frames_total, int64_t uniform_samples, int32_t L, int32_t S) {
    BatchGeom bg;
    bg.sample_off = d_sample_offsets;
    bg.frame_off = d_frame_offsets;
    bg.uniform_samples = uniform_samples > 0 ? uniform_samples : 0;
    bg.uniform_frames = 0;
    if (uniform_samples > 0) {
        int64_t T;
        dsp_frame_count(uniform_samples, L, S, &T);
        bg.uniform_frames = T;
    }
    bg.total_frames = n_frames_total;
    bg.n_utt = n_utt;
    bg.seg = nullptr;
    bg.stats = nullptr;
    return bg;
}

GenericParams generic_params(const dsp_plan* p) {
    GenericParams P;
    memset(&P, 0, sizeof(P));
    P.L = p->L; P.S = p->S; P.nfft = p->nfft; P.K = p->K; P.M = p->M; P.C = p->C;
    P.lfft = p->lfft; P.append_energy = p->append_energy; P.preemph = p->preemph;
    P.window = p->d_window; P.tw = p->d_twiddle;
    P.mel_start = p->d_mel_start; P.mel_count = p->d_mel_count; P.mel_off = p->d_mel_off;
    P.mel_w = p->d_mel_w; P.dct = p->d_dct;
    P.repair = static_cast<const DspRepairTab*>(p->d_repair);
    P.n_pass = p->n_pass;
    for (int i = 0; i < P.n_pass; ++i) P.radix[i] = p->radix[i];
    P.conv_len = p->conv_len; P.cz_w = p->d_cz_w; P.cz_spec = p->d_cz_spec; P.cz_tw = p->d_cz_tw;
    return P;
}

// sample_off'[b] = (dense ? b * n : sample_off[b]) + shift, frame_off'[b] = dense ? b * t : frame_off[b]
__global__ void offsets_view_kernel(const int64_t* __restrict__ src_sample, const int64_t* __restrict__ src_frame,
                                    int64_t* __restrict__ sample_off, int64_t* __restrict__ frame_off,
                                    int32_t n_utt, int64_t n, int64_t t, int64_t shift) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b <= n_utt; b += gridDim.x * blockDim.x) {
        sample_off[b] = (src_sample ? src_sample[b] : (int64_t)b * n) + shift;
        frame_off[b] = src_frame ? src_frame[b] : (int64_t)b * t;
    }
}

// dsp_batch_offsets_batch: one workgroup.  Clip b (b = 1024 p + tid in pass p) reads in[b], in[b + 1]; the sanitised table is a
// running maximum (out[b + 1] = clamp(in[b + 1], out[b], cap) = min(cap, max(0, in[1], .., in[b + 1]))), the frame offsets running
// sums of T(out[b + 1] - out[b]); both scans run inside the waves with shuffles and across the 16 waves through LDS, and carry from
// pass to pass.  Plain vector stores only; every word of every output is written.
#define DSP_MAX_FRAMINGS 4
struct BatchOffsetsArgs {
    int32_t n_framings;
    int32_t L[DSP_MAX_FRAMINGS], S[DSP_MAX_FRAMINGS];
    int64_t* frame_off[DSP_MAX_FRAMINGS];
};

template <bool MAX>
__device__ __forceinline__ int64_t block_scan_i64(int64_t v, int64_t* wtot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t t = __shfl_up(v, off, 64);
        if (lane >= off) v = MAX ? (t > v ? t : v) : v + t;
    }
    if (lane == 63) wtot[w] = v;
    __syncthreads();
    for (int k = 0; k < w; ++k) {
        const int64_t t = wtot[k];
        v = MAX ? (t > v ? t : v) : v + t;
    }
    __syncthreads();       // wtot is free again
    return v;
}

__global__ __launch_bounds__(1024) void batch_offsets_kernel(const int64_t* __restrict__ in, int32_t n_utt, int64_t cap,
                                                             BatchOffsetsArgs A, int64_t* __restrict__ out,
                                                             int32_t* __restrict__ status) {
    __shared__ int64_t wtot[16];
    __shared__ int64_t incl[1024];
    __shared__ int64_t carry[1 + DSP_MAX_FRAMINGS];      // running maximum, running frame sums
    const int tid = threadIdx.x;
    if (tid == 0) {
        out[0] = 0;
        carry[0] = 0;
        for (int f = 0; f < A.n_framings; ++f) { carry[1 + f] = 0; A.frame_off[f][0] = 0; }
    }
    int flags = 0;
    __syncthreads();
    for (int base = 0; base < n_utt; base += 1024) {
        const int b = base + tid;
        const bool live = b < n_utt;
        const int64_t lo = live ? in[b] : 0, hi = live ? in[b + 1] : 0;
        if (live) {
            if (b == 0 && lo != 0) flags |= 1;
            if (hi < lo) flags |= 2;
            if (hi > cap || (b == 0 && lo > cap)) flags |= 4;
            if (hi == lo) flags |= 8;
        }
        const int64_t before = carry[0];
        int64_t m = block_scan_i64<true>(live ? hi : 0, wtot);      // max over this pass's in[base + 1 .. b + 1]
        m = m > before ? m : before;
        incl[tid] = m;
        __syncthreads();
        const int64_t mprev = tid == 0 ? before : incl[tid - 1];
        const int64_t end = m < cap ? m : cap, start = mprev < cap ? mprev : cap;
        if (live) out[b + 1] = end;
        const int64_t n = end - start;
        for (int f = 0; f < A.n_framings; ++f) {
            const int64_t L = A.L[f], S = A.S[f];
            const int64_t T = !live ? 0 : (n <= L ? 1 : 1 + (n - L + S - 1) / S);
            const int64_t sum_before = carry[1 + f];
            const int64_t sum = block_scan_i64<false>(T, wtot) + sum_before;
            if (live) A.frame_off[f][b + 1] = sum;
            if (tid == 1023) carry[1 + f] = sum;         // read by everyone above, before the scan's barriers
        }
        if (tid == 1023) carry[0] = m;
        __syncthreads();
    }
    // the OR of every thread's bits: inside the waves with shuffles, across them through LDS
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) flags |= __shfl_xor(flags, off, 64);
    if ((tid & 63) == 0) wtot[tid >> 6] = flags;
    __syncthreads();
    if (tid == 0) {
        int all = 0;
        for (int k = 0; k < 16; ++k) all |= (int)wtot[k];
        *status = all;
    }
}

// dsp_rate_groups_batch: one workgroup, built like batch_offsets_kernel.  Clip b (b = 1024 p + tid in pass p) is sanitised
// as there (running maximum, clamped to the capacity), matched against the table of known rates (no match: group 0 and
// status bit 4), and per group g two sum-scans over batch order -- of the flag "clip b is in g" and of flag * length -- give
// its slot k and the rebased offset of that slot: a stable partition, group_by_rate's order (model_glue.py).  Both scans carry
// from pass to pass.  Behind the real slots every group's tables are completed with pad slots (pick = dst_col = -1, a clip
// of `pad` samples, zero jitter), so each table has n_utt slots whatever the rates are.  Plain vector stores and fixed
// scans: no atomics, no memset, the same bits on every run; every word of every table is written.
struct RateGroupsArgs {
    int32_t n_groups;
    int32_t rate[DSP_MAX_RATE_GROUPS];
    int32_t* pick[DSP_MAX_RATE_GROUPS];
    int32_t* dst_col[DSP_MAX_RATE_GROUPS];
    int64_t* offsets[DSP_MAX_RATE_GROUPS];
    int64_t* jitter[DSP_MAX_RATE_GROUPS];       // all NULL without a source jitter table
};

__global__ __launch_bounds__(1024) void rate_groups_kernel(const int32_t* __restrict__ rates, const int64_t* __restrict__ in,
                                                           const int64_t* __restrict__ jitter, int32_t n_utt, int64_t cap,
                                                           int64_t pad, RateGroupsArgs A, int64_t* __restrict__ out,
                                                           int32_t* __restrict__ count, int32_t* __restrict__ status) {
    __shared__ int64_t wtot[16];
    __shared__ int64_t incl[1024];
    __shared__ int64_t carry[1 + 2 * DSP_MAX_RATE_GROUPS];      // running maximum; per group: slots so far, samples so far
    const int tid = threadIdx.x;
    if (tid == 0) {
        out[0] = 0;
        for (int k = 0; k < 1 + 2 * DSP_MAX_RATE_GROUPS; ++k) carry[k] = 0;
    }
    int flags = 0;
    __syncthreads();
    for (int base = 0; base < n_utt; base += 1024) {
        const int b = base + tid;
        const bool live = b < n_utt;
        const int64_t lo = live ? in[b] : 0, hi = live ? in[b + 1] : 0;
        int grp = -1;
        if (live) {
            if (b == 0 && lo != 0) flags |= 1;
            if (hi < lo) flags |= 2;
            if (hi > cap || (b == 0 && lo > cap)) flags |= 4;
            if (hi == lo) flags |= 8;
            const int32_t r = rates[b];
            for (int g = A.n_groups - 1; g >= 0; --g)
                if (r == A.rate[g]) grp = g;
            if (grp < 0) { flags |= 16; grp = 0; }                   // an unknown rate: defined and memory-safe, reported
        }
        const int64_t before = carry[0];
        int64_t m = block_scan_i64<true>(live ? hi : 0, wtot);
        m = m > before ? m : before;
        incl[tid] = m;
        __syncthreads();
        const int64_t mprev = tid == 0 ? before : incl[tid - 1];
        const int64_t end = m < cap ? m : cap, start = mprev < cap ? mprev : cap;
        if (live) out[b + 1] = end;
        const int64_t n = end - start;
        for (int g = 0; g < A.n_groups; ++g) {
            const bool mine = grp == g;
            const int64_t k_before = carry[1 + 2 * g], s_before = carry[2 + 2 * g];
            const int64_t k_incl = block_scan_i64<false>(mine ? 1 : 0, wtot) + k_before;
            const int64_t s_incl = block_scan_i64<false>(mine ? n : 0, wtot) + s_before;
            if (mine) {
                const int64_t k = k_incl - 1;
                A.pick[g][k] = b;
                A.dst_col[g][k] = b;
                A.offsets[g][k] = s_incl - n;
                if (jitter != nullptr) {
                    A.jitter[g][2 * k] = jitter[2 * (int64_t)b];
                    A.jitter[g][2 * k + 1] = jitter[2 * (int64_t)b + 1];
                }
            }
            if (tid == 1023) { carry[1 + 2 * g] = k_incl; carry[2 + 2 * g] = s_incl; }   // read by everyone above, before the scans' barriers
        }
        if (tid == 1023) carry[0] = m;
        __syncthreads();
    }
    // pad slots: from the group's count up to n_utt; offsets[cnt] is the end of the real clips, offsets[n_utt] the group's total
    for (int g = 0; g < A.n_groups; ++g) {
        const int64_t cnt = carry[1 + 2 * g], tot = carry[2 + 2 * g];
        for (int64_t k = cnt + tid; k <= n_utt; k += 1024) {
            A.offsets[g][k] = tot + (k - cnt) * pad;
            if (k < n_utt) {
                A.pick[g][k] = -1;
                A.dst_col[g][k] = -1;
                if (jitter != nullptr) { A.jitter[g][2 * k] = 0; A.jitter[g][2 * k + 1] = 0; }
            }
        }
        if (tid == 0) count[g] = (int32_t)cnt;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) flags |= __shfl_xor(flags, off, 64);
    if ((tid & 63) == 0) wtot[tid >> 6] = flags;
    __syncthreads();
    if (tid == 0) {
        int all = 0;
        for (int k = 0; k < 16; ++k) all |= (int)wtot[k];
        *status = all;
    }
}

// Can the vector kernels (the NFFT = 512 and 1536 MFCC kernels, the VAD tile kernels) read this batch where it lies?
// They load 16-byte vectors of four samples (8 bytes for int16), so the buffer must start on one; the dense
// instantiations also need N % 4 == 0 (a vector must not straddle two utterances; ragged batches take any lengths and
// offsets); and the group counters are 32-bit.  `frames_per_group`: the frames one wave takes at a time.
bool vector_kernels_can_read(const BatchGeom& bg, const void* d_wave, int dtype, int64_t frames_per_group) {
    if ((reinterpret_cast<uintptr_t>(d_wave) % (dtype == DSP_WAVE_I16 ? 8 : 16)) != 0) return false;
    if (bg.uniform_samples > 0) {
        if ((bg.uniform_samples % 4) != 0) return false;
        return bg.uniform_samples <= 0x3fffffff &&
               ((bg.uniform_frames + frames_per_group - 1) / frames_per_group) * bg.n_utt <= 0x3fffffff;
    }
    return bg.total_frames / frames_per_group + bg.n_utt <= 0x3fffffff;
}
bool fast512_applicable(const dsp_plan* p, const BatchGeom& bg, const void* d_wave, int dtype) {
    return p->d_fast && vector_kernels_can_read(bg, d_wave, dtype, 8);
}
bool fast1536_applicable(const dsp_plan* p, const BatchGeom& bg, const void* d_wave, int dtype) {
    return p->d_fast1536 && vector_kernels_can_read(bg, d_wave, dtype, 4);
}
bool vad_tile_applicable(const BatchGeom& bg, const void* d_wave, int dtype, int FR) {
    return FR != 0 && vector_kernels_can_read(bg, d_wave, dtype, FR);
}

// A batch that fails the alignment or the N % 4 rule above is still a perfectly good ragged batch of a buffer that
// starts a few samples earlier: write offset tables (arithmetic for dense input, shifted copies otherwise) into a pooled
// workspace and describe it that way.  `d_wave` is moved down to the aligned address.
// Returns nullptr and changes nothing if no view is needed or the workspace cannot be had.
DspWorkspace* fused_kernel_view(BatchGeom& bg, const void*& d_wave, int wave_dtype, hipStream_t st) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_wave);
    const size_t elem = wave_dtype == DSP_WAVE_I16 ? 2 : 4;
    const uintptr_t mis = addr % (4 * elem);               // bytes past the previous aligned vector
    const bool odd_dense = bg.uniform_samples > 0 && (bg.uniform_samples % 4) != 0;
    if ((mis == 0 && !odd_dense) || (mis % elem) != 0) return nullptr;
    DspWorkspace* w = dsp_workspace_pool().acquire(2 * ((size_t)bg.n_utt + 1) * sizeof(int64_t), st);
    if (!w) return nullptr;
    int64_t* so = static_cast<int64_t*>(w->ptr);
    int64_t* fo = so + bg.n_utt + 1;
    const int blocks = (bg.n_utt + 256) / 256 < 1024 ? (bg.n_utt + 256) / 256 : 1024;
    const bool dense = bg.uniform_samples > 0;
    offsets_view_kernel<<<blocks, 256, 0, st>>>(dense ? nullptr : bg.sample_off, dense ? nullptr : bg.frame_off, so, fo,
                                                bg.n_utt, bg.uniform_samples, bg.uniform_frames, (int64_t)(mis / elem));
    bg.sample_off = so;
    bg.frame_off = fo;
    bg.uniform_samples = 0;
    bg.uniform_frames = 0;
    d_wave = reinterpret_cast<const void*>(addr - mis);
    return w;
}

// A plan's (a layout's) tables live on the device it was created on.
int check_owner_device(int owner, bool is_plan) {
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev == owner) return DSP_OK;
    return is_plan ? dsp_fail(DSP_EINVAL, "plan belongs to device %d, current device is %d", owner, dev)
                   : dsp_fail(DSP_EINVAL, "layout belongs to device %d, current device is %d", owner, dev);
}

// dense batches: the caller's frame count must be n_utt utterances of T frames
int check_dense_frames(int64_t n_frames_total, int32_t n_utt, int64_t T) {
    if (T * n_utt != n_frames_total)
        return dsp_fail(DSP_EINVAL, "n_frames_total %lld != n_utt*T (%d*%lld)", (long long)n_frames_total, n_utt, (long long)T);
    return DSP_OK;
}

size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

// The opt-in matrix-pipe kernels of dense NFFT = 512 batches: the frame-per-product form first, then the other.
// DSP_OK: launched; 1: neither took the batch; < 0: HIP error (the caller reports it).
int try_matrix_pipe(const dsp_plan* plan, const void* d_wave, int wave_dtype, const BatchGeom& bg, int delta_n,
                    float* d_out, int64_t ld_out, hipStream_t st) {
    if (mfma512t_applicable(plan, bg, wave_dtype, delta_n)) {
        const int rc = mfma512t_launch(plan, d_wave, wave_dtype, bg, delta_n, d_out, ld_out, st);
        if (rc <= 0) return rc;
    }
    if (mfma512_applicable(plan, bg, wave_dtype, delta_n)) {
        const int rc = mfma512_launch(plan, d_wave, wave_dtype, bg, delta_n, d_out, ld_out, st);
        if (rc <= 0) return rc;
    }
    return 1;
}

// ---- the delta pass: delta_tiled_kernel / delta_rows_kernel, one workgroup per DT_TILE frames of one utterance ----
static_assert(DT_TILE == (1 << DT_SHIFT), "tile tables are built with shifts");

// dynamic LDS of a workgroup: DT_TILE + 4 N input rows and DT_TILE + 2 N delta rows of D floats
size_t delta_tile_lds(int N, int D) { return ((size_t)(DT_TILE + 4 * N) + (size_t)(DT_TILE + 2 * N)) * D * sizeof(float); }

// geometry of a pass over finished rows: frames only (uniform_frames <= 0: ragged)
BatchGeom frames_geom(const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total, int64_t uniform_frames) {
    BatchGeom bg;
    memset(&bg, 0, sizeof(bg));
    bg.frame_off = d_frame_offsets;
    bg.uniform_frames = uniform_frames > 0 ? uniform_frames : 0;
    bg.total_frames = n_frames_total;
    bg.n_utt = n_utt;
    return bg;
}

// workgroups of a pass: tiles per utterance (left in `tiles`) x utterances for a uniform batch (the tile table is
// arithmetic); for a ragged one a bound on sum ceil(T_b / DT_TILE), `tiles` = 0.  The caller holds it against INT_MAX.
int64_t delta_tile_blocks(int64_t uniform_frames, int64_t n_frames_total, int32_t n_utt, int64_t* tiles) {
    *tiles = uniform_frames > 0 ? (uniform_frames + DT_TILE - 1) / DT_TILE : 0;
    return uniform_frames > 0 ? *tiles * n_utt : n_frames_total / DT_TILE + n_utt;
}

void launch_delta_tiled(int64_t blocks, hipStream_t st, const float* d_in, int64_t ld_in, const BatchGeom& bg, int32_t D,
                        int32_t N, float* d_out, int64_t ld_out, float* d_out_dd, int64_t ld_out_dd, int64_t tiles,
                        const int64_t* tile_off) {
    const size_t lds = delta_tile_lds(N, D);
    const float inv_den = dsp_delta_inv_den(N);
    if (D == 13)
        delta_tiled_kernel<13><<<(int)blocks, 256, lds, st>>>(d_in, ld_in, bg, D, N, inv_den, d_out, ld_out, d_out_dd, ld_out_dd, (int32_t)tiles, tile_off);
    else
        delta_tiled_kernel<0><<<(int)blocks, 256, lds, st>>>(d_in, ld_in, bg, D, N, inv_den, d_out, ld_out, d_out_dd, ld_out_dd, (int32_t)tiles, tile_off);
}

void launch_delta_rows(int64_t blocks, hipStream_t st, const float* cep, const BatchGeom& bg, int32_t C, int32_t N,
                       float* d_out, int64_t tiles, const int64_t* tile_off, const int64_t* seg = nullptr,
                       const double* stats = nullptr, const int32_t* tile_utt = nullptr) {
    const size_t lds = delta_tile_lds(N, C);
    const float inv_den = dsp_delta_inv_den(N);
    if (C == 13)
        delta_rows_kernel<13><<<(int)blocks, 256, lds, st>>>(cep, bg, C, N, inv_den, d_out, (int32_t)tiles, tile_off, seg, stats, tile_utt);
    else
        delta_rows_kernel<0><<<(int)blocks, 256, lds, st>>>(cep, bg, C, N, inv_den, d_out, (int32_t)tiles, tile_off, seg, stats, tile_utt);
}

int launch_generic(const dsp_plan* plan, const void* d_wave, int wave_dtype, const BatchGeom& bg,
                   int out_kind, float* d_out, int64_t ld_out, float* d_out2, hipStream_t st) {
    GenericParams P = generic_params(plan);
    // frames (waves) of a workgroup: DSP_GEN_WAVES; on the chirp-z route as many of them as fit 160 KiB of LDS
    int waves = DSP_GEN_WAVES;
    size_t lds = (size_t)DSP_GEN_WAVES * 2 * (plan->nfft / 2) * sizeof(float2);
    if (plan->route == DSP_ROUTE_CHIRP) {
        const size_t per_frame = (size_t)dsp_chirp_frame_lds(plan->conv_len, plan->K) * sizeof(float2);
        while (waves > 1 && waves * per_frame > DSP_CHIRP_LDS_MAX) --waves;
        lds = waves * per_frame;
    }
    const int grid = grid_for(bg.total_frames, waves);
    auto launch = [&](auto k) {
        if (lds > 48 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k<<<grid, 64 * waves, lds, st>>>(P, bg, d_wave, out_kind, d_out, ld_out, d_out2);
        HIP_TRY(hipGetLastError());
        return (int)DSP_OK;
    };
    return dsp_dispatch_wave(wave_dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (plan->route == DSP_ROUTE_CHIRP) return launch(features_generic_kernel<DT, DSP_ROUTE_CHIRP>);
        if (plan->route == DSP_ROUTE_MIXED) return launch(features_generic_kernel<DT, DSP_ROUTE_MIXED>);
        return launch(features_generic_kernel<DT>);
    });
}

int features_batch_impl(const dsp_plan* plan, const void* d_wave, int wave_dtype,
                        const int64_t* d_sample_offsets, const int64_t* d_frame_offsets, int32_t n_utt,
                        int64_t n_frames_total, int64_t uniform_samples, int out_kind, float* d_out,
                        int64_t ld_out, float* d_out2, void* stream, const DspRaggedTables* pre) {
    if (!plan || !d_out) return dsp_fail(DSP_EINVAL, "plan/d_out is NULL");
    int rc = check_owner_device(plan->device, true);
    if (rc != DSP_OK) return rc;
    rc = check_geom(d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples);
    if (rc != DSP_OK) return rc;
    int width;
    switch (out_kind) {
        case DSP_OUT_FRAMES: width = plan->L; break;
        case DSP_OUT_MAGSPEC:
        case DSP_OUT_POWSPEC: width = plan->K; break;
        case DSP_OUT_FBANK:
            width = plan->M;
            if (plan->M <= 0) return dsp_fail(DSP_EINVAL, "plan has no mel filterbank");
            if (!d_out2) return dsp_fail(DSP_EINVAL, "DSP_OUT_FBANK needs d_out2 (energy)");
            break;
        case DSP_OUT_MFCC:
            width = plan->C;
            if (plan->M <= 0 || plan->C <= 0) return dsp_fail(DSP_EINVAL, "plan has no mel/DCT tables");
            break;
        default: return dsp_fail(DSP_EINVAL, "unknown out_kind %d", out_kind);
    }
    if (ld_out == 0) ld_out = width;
    if (ld_out < width) return dsp_fail(DSP_EINVAL, "ld_out %lld < row width %d", (long long)ld_out, width);
    BatchGeom bg = make_geom(d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples, plan->L, plan->S);
    if (uniform_samples > 0 && (rc = check_dense_frames(n_frames_total, n_utt, bg.uniform_frames)) != DSP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (out_kind == DSP_OUT_MFCC && !g_force_generic && !pre) {
        const int mrc = try_matrix_pipe(plan, d_wave, wave_dtype, bg, 0, d_out, ld_out, st);
        if (mrc == DSP_OK) return DSP_OK;
        if (mrc < 0) return dsp_fail(mrc, "matrix-pipe MFCC kernel launch failed");
    }
    if (out_kind == DSP_OUT_MFCC && !g_force_generic && (plan->d_fast || plan->d_fast1536)) {
        BatchGeom fg = bg;
        const void* fw = d_wave;
        DspWorkspace* view = fused_kernel_view(fg, fw, wave_dtype, st);
        int frc = 1;   // 1 = no fused kernel took it
        if (fast512_applicable(plan, fg, fw, wave_dtype))
            frc = fast512_launch(plan, fw, wave_dtype, fg, d_out, ld_out, st, pre);
        else if (fast1536_applicable(plan, fg, fw, wave_dtype))
            frc = fast1536_launch(plan, fw, wave_dtype, fg, d_out, ld_out, st, pre);
        if (view && dsp_workspace_pool().release(view, st) != 0 && frc == DSP_OK) frc = DSP_EHIP;
        if (frc == DSP_OK) return DSP_OK;
        if (frc < 0) return dsp_fail(frc, "fused kernel launch failed");
    }
    return launch_generic(plan, d_wave, wave_dtype, bg, out_kind, d_out, ld_out, d_out2, st);
}

// ---- the three routes of dsp_mfcc_delta_batch.  Each returns 1 where it does not serve the batch: the next one does. ----

// Dense batches of the NFFT = 512 plans: ONE kernel writes the finished rows (kernels_fast512.h, "Fused delta").
int mfcc_delta_one_launch(const dsp_plan* plan, const void* d_wave, int wave_dtype, int32_t n_utt, int64_t n_frames_total,
                          int64_t uniform_samples, int64_t uniform_frames, int32_t delta_n, float* d_out, hipStream_t st) {
    int rc = check_owner_device(plan->device, true);
    if (rc != DSP_OK) return rc;
    rc = check_dense_frames(n_frames_total, n_utt, uniform_frames);
    if (rc != DSP_OK) return rc;
    const BatchGeom fbg = make_geom(nullptr, nullptr, n_utt, n_frames_total, uniform_samples, plan->L, plan->S);
    const int mrc = try_matrix_pipe(plan, d_wave, wave_dtype, fbg, delta_n, d_out, 3 * (int64_t)plan->C, st);
    if (mrc == DSP_OK) return DSP_OK;
    if (mrc < 0) return dsp_fail(mrc, "matrix-pipe MFCC + delta kernel launch failed");
    if (!fast512_applicable(plan, fbg, d_wave, wave_dtype)) return 1;
    const int frc = fast512_launch_fused(plan, d_wave, wave_dtype, fbg, delta_n, d_out, st);
    if (frc < 0) return dsp_fail(frc, "fused MFCC + delta kernel launch failed");
    return frc;
}

// Two passes, every byte written once as part of a full line: the MFCC kernel writes DENSE cepstra
// [sum T, C] into a pooled scratch buffer, delta_rows_kernel turns them into whole 3C-float rows.
// (Writing the 52-byte cepstra straight into the 156-byte rows cost 1.5x write amplification and a
// strided re-read.)  Scratch above 256 MiB is left to the in-place form.
int mfcc_delta_via_scratch(const dsp_plan* plan, const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                           const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total, int64_t uniform_samples,
                           int64_t uniform_frames, int32_t delta_n, float* d_out, void* stream) {
    const int C = plan->C;
    const size_t scratch_bytes = (size_t)n_frames_total * C * sizeof(float);
    if (delta_tile_lds(delta_n, C) > 64 * 1024 || scratch_bytes > ((size_t)256 << 20)) return 1;
    const bool ragged = uniform_frames <= 0;
    int64_t tiles;
    const int64_t blocks = delta_tile_blocks(uniform_frames, n_frames_total, n_utt, &tiles);
    if (blocks > 0x7fffffff) return 1;
    hipStream_t st = (hipStream_t)stream;
    // ragged: the delta tile table and the fused MFCC kernel's group tables come from ONE small launch
    const int gshift = plan->d_fast ? 3 : (plan->d_fast1536 ? 2 : 0);
    const int64_t gbound = gshift ? (n_frames_total >> gshift) + n_utt : 0;
    const size_t tile_bytes = ragged ? pad256(((size_t)n_utt + 1) * sizeof(int64_t)) : 0;
    const size_t goff_bytes = ragged && gshift ? pad256(((size_t)n_utt + 1) * sizeof(int32_t)) : 0;
    const size_t gutt_bytes = ragged && gshift ? pad256((size_t)gbound * sizeof(int32_t)) : 0;
    DspWorkspace* w = dsp_workspace_pool().acquire(tile_bytes + goff_bytes + gutt_bytes + scratch_bytes, st);
    // no scratch to be had (device memory exhausted, or `stream` is being captured into a HIP graph): the
    // in-place form needs none -- same values, 52-byte partial row writes instead of whole lines
    if (!w) return 1;
    char* wp = static_cast<char*>(w->ptr);
    int64_t* tile_off = ragged ? reinterpret_cast<int64_t*>(wp) : nullptr;
    DspRaggedTables pre;
    pre.shift = gshift;
    pre.group_off = reinterpret_cast<int32_t*>(wp + tile_bytes);
    pre.group_utt = reinterpret_cast<int32_t*>(wp + tile_bytes + goff_bytes);
    float* cep = reinterpret_cast<float*>(wp + tile_bytes + goff_bytes + gutt_bytes);
    const bool have_pre = ragged && gshift != 0 && gbound <= 0x3fffffff;
    if (have_pre) f512_build_group_tables(d_frame_offsets, n_utt, gshift, pre.group_off, pre.group_utt, st, tile_off);
    int rc = features_batch_impl(plan, d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt,
                                 n_frames_total, uniform_samples, DSP_OUT_MFCC, cep, (int64_t)C, nullptr, stream,
                                 have_pre ? &pre : nullptr);
    if (rc == DSP_OK) {
        if (ragged && !have_pre) prefix_ceil_kernel<<<1, 1024, 0, st>>>(d_frame_offsets, n_utt, DT_SHIFT, tile_off);
        launch_delta_rows(blocks, st, cep, frames_geom(d_frame_offsets, n_utt, n_frames_total, uniform_frames), C, delta_n,
                          d_out, tiles, tile_off);
        if (hipGetLastError() != hipSuccess) rc = dsp_fail(DSP_EHIP, "delta_rows_kernel launch failed");
    }
    if (dsp_workspace_pool().release(w, st) != 0 && rc == DSP_OK) rc = dsp_fail(DSP_EHIP, "workspace release failed");
    return rc;
}

// In place, no workspace: the cepstra go straight into the first C columns of the 3C-float rows, the delta pass reads
// them back from there.
int mfcc_delta_in_place(const dsp_plan* plan, const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                        const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total, int64_t uniform_samples,
                        int64_t uniform_frames, int32_t delta_n, float* d_out, void* stream) {
    const int C = plan->C;
    int rc = dsp_features_batch(plan, d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt,
                                n_frames_total, uniform_samples, DSP_OUT_MFCC, d_out, 3 * (int64_t)C, nullptr, stream);
    if (rc != DSP_OK) return rc;
    return dsp_delta_batch(d_out, 3 * (int64_t)C, d_frame_offsets, n_utt, n_frames_total, uniform_frames, C,
                           delta_n, d_out + C, 3 * (int64_t)C, d_out + 2 * C, 3 * (int64_t)C, stream);
}

int vad_features_impl(const dsp_layout* layout, const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                      const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total,
                      int64_t uniform_samples, int32_t frame_len, int32_t frame_step, int32_t use_sq,
                      double* d_amp_sum, int32_t* d_zcr, void* stream) {
    if (!d_amp_sum || !d_zcr) return dsp_fail(DSP_EINVAL, "dsp_vad_features_batch: NULL output");
    if (frame_len <= 0 || frame_step <= 0) return dsp_fail(DSP_EINVAL, "frame_len/frame_step must be > 0");
    int rc = check_geom(d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples);
    if (rc != DSP_OK) return rc;
    BatchGeom bg = make_geom(d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples, frame_len, frame_step);
    hipStream_t st = (hipStream_t)stream;
    const VadRoute route = vad_route(frame_len, frame_step, wave_dtype, use_sq, g_force_generic != 0);   // what dsp_debug_vad_route returns
    // a capacity handle (dsp_layout_create_capacity) is served from its own tables alone: a recorded call must not touch the
    // workspace pool, so what would need the shifted view or tables built on the fly is refused, never rerouted
    const bool capacity = layout != nullptr && layout->capacity != 0;
    if (route.family != DSP_VAD_ROUTE_PER_FRAME) {
        BatchGeom fg = bg;
        const void* fw = d_wave;
        DspWorkspace* view = capacity ? nullptr : fused_kernel_view(fg, fw, wave_dtype, st);
        const bool ok = vad_tile_applicable(fg, fw, wave_dtype, route.fr);
        if (capacity) {
            if (!ok) return dsp_fail(DSP_EINVAL, "capacity layout: the wave buffer must start on a %d-byte boundary and the frame bound must fit 32-bit group counters",
                                     wave_dtype == DSP_WAVE_I16 ? 8 : 16);
            const int want = route.fr == 16 ? 4 : (route.fr == 8 ? 3 : 2);
            const bool first = layout->group_off != nullptr && layout->shift == want;
            const bool second = layout->group_off2 != nullptr && want == 3;
            if (!first && !second) return dsp_fail(DSP_EINVAL, "capacity layout: no tables for %d-frame groups", route.fr);
        }
        DspRaggedTables pre;
        const bool have_pre = layout != nullptr && layout->group_off != nullptr && view == nullptr;
        if (have_pre) {
            pre.shift = layout->shift; pre.group_off = layout->group_off; pre.group_utt = layout->group_utt;
            if (layout->group_off2 != nullptr) { pre.shift2 = 3; pre.group_off2 = layout->group_off2; pre.group_utt2 = layout->group_utt2; }
        }
        if (ok) rc = vad_tile_launch(route, frame_len, frame_step, use_sq, fg, fw, wave_dtype, d_amp_sum, d_zcr, st,
                                     have_pre ? &pre : nullptr);
        if (view && dsp_workspace_pool().release(view, st) != 0 && ok && rc == DSP_OK) rc = DSP_EHIP;
        if (ok) {
            if (rc != DSP_OK) return dsp_fail(rc, "vad tile kernel launch failed");
            return DSP_OK;
        }
    }
    const int grid = grid_for(n_frames_total, 4);
    dsp_dispatch_wave(wave_dtype, [&](auto dt) {
        vad_features_kernel<decltype(dt)::value><<<grid, 256, 0, st>>>(d_wave, bg, frame_len, frame_step, use_sq, d_amp_sum, d_zcr);
    });
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

struct SegWork {
    size_t stats, tile, goff, gutt, tutt, cep, total;
};
// layout of the caller-owned work buffer of dsp_mfcc_delta_segments_batch (every part 256-byte aligned)
SegWork seg_work_layout(int32_t n_utt, int64_t n_frames_bound, int32_t C) {
    SegWork w;
    w.stats = 0;
    w.tile = w.stats + pad256((size_t)n_utt * 2 * sizeof(double));
    w.goff = w.tile + pad256(((size_t)n_utt + 1) * sizeof(int64_t));
    w.gutt = w.goff + pad256(((size_t)n_utt + 1) * sizeof(int32_t));
    w.tutt = w.gutt + pad256(((size_t)(n_frames_bound >> 2) + (size_t)n_utt) * sizeof(int32_t));   // 4-frame groups (NFFT = 1536) at most
    w.cep = w.tutt + pad256(((size_t)(n_frames_bound >> DT_SHIFT) + (size_t)n_utt) * sizeof(int32_t));
    w.total = w.cep + pad256((size_t)n_frames_bound * (size_t)C * sizeof(float));
    return w;
}

// The identity placement of the unplaced entry points: utterance b is column b of a [max_len, n_utt, width] tensor.
inline OutPlacement identity_placement(int32_t n_utt, int32_t width) { return OutPlacement{nullptr, n_utt, width, 0}; }

// The checks of a caller's placement (dsp_model_*_placed_batch) for a stream `width` floats wide; before any launch.  A
// thread under dsp_debug_host_dry_run has no device: what passed every check is refused here instead of launched.
int placement_check(const OutPlacement& pl, int32_t n_utt, int32_t width) {
    if (pl.n_cols < n_utt) return dsp_fail(DSP_EINVAL, "n_cols %d < n_utt %d", pl.n_cols, n_utt);
    if (pl.col_offset < 0) return dsp_fail(DSP_EINVAL, "col_offset %d is negative", pl.col_offset);
    if ((int64_t)pl.col_offset + width > pl.row_width)
        return dsp_fail(DSP_EINVAL, "col_offset %d + %d columns do not fit row_width %d", pl.col_offset, width, pl.row_width);
    return dsp_refuse_dry_run(nullptr);
}

// The argument checks the model-finalize entry points share (behind their own), and the launch.  pl.row_width == 0: the
// identity placement at this stream's own width.
int model_finalize_impl(const float* d_mfcc, int64_t ld_in, const int64_t* d_frame_offsets, int32_t n_utt, int32_t C,
                        int32_t N, int32_t max_len, float* d_out, int32_t* d_len0, const int64_t* d_segments,
                        const double* d_stats, OutPlacement pl, void* stream) {
    if (N < 1) return dsp_fail(DSP_EINVAL, "N must be an integer >= 1");  // base.py:71-72
    if (C <= 0 || C > 32 || max_len <= 0) return dsp_fail(DSP_EINVAL, "need 0 < C <= 32 and max_len > 0");
    if (ld_in == 0) ld_in = C;
    if (ld_in < C) return dsp_fail(DSP_EINVAL, "ld_in %lld < C %d", (long long)ld_in, C);
    const size_t lds = ((size_t)(max_len + 2 * N) + (size_t)(max_len + N)) * C * sizeof(float);
    if (lds > 64 * 1024) return dsp_fail(DSP_EINVAL, "max_len * C too large for the LDS tile (%zu bytes)", lds);
    int rc;
    if (pl.row_width == 0) pl.row_width = 3 * C;                      // the unplaced entry points: rows of this stream alone
    else if ((rc = placement_check(pl, n_utt, 3 * C)) != DSP_OK) return rc;
    model_finalize_kernel<<<n_utt, 256, lds, (hipStream_t)stream>>>(d_mfcc, ld_in, d_frame_offsets, n_utt, C, N, max_len,
                                                                   d_out, d_len0, pl, d_segments, d_stats);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

// The same for the two endpoint-rule entry points (d_voiced: the autocorrelation gate's verdicts, or NULL).
int endpoint_rule_impl(const double* d_amp_sum, const int32_t* d_zcr, const uint8_t* d_voiced, const int64_t* d_frame_offsets,
                       int32_t n_utt, int32_t frame_len, double cfg_frame, double cfg_step, int32_t* d_endpoints,
                       void* stream) {
    if (!(cfg_frame > 0.0) || !(cfg_step > 0.0)) return dsp_fail(DSP_EINVAL, "cfg.frame / cfg.step must be > 0");
    if (2 * (int)(0.100 / cfg_step) > DSP_MAX_SIL)
        return dsp_fail(DSP_EINVAL, "cfg.step %g gives a silence window > %d frames", cfg_step, DSP_MAX_SIL);
    endpoint_rule_kernel<<<n_utt, 64, 0, (hipStream_t)stream>>>(
        d_amp_sum, d_zcr, d_frame_offsets, n_utt, frame_len, cfg_frame, cfg_step, d_endpoints, d_voiced);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

// what both endpoint-layout entry points ask of their shared arguments
bool endpoint_layout_args_ok(const int32_t* d_endpoints, const int64_t* d_sample_offsets, const int64_t* d_segments,
                             const int64_t* d_dst_offsets, const int64_t* d_frame_offsets, int32_t n_utt) {
    return d_endpoints && d_sample_offsets && d_segments && d_dst_offsets && d_frame_offsets && n_utt > 0;
}

// The cepstrum kernels are instantiated for power-of-two frame lengths in [128, 1024]: f(std::integral_constant<int, L>).
bool cepstrum_frame_len_ok(int32_t frame_len) {
    return frame_len >= 128 && frame_len <= 1024 && (frame_len & (frame_len - 1)) == 0;
}
template <class F>
void dispatch_cepstrum_frame_len(int32_t frame_len, F&& f) {
    switch (frame_len) {
        case 128: f(std::integral_constant<int, 128>{}); break;
        case 256: f(std::integral_constant<int, 256>{}); break;
        case 512: f(std::integral_constant<int, 512>{}); break;
        default: f(std::integral_constant<int, 1024>{}); break;
    }
}

// pitch_scores_kernel_v2 is instantiated for W = 3 and 4 outputs per lane and half: f(std::integral_constant<int, W>).
template <class F>
void dispatch_pitch_v2_width(int W, F&& f) {
    if (W == 3) f(std::integral_constant<int, 3>{}); else f(std::integral_constant<int, 4>{});
}

// diagnostic builds only: sums a kernel's per-phase shader-clock stamps (`sym`: [slots][n_stamp] on the device) over the
// slots into out[0 .. min(n, n_stamp)) and zeroes them
template <class Sym>
int read_stamps(const Sym& sym, int n_stamp, int slots, unsigned long long* out, int n) {
    std::vector<unsigned int> h((size_t)n_stamp * slots);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(sym), h.size() * 4));
    for (int i = 0; i < n && i < n_stamp; ++i) {
        out[i] = 0;
        for (int w = 0; w < slots; ++w) out[i] += h[(size_t)w * n_stamp + i];
    }
    h.assign(h.size(), 0u);
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(sym), h.data(), h.size() * 4));
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_abi_version(void) { return DSP_ABI_VERSION; }

int dsp_debug_force_generic(int on) {
    g_force_generic = on ? 1 : 0;
    return DSP_OK;
}

int dsp_debug_vad_route(int32_t frame_len, int32_t frame_step, int wave_dtype, int32_t use_sq, int32_t* frames_per_wave) {
    if (frame_len <= 0 || frame_step <= 0) return dsp_fail(DSP_EINVAL, "frame_len/frame_step must be > 0");
    if (wave_dtype != DSP_WAVE_F32 && wave_dtype != DSP_WAVE_I16) return dsp_fail(DSP_EINVAL, "dsp_debug_vad_route: unknown wave_dtype %d", wave_dtype);
    const VadRoute route = vad_route(frame_len, frame_step, wave_dtype, use_sq, g_force_generic != 0);   // what vad_features_impl switches on
    if (frames_per_wave) *frames_per_wave = route.fr;
    return route.family;
}

int dsp_debug_host_dry_run(int on) {
    g_host_dry_run = on ? 1 : 0;
    return DSP_OK;
}

int dsp_debug_use_mfma512(int on) {
    g_use_mfma512 = on < 0 ? -1 : (on > 2 ? 1 : on);
    return DSP_OK;
}

int dsp_plan_has_mfma512(const dsp_plan* plan) { return plan ? (plan->d_mfma ? 1 : 0) | (plan->d_mfmat ? 2 : 0) : 0; }

int dsp_debug_pool_stats(long long* n_buffers, long long* bytes) {
    dsp_workspace_pool().stats(n_buffers, bytes);
    return DSP_OK;
}

// diagnostic builds only (not declared in the public header): per-phase shader-clock sums of mfcc512_kernel,
// mfcc512t_kernel and mfcc512m_kernel
#ifdef F512_STAMPS
int dsp_debug_read_stamps(unsigned long long* out, int n) { return read_stamps(f512_stamp_sum, F512_NSTAMP, 8192, out, n); }
#endif
#ifdef M512T_STAMPS
int dsp_debug_read_stamps_m512t(unsigned long long* out, int n) { return read_stamps(m512t_stamp_sum, M512T_NSTAMP, 4096, out, n); }
#endif
#ifdef M512_STAMPS
int dsp_debug_read_stamps_m512(unsigned long long* out, int n) { return read_stamps(m512_stamp_sum, M512_NSTAMP, 2048, out, n); }
#endif

int dsp_plan_has_fast_path(const dsp_plan* plan) { return plan && (plan->d_fast || plan->d_fast1536) ? 1 : 0; }

const char* dsp_last_error(void) { return g_err.c_str(); }

int dsp_device_count(int* n) {
    if (!n) return dsp_fail(DSP_EINVAL, "n is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return dsp_fail(DSP_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n = c;
    return DSP_OK;
}

int dsp_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return DSP_OK;
}

int dsp_get_device(int* device) {
    if (!device) return dsp_fail(DSP_EINVAL, "dsp_get_device: NULL argument");
    HIP_TRY(hipGetDevice(device));
    return DSP_OK;
}

int dsp_malloc(void** d_ptr, size_t bytes) {
    if (!d_ptr) return dsp_fail(DSP_EINVAL, "d_ptr is NULL");
    HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 1));
    return DSP_OK;
}

int dsp_free(void* d_ptr) {
    if (d_ptr) HIP_TRY(hipFree(d_ptr));
    return DSP_OK;
}

int dsp_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return DSP_OK;
}

int dsp_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return DSP_OK;
}

int dsp_memset(void* d_dst, int value, size_t bytes, void* stream) {
    HIP_TRY(hipMemsetAsync(d_dst, value, bytes, (hipStream_t)stream));
    return DSP_OK;
}

int dsp_stream_synchronize(void* stream) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return DSP_OK;
}

int dsp_frame_count(int64_t n_samples, int32_t frame_len, int32_t frame_step, int64_t* n_frames) {
    if (!n_frames || frame_len <= 0 || frame_step <= 0 || n_samples < 0)
        return dsp_fail(DSP_EINVAL, "dsp_frame_count: bad arguments");
    if (n_samples <= frame_len) *n_frames = 1;
    else *n_frames = 1 + (n_samples - frame_len + frame_step - 1) / frame_step;
    return DSP_OK;
}

int dsp_frame_offsets(const int64_t* h_sample_offsets, int32_t n_utt, int32_t frame_len,
                      int32_t frame_step, int64_t* h_frame_offsets) {
    if (!h_sample_offsets || !h_frame_offsets || n_utt < 0)
        return dsp_fail(DSP_EINVAL, "dsp_frame_offsets: bad arguments");
    h_frame_offsets[0] = 0;
    for (int32_t b = 0; b < n_utt; ++b) {
        int64_t T;
        const int64_t n = h_sample_offsets[b + 1] - h_sample_offsets[b];
        if (n < 0) return dsp_fail(DSP_EINVAL, "sample_offsets not monotone at %d", b);
        int rc = dsp_frame_count(n, frame_len, frame_step, &T);
        if (rc != DSP_OK) return rc;
        h_frame_offsets[b + 1] = h_frame_offsets[b] + T;
    }
    return DSP_OK;
}

int dsp_plan_create(const dsp_plan_desc* d, dsp_plan** out) { return dsp_plan_create_ex(d, 0, out); }

int dsp_plan_create_ex(const dsp_plan_desc* d, uint32_t flags, dsp_plan** out) {
    if (!d || !out) return dsp_fail(DSP_EINVAL, "NULL desc/out");
    *out = nullptr;
    if (flags & ~(uint32_t)DSP_PLAN_ANY_NFFT) return dsp_fail(DSP_EINVAL, "unknown plan flags 0x%x", flags);
    if (d->frame_len <= 0 || d->frame_step <= 0) return dsp_fail(DSP_EINVAL, "frame_len/frame_step must be > 0");
    if ((flags & DSP_PLAN_ANY_NFFT) && (d->nfft < 16 || d->nfft > 4096))
        return dsp_fail(DSP_EINVAL, "unsupported nfft %d (need 16 <= nfft <= 4096)", d->nfft);
    if (!(flags & DSP_PLAN_ANY_NFFT) && (d->nfft < 16 || d->nfft > 4096 || !is_pow2_or_3pow2(d->nfft)))
        return dsp_fail(DSP_EINVAL, "unsupported nfft %d (need 2^k or 3*2^k in [16, 4096])", d->nfft);
    // the transform: the pass list of the 17 sizes, mixed radix for the other even sizes with a 5-smooth half, chirp-z for the rest
    std::vector<int> radix;
    int route = DSP_ROUTE_PASSES, conv_len = 0;
    const int lfft_ = d->frame_len < d->nfft ? d->frame_len : d->nfft;
    if (is_pow2_or_3pow2(d->nfft)) {
        factor_half_fft(d->nfft / 2, radix);
    } else if (!(d->nfft & 1) && factor_half_fft(d->nfft / 2, radix)) {
        route = DSP_ROUTE_MIXED;
    } else {
        route = DSP_ROUTE_CHIRP;
        conv_len = chirp_conv_len(lfft_ + d->nfft / 2);      // lfft + K - 1
        factor_half_fft(conv_len, radix);
    }
    if (!d->h_window) return dsp_fail(DSP_EINVAL, "h_window is NULL");
    if (d->nfilt > 0 && !d->h_window64) return dsp_fail(DSP_EINVAL, "h_window64 is NULL");
    if (d->nfilt > 0 && (float)d->preemph64 != d->preemph) return dsp_fail(DSP_EINVAL, "preemph64 does not round to preemph");
    if (d->nfilt < 0 || d->numcep < 0 || d->numcep > d->nfilt)
        return dsp_fail(DSP_EINVAL, "need 0 <= numcep <= nfilt (got %d, %d)", d->numcep, d->nfilt);
    if (d->nfilt > d->nfft) return dsp_fail(DSP_EINVAL, "nfilt %d > nfft %d", d->nfilt, d->nfft);
    const int K = d->nfft / 2 + 1;
    std::vector<int32_t> off(d->nfilt > 0 ? d->nfilt : 1, 0);
    int64_t nnz = 0;
    if (d->nfilt > 0) {
        if (!d->h_mel_start || !d->h_mel_count || !d->h_mel_weights)
            return dsp_fail(DSP_EINVAL, "mel tables missing");
        if (d->numcep > 0 && !d->h_dct) return dsp_fail(DSP_EINVAL, "h_dct is NULL");
        for (int j = 0; j < d->nfilt; ++j) {
            if (d->h_mel_count[j] < 0 || d->h_mel_start[j] < 0 || d->h_mel_start[j] + d->h_mel_count[j] > K)
                return dsp_fail(DSP_EINVAL, "mel filter %d spans bins outside [0,%d)", j, K);
            off[j] = (int32_t)nnz;
            nnz += d->h_mel_count[j];
        }
    }
    int dev = 0;
    if (!g_host_dry_run) HIP_TRY(hipGetDevice(&dev));
    dsp_plan* p = new dsp_plan();
    memset(p, 0, sizeof(*p));
    p->dry_run = g_host_dry_run ? 1 : 0;
    if (p->dry_run) dev = -1;      // no device owns these tables: every launch path that checks the plan's device refuses
    p->L = d->frame_len; p->S = d->frame_step; p->nfft = d->nfft; p->K = K;
    p->M = d->nfilt; p->C = d->numcep; p->append_energy = d->append_energy ? 1 : 0;
    p->lfft = d->frame_len < d->nfft ? d->frame_len : d->nfft;
    p->preemph = d->preemph; p->mel_nnz = (int32_t)nnz; p->device = dev;
    p->route = route; p->conv_len = conv_len; p->n_pass = (int32_t)radix.size();
    for (size_t i = 0; i < radix.size(); ++i) p->radix[i] = radix[i];
    std::vector<float2> tw(d->nfft);
    for (int k = 0; k < d->nfft; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)d->nfft;
        tw[k] = make_float2((float)cos(a), (float)sin(a));
    }
    int rc = DSP_OK;
    if (rc == DSP_OK) rc = upload(&p->d_window, d->h_window, (size_t)d->frame_len);
    if (rc == DSP_OK) rc = upload(&p->d_twiddle, tw.data(), tw.size());
    if (rc == DSP_OK && route == DSP_ROUTE_CHIRP) {
        std::vector<float2> cw, cspec, ctw;
        chirp_tables(p->nfft, p->lfft, K, conv_len, radix, cw, cspec, ctw);
        // host copies for dsp_debug_plan_transform_tables
        p->h_cz_w = static_cast<float2*>(malloc(cw.size() * sizeof(float2)));
        p->h_cz_spec = static_cast<float2*>(malloc(cspec.size() * sizeof(float2)));
        if (!p->h_cz_w || !p->h_cz_spec) rc = dsp_fail(DSP_EHIP, "out of host memory");
        if (rc == DSP_OK) {
            memcpy(p->h_cz_w, cw.data(), cw.size() * sizeof(float2));
            memcpy(p->h_cz_spec, cspec.data(), cspec.size() * sizeof(float2));
            rc = upload(&p->d_cz_w, cw.data(), cw.size());
        }
        if (rc == DSP_OK) rc = upload(&p->d_cz_spec, cspec.data(), cspec.size());
        if (rc == DSP_OK) rc = upload(&p->d_cz_tw, ctw.data(), ctw.size());
    }
    if (rc == DSP_OK && d->nfilt > 0) {
        rc = upload(&p->d_mel_start, d->h_mel_start, (size_t)d->nfilt);
        if (rc == DSP_OK) rc = upload(&p->d_mel_count, d->h_mel_count, (size_t)d->nfilt);
        if (rc == DSP_OK) rc = upload(&p->d_mel_off, off.data(), (size_t)d->nfilt);
        if (rc == DSP_OK) rc = upload(&p->d_mel_w, d->h_mel_weights, (size_t)nnz);
        if (rc == DSP_OK && d->numcep > 0) rc = upload(&p->d_dct, d->h_dct, (size_t)d->numcep * d->nfilt);
    }
    if (rc == DSP_OK && d->nfilt > 0) {
        // the fp64 side of the plan (kernels_repair.h): window and coefficient as the caller has them in fp64, and an
        // exact twiddle table
        std::vector<double> tw64((size_t)2 * d->nfft);
        for (int k = 0; k < d->nfft; ++k) {
            const double a = 2.0 * M_PI * (double)k / (double)d->nfft;
            tw64[2 * k] = cos(a);
            tw64[2 * k + 1] = sin(a);
        }
        rc = upload(&p->d_window64, d->h_window64, (size_t)p->lfft);
        if (rc == DSP_OK) rc = upload(&p->d_twiddle64, tw64.data(), tw64.size());
        if (rc == DSP_OK) {
            DspRepairTab t;
            memset(&t, 0, sizeof(t));
            t.preemph = d->preemph64; t.lfft = p->lfft; t.nfft = p->nfft;
            t.window = p->d_window64; t.tw = p->d_twiddle64;
            t.mel_start = p->d_mel_start; t.mel_count = p->d_mel_count; t.mel_off = p->d_mel_off; t.mel_w = p->d_mel_w;
            DspRepairTab* dt = nullptr;
            rc = upload(&dt, &t, 1);
            p->d_repair = dt;
        }
    }
    if (rc == DSP_OK) rc = fast512_plan_init(p, d, off.data());
    if (rc == DSP_OK && d->nfilt > 0 && d->numcep > 0) rc = fast1536_plan_init(p, d, off.data());
    if (rc == DSP_OK && d->nfilt > 0 && d->numcep > 0 && p->d_fast) rc = mfma512_plan_init(p, d);
    if (rc == DSP_OK && d->nfilt > 0 && d->numcep > 0 && p->d_fast) rc = mfma512t_plan_init(p, d);
    if (rc != DSP_OK) { dsp_plan_destroy(p); return rc; }
    *out = p;
    return DSP_OK;
}

int dsp_plan_transform(const dsp_plan* plan, int32_t* route, int32_t* conv_len) {
    if (!plan || !route || !conv_len) return dsp_fail(DSP_EINVAL, "dsp_plan_transform: NULL argument");
    *route = plan->route;
    *conv_len = plan->conv_len;
    return DSP_OK;
}

int dsp_debug_plan_transform_tables(const dsp_plan* plan, int32_t* radix, int32_t radix_cap, int32_t* n_pass, float* h_chirp,
                                    float* h_chirp_spec) {
    if (!plan || !radix || !n_pass) return dsp_fail(DSP_EINVAL, "dsp_debug_plan_transform_tables: NULL argument");
    if (radix_cap < plan->n_pass) return dsp_fail(DSP_EINVAL, "radix_cap %d < %d passes", radix_cap, plan->n_pass);
    *n_pass = plan->n_pass;
    for (int i = 0; i < plan->n_pass; ++i) radix[i] = plan->radix[i];
    if (plan->route == DSP_ROUTE_CHIRP) {
        if (h_chirp) memcpy(h_chirp, plan->h_cz_w, (size_t)plan->nfft * sizeof(float2));
        if (h_chirp_spec) memcpy(h_chirp_spec, plan->h_cz_spec, (size_t)plan->conv_len * sizeof(float2));
    }
    return DSP_OK;
}

int dsp_plan_destroy(dsp_plan* p) {
    if (!p) return DSP_OK;
    void* bufs[] = {p->d_window, p->d_twiddle, p->d_mel_start, p->d_mel_count, p->d_mel_off, p->d_mel_w, p->d_dct,
                    p->d_window64, p->d_twiddle64, p->d_repair, p->d_cz_w, p->d_cz_spec, p->d_cz_tw};
    for (void* b : bufs) dsp_table_free(b, p->dry_run);
    free(p->h_cz_w);
    free(p->h_cz_spec);
    fast512_plan_free(p);
    fast1536_plan_free(p);
    mfma512_plan_free(p);
    mfma512t_plan_free(p);
    delete p;
    return DSP_OK;
}

int dsp_preemphasis_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                          int32_t n_utt, int64_t n_samples_total, float coeff, float* d_out, void* stream) {
    if (!d_wave || !d_out || !d_sample_offsets || n_utt <= 0 || n_samples_total <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_preemphasis_batch: bad arguments");
    if (wave_dtype != DSP_WAVE_I16 && wave_dtype != DSP_WAVE_F32) return dsp_fail(DSP_EINVAL, "unsupported wave_dtype %d", wave_dtype);
    const int grid = grid_for(n_samples_total, 256);
    dsp_dispatch_wave(wave_dtype, [&](auto dt) {
        preemphasis_kernel<decltype(dt)::value><<<grid, 256, 0, (hipStream_t)stream>>>(d_wave, d_sample_offsets, n_utt, n_samples_total, coeff, d_out);
    });
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_features_batch(const dsp_plan* plan, const void* d_wave, int wave_dtype,
                       const int64_t* d_sample_offsets, const int64_t* d_frame_offsets, int32_t n_utt,
                       int64_t n_frames_total, int64_t uniform_samples, int out_kind, float* d_out,
                       int64_t ld_out, float* d_out2, void* stream) {
    return features_batch_impl(plan, d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total,
                               uniform_samples, out_kind, d_out, ld_out, d_out2, stream, nullptr);
}

int dsp_delta_batch(const float* d_in, int64_t ld_in, const int64_t* d_frame_offsets, int32_t n_utt,
                    int64_t n_frames_total, int64_t uniform_frames, int32_t D, int32_t N, float* d_out,
                    int64_t ld_out, float* d_out_dd, int64_t ld_out_dd, void* stream) {
    if (!d_in || !d_out) return dsp_fail(DSP_EINVAL, "dsp_delta_batch: NULL buffer");
    if (N < 1) return dsp_fail(DSP_EINVAL, "N must be an integer >= 1");  // base.py:71-72
    if (D <= 0 || n_utt <= 0 || n_frames_total <= 0) return dsp_fail(DSP_EINVAL, "dsp_delta_batch: empty input");
    if (uniform_frames <= 0 && !d_frame_offsets) return dsp_fail(DSP_EINVAL, "ragged batch needs d_frame_offsets");
    if (ld_in == 0) ld_in = D;
    if (ld_out == 0) ld_out = D;
    if (ld_out_dd == 0) ld_out_dd = D;
    const BatchGeom bg = frames_geom(d_frame_offsets, n_utt, n_frames_total, uniform_frames);
    hipStream_t st = (hipStream_t)stream;
    const bool strides_ok = ld_in <= 0x7fffff && ld_out <= 0x7fffff && ld_out_dd <= 0x7fffff;
    int64_t tiles;
    const int64_t blocks = delta_tile_blocks(uniform_frames, n_frames_total, n_utt, &tiles);
    // tiled LDS kernel where a tile fits (the tile table of a uniform batch is arithmetic); per-element kernel otherwise
    if (uniform_frames > 0 && delta_tile_lds(N, D) <= 64 * 1024) {
        if (blocks > 0x7fffffff) return dsp_fail(DSP_EINVAL, "too many delta tiles");
        if (!strides_ok) return dsp_fail(DSP_EINVAL, "row stride too large");
        launch_delta_tiled(blocks, st, d_in, ld_in, bg, D, N, d_out, ld_out, d_out_dd, ld_out_dd, tiles, nullptr);
    } else if (uniform_frames <= 0 && delta_tile_lds(N, D) <= 64 * 1024 && strides_ok) {
        // ragged: per-utterance tile prefix in a pooled, event-guarded workspace, grid sized by a bound
        if (blocks > 0x7fffffff) return dsp_fail(DSP_EINVAL, "too many delta tiles");
        DspWorkspace* w = dsp_workspace_pool().acquire(((size_t)n_utt + 1) * sizeof(int64_t), st);
        if (!w) return dsp_fail(DSP_EHIP, "workspace allocation failed");
        int64_t* tile_off = static_cast<int64_t*>(w->ptr);
        prefix_ceil_kernel<<<1, 1024, 0, st>>>(d_frame_offsets, n_utt, DT_SHIFT, tile_off);
        launch_delta_tiled(blocks, st, d_in, ld_in, bg, D, N, d_out, ld_out, d_out_dd, ld_out_dd, 0, tile_off);
        if (dsp_workspace_pool().release(w, st) != 0) return dsp_fail(DSP_EHIP, "workspace release failed");
    } else {
        delta_kernel<<<grid_for(n_frames_total * D, 256), 256, 0, st>>>(
            d_in, ld_in, bg, D, N, dsp_delta_inv_den(N), d_out, ld_out, d_out_dd, ld_out_dd);
    }
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_mfcc_delta_batch(const dsp_plan* plan, const void* d_wave, int wave_dtype,
                         const int64_t* d_sample_offsets, const int64_t* d_frame_offsets, int32_t n_utt,
                         int64_t n_frames_total, int64_t uniform_samples, int32_t delta_n, float* d_out,
                         void* stream) {
    if (!plan) return dsp_fail(DSP_EINVAL, "plan is NULL");
    if (delta_n < 1) return dsp_fail(DSP_EINVAL, "N must be an integer >= 1");  // base.py:71-72
#ifdef DSP_WS_MALLOC_ASYNC
    dsp_ws_diag_stream() = (hipStream_t)stream;
#endif
    const int C = plan->C;
    if (C <= 0) return dsp_fail(DSP_EINVAL, "plan has no mel/DCT tables");
    if (!d_out) return dsp_fail(DSP_EINVAL, "plan/d_out is NULL");
    {   // validate before the first launch or workspace acquire (the table kernels read the offset arrays)
        const int grc = check_geom(d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples);
        if (grc != DSP_OK) return grc;
    }
    int64_t uniform_frames = 0;
    if (uniform_samples > 0) dsp_frame_count(uniform_samples, plan->L, plan->S, &uniform_frames);
    hipStream_t st = (hipStream_t)stream;
    if (uniform_samples > 0 && !g_force_generic && plan->d_fast) {
        const int rc = mfcc_delta_one_launch(plan, d_wave, wave_dtype, n_utt, n_frames_total, uniform_samples, uniform_frames,
                                             delta_n, d_out, st);
        if (rc != 1) return rc;
    }
    const int rc = mfcc_delta_via_scratch(plan, d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total,
                                          uniform_samples, uniform_frames, delta_n, d_out, stream);
    if (rc != 1) return rc;
    return mfcc_delta_in_place(plan, d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total,
                               uniform_samples, uniform_frames, delta_n, d_out, stream);
}

int dsp_scale_columns(float* d_x, int64_t rows, int32_t cols, const float* d_scale, void* stream) {
    if (!d_x || !d_scale || rows <= 0 || cols <= 0) return dsp_fail(DSP_EINVAL, "dsp_scale_columns: bad arguments");
    scale_columns_kernel<<<grid_for(rows * cols, 256), 256, 0, (hipStream_t)stream>>>(d_x, rows, cols, d_scale);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_layout_create(const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total, int32_t frame_len,
                      int32_t frame_step, void* stream, dsp_layout** out) {
    if (!out) return dsp_fail(DSP_EINVAL, "dsp_layout_create: out is NULL");
    *out = nullptr;
    if (!d_frame_offsets || n_utt <= 0 || n_frames_total <= 0 || frame_len <= 0 || frame_step <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_layout_create: bad arguments");
    // the group sizes vad_route can answer for this framing: fp32 callers (and x^2) take `tile` frames per wave, int16 sums of |x|
    // `tile` or eight (the handle serves every thread: dsp_debug_force_generic is not consulted, a forced call ignores the tables)
    const VadRoute r32 = vad_route(frame_len, frame_step, DSP_WAVE_F32, 0, false);
    const int tile = r32.family == DSP_VAD_ROUTE_PER_FRAME ? 0 : r32.fr;
    dsp_layout* l = new dsp_layout();
    memset(l, 0, sizeof(*l));
    l->n_utt = n_utt; l->frame_len = frame_len; l->frame_step = frame_step; l->n_frames_total = n_frames_total;
    if (hipGetDevice(&l->device) != hipSuccess) { delete l; return dsp_fail(DSP_EHIP, "dsp_layout_create: hipGetDevice failed"); }
    if (tile != 0) {
        l->shift = tile == 16 ? 4 : 2;
        const int64_t bound = n_frames_total / tile + n_utt;
        if (bound > 0x3fffffff) { delete l; return dsp_fail(DSP_EINVAL, "dsp_layout_create: batch too large"); }
        const bool second = vad_route(frame_len, frame_step, DSP_WAVE_I16, 0, false).fr == 8;      // int16 callers take 8-frame groups
        const int64_t bound2 = second ? n_frames_total / 8 + n_utt : 0;
        const size_t n1 = (size_t)n_utt + 1 + (size_t)bound, n2 = second ? (size_t)n_utt + 1 + (size_t)bound2 : 0;
        if (hipMalloc(reinterpret_cast<void**>(&l->group_off), (n1 + n2) * sizeof(int32_t)) != hipSuccess) {
            delete l;
            return dsp_fail(DSP_EHIP, "dsp_layout_create: allocation failed");
        }
        l->group_utt = l->group_off + n_utt + 1;
        f512_build_group_tables(d_frame_offsets, n_utt, l->shift, l->group_off, l->group_utt, (hipStream_t)stream);
        if (second) {
            l->group_off2 = l->group_off + n1;
            l->group_utt2 = l->group_off2 + n_utt + 1;
            f512_build_group_tables(d_frame_offsets, n_utt, 3, l->group_off2, l->group_utt2, (hipStream_t)stream);
        }
        if (hipGetLastError() != hipSuccess) { (void)hipFree(l->group_off); delete l; return dsp_fail(DSP_EHIP, "dsp_layout_create: launch failed"); }
    }
    *out = l;
    return DSP_OK;
}

int dsp_layout_destroy(dsp_layout* layout) {
    if (!layout) return DSP_OK;
    dsp_table_free(layout->group_off, layout->dry_run);
    delete layout;
    return DSP_OK;
}

int dsp_frames_bound(int64_t sample_capacity, int32_t n_utt, int32_t frame_len, int32_t frame_step, int64_t* n_frames_bound) {
    if (!n_frames_bound) return dsp_fail(DSP_EINVAL, "dsp_frames_bound: n_frames_bound is NULL");
    if (sample_capacity < 0 || n_utt <= 0 || frame_len <= 0 || frame_step <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_frames_bound: need sample_capacity >= 0, n_utt > 0, frame_len > 0, frame_step > 0");
    // T(n) = 1 for n <= L, else 1 + ceil((n - L) / S).  L >= S: ceil((n - L) / S) <= ceil((n - S) / S) = ceil(n / S) - 1, so
    // T(n) <= ceil(n / S) <= n / S + 1 (integer division).  Any L: ceil((n - L) / S) <= ceil(n / S), so T(n) <= n / S + 2.
    // And sum_b (n_b / S) <= (sum_b n_b) / S <= sample_capacity / S.
    const int64_t per_clip = frame_len >= frame_step ? 1 : 2;
    if (sample_capacity / frame_step > INT64_MAX - per_clip * n_utt) return dsp_fail(DSP_EINVAL, "dsp_frames_bound: the bound overflows int64");
    *n_frames_bound = sample_capacity / frame_step + per_clip * n_utt;
    return DSP_OK;
}

int dsp_batch_offsets_batch(const int64_t* d_sample_offsets_in, int32_t n_utt, int64_t sample_capacity, int32_t n_framings,
                            const int32_t* frame_len, const int32_t* frame_step, int64_t* d_sample_offsets,
                            int64_t* const* d_frame_offsets, int32_t* d_status, void* stream) {
    if (!d_sample_offsets_in || !d_sample_offsets || !d_status) return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: NULL argument");
    if (n_utt <= 0) return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: n_utt %d must be >= 1", n_utt);
    if (sample_capacity <= 0) return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: sample_capacity %lld must be >= 1", (long long)sample_capacity);
    if (n_framings < 0 || n_framings > DSP_MAX_FRAMINGS)
        return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: n_framings %d must be in [0, %d]", n_framings, DSP_MAX_FRAMINGS);
    if (n_framings > 0 && (!frame_len || !frame_step || !d_frame_offsets)) return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: NULL argument");
    if (d_sample_offsets == d_sample_offsets_in) return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: the sanitised table must not be the caller's (overlap)");
    BatchOffsetsArgs A;
    memset(&A, 0, sizeof(A));
    A.n_framings = n_framings;
    for (int f = 0; f < n_framings; ++f) {
        if (frame_len[f] <= 0 || frame_step[f] <= 0)
            return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: framing %d: frame_len %d and frame_step %d must be > 0", f, frame_len[f], frame_step[f]);
        if (!d_frame_offsets[f]) return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: framing %d: NULL frame offsets", f);
        if (d_frame_offsets[f] == d_sample_offsets || d_frame_offsets[f] == d_sample_offsets_in)
            return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: framing %d: the frame offsets overlap a sample table", f);
        for (int g = 0; g < f; ++g)
            if (d_frame_offsets[g] == d_frame_offsets[f]) return dsp_fail(DSP_EINVAL, "dsp_batch_offsets_batch: framings %d and %d share a table (overlap)", g, f);
        A.L[f] = frame_len[f]; A.S[f] = frame_step[f]; A.frame_off[f] = d_frame_offsets[f];
    }
    if (int rc = dsp_refuse_dry_run("dsp_batch_offsets_batch")) return rc;
    batch_offsets_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(d_sample_offsets_in, n_utt, sample_capacity, A, d_sample_offsets, d_status);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_layout_create_capacity(int32_t n_utt, int64_t n_frames_bound, int32_t frame_len, int32_t frame_step, dsp_layout** out) {
    if (!out) return dsp_fail(DSP_EINVAL, "dsp_layout_create_capacity: out is NULL");
    *out = nullptr;
    if (n_utt <= 0 || n_frames_bound <= 0 || frame_len <= 0 || frame_step <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_layout_create_capacity: need n_utt > 0, n_frames_bound > 0, frame_len > 0, frame_step > 0");
    if (n_frames_bound < n_utt) return dsp_fail(DSP_EINVAL, "dsp_layout_create_capacity: n_frames_bound %lld is below one frame per clip (%d)", (long long)n_frames_bound, n_utt);
    const VadRoute r32 = vad_route(frame_len, frame_step, DSP_WAVE_F32, 0, false);       // as dsp_layout_create
    const int tile = r32.family == DSP_VAD_ROUTE_PER_FRAME ? 0 : r32.fr;
    const bool second = tile != 0 && vad_route(frame_len, frame_step, DSP_WAVE_I16, 0, false).fr == 8;
    const int64_t bound = tile ? n_frames_bound / tile + n_utt : 0, bound2 = second ? n_frames_bound / 8 + n_utt : 0;
    if (bound > 0x3fffffff || bound2 > 0x3fffffff) return dsp_fail(DSP_EINVAL, "dsp_layout_create_capacity: batch too large");
    dsp_layout* l = new dsp_layout();
    memset(l, 0, sizeof(*l));
    l->n_utt = n_utt; l->frame_len = frame_len; l->frame_step = frame_step; l->n_frames_total = n_frames_bound;
    l->capacity = 1;
    l->dry_run = g_host_dry_run ? 1 : 0;
    l->device = -1;
    if (!l->dry_run && hipGetDevice(&l->device) != hipSuccess) { delete l; return dsp_fail(DSP_EHIP, "dsp_layout_create_capacity: hipGetDevice failed"); }
    if (tile != 0) {
        l->shift = tile == 16 ? 4 : 2;
        const size_t n1 = (size_t)n_utt + 1 + (size_t)bound, n2 = second ? (size_t)n_utt + 1 + (size_t)bound2 : 0;
        void* mem = nullptr;
        if (l->dry_run) mem = malloc((n1 + n2) * sizeof(int32_t));
        else if (hipMalloc(&mem, (n1 + n2) * sizeof(int32_t)) != hipSuccess) mem = nullptr;
        if (!mem) { delete l; return dsp_fail(DSP_EHIP, "dsp_layout_create_capacity: allocation failed"); }
        l->group_off = static_cast<int32_t*>(mem);
        l->group_utt = l->group_off + n_utt + 1;
        if (second) {
            l->group_off2 = l->group_off + n1;
            l->group_utt2 = l->group_off2 + n_utt + 1;
        }
    }
    *out = l;
    return DSP_OK;
}

int dsp_layout_refresh(dsp_layout* layout, const int64_t* d_frame_offsets, void* stream) {
    if (!layout || !d_frame_offsets) return dsp_fail(DSP_EINVAL, "dsp_layout_refresh: NULL argument");
    if (!layout->capacity) return dsp_fail(DSP_EINVAL, "dsp_layout_refresh: the handle is not from dsp_layout_create_capacity: its tables fit one batch shape");
    if (int rc = dsp_refuse_dry_run("dsp_layout_refresh", layout->dry_run)) return rc;
    const int rc = check_owner_device(layout->device, false);
    if (rc != DSP_OK) return rc;
    if (layout->group_off != nullptr) {
        f512_build_group_tables(d_frame_offsets, layout->n_utt, layout->shift, layout->group_off, layout->group_utt, (hipStream_t)stream);
        if (layout->group_off2 != nullptr)
            f512_build_group_tables(d_frame_offsets, layout->n_utt, 3, layout->group_off2, layout->group_utt2, (hipStream_t)stream);
        HIP_TRY(hipGetLastError());
    }
    return DSP_OK;
}

int dsp_vad_features_layout_batch(const dsp_layout* layout, const void* d_wave, int wave_dtype,
                                  const int64_t* d_sample_offsets, const int64_t* d_frame_offsets, int32_t use_sq,
                                  double* d_amp_sum, int32_t* d_zcr, void* stream) {
    if (!layout) return dsp_fail(DSP_EINVAL, "dsp_vad_features_layout_batch: layout is NULL");
    if (layout->dry_run) return dsp_fail(DSP_EINVAL, "dsp_vad_features_layout_batch: dry_run: launches are refused under dsp_debug_host_dry_run");
    const int rc = check_owner_device(layout->device, false);
    if (rc != DSP_OK) return rc;
    return vad_features_impl(layout, d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, layout->n_utt,
                             layout->n_frames_total, 0, layout->frame_len, layout->frame_step, use_sq, d_amp_sum, d_zcr,
                             stream);
}

int dsp_vad_features_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                           const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total,
                           int64_t uniform_samples, int32_t frame_len, int32_t frame_step, int32_t use_sq,
                           double* d_amp_sum, int32_t* d_zcr, void* stream) {
    return vad_features_impl(nullptr, d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total,
                             uniform_samples, frame_len, frame_step, use_sq, d_amp_sum, d_zcr, stream);
}

int dsp_trim_scale_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                         const int64_t* d_segments, const int64_t* d_dst_offsets, int32_t n_utt,
                         int32_t unit_variance, float* d_out, void* stream) {
    if (!d_wave || !d_sample_offsets || !d_segments || !d_dst_offsets || !d_out || n_utt <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_trim_scale_batch: bad arguments");
    if (wave_dtype != DSP_WAVE_I16 && wave_dtype != DSP_WAVE_F32) return dsp_fail(DSP_EINVAL, "unsupported wave_dtype %d", wave_dtype);
    dsp_dispatch_wave(wave_dtype, [&](auto dt) {
        trim_scale_kernel<decltype(dt)::value><<<n_utt, 256, 0, (hipStream_t)stream>>>(d_wave, d_sample_offsets, d_segments, d_dst_offsets, unit_variance, d_out);
    });
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_segments_workspace_bytes(const dsp_plan* plan, int32_t n_utt, int64_t n_frames_bound, size_t* bytes) {
    if (!plan || !bytes || n_utt <= 0 || n_frames_bound <= 0) return dsp_fail(DSP_EINVAL, "dsp_segments_workspace_bytes: bad arguments");
    *bytes = seg_work_layout(n_utt, n_frames_bound, plan->C).total;
    return DSP_OK;
}

int dsp_mfcc_delta_segments_batch(const dsp_plan* plan, const void* d_wave, int wave_dtype,
                                  const int64_t* d_sample_offsets, const int64_t* d_segments,
                                  const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_bound,
                                  int32_t delta_n, int32_t flags, void* d_work, size_t work_bytes,
                                  float* d_out, void* stream) {
    const int unit_variance = flags & DSP_SEG_UNIT_VARIANCE;
    if (!plan || !d_out || !d_work || !d_segments) return dsp_fail(DSP_EINVAL, "dsp_mfcc_delta_segments_batch: NULL argument");
    if (delta_n < 0) return dsp_fail(DSP_EINVAL, "N must be an integer >= 1 (or 0: cepstra only)");  // base.py:71-72
    int rc = check_geom(d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt, n_frames_bound, 0);
    if (rc != DSP_OK) return rc;
    rc = check_owner_device(plan->device, true);
    if (rc != DSP_OK) return rc;
    const int C = plan->C;
    BatchGeom bg = make_geom(d_sample_offsets, d_frame_offsets, n_utt, n_frames_bound, 0, plan->L, plan->S);
    // Served by the NFFT = 512 and NFFT = 1536 kernels on buffers they can read in place; everything else (and unit
    // variance without appendEnergy, where the scaling does not reduce to a shift of c0) reports 1: "use the
    // trimmed-copy path".
    const bool k512 = plan->d_fast && fast512_applicable(plan, bg, d_wave, wave_dtype);
    const bool k1536 = !k512 && plan->d_fast1536 && fast1536_applicable(plan, bg, d_wave, wave_dtype);
    if (g_force_generic || (!k512 && !k1536) || C <= 0 || delta_tile_lds(delta_n, C) > 64 * 1024 ||
        (unit_variance && !plan->append_energy) || (n_frames_bound >> 2) + n_utt > 0x3fffffff)
        return 1;
    const SegWork w = seg_work_layout(n_utt, n_frames_bound, C);
    if (work_bytes < w.total) return dsp_fail(DSP_EINVAL, "work buffer too small (%zu < %zu bytes)", work_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    char* wp = static_cast<char*>(d_work);
    double* stats = unit_variance ? reinterpret_cast<double*>(wp + w.stats) : nullptr;
    int64_t* tile_off = reinterpret_cast<int64_t*>(wp + w.tile);
    DspRaggedTables pre;
    pre.shift = k512 ? 3 : 2;
    pre.group_off = reinterpret_cast<int32_t*>(wp + w.goff);
    pre.group_utt = reinterpret_cast<int32_t*>(wp + w.gutt);
    float* cep = delta_n >= 1 ? reinterpret_cast<float*>(wp + w.cep) : d_out;   // cepstra only: straight into the result
    // one small launch: group tables of the MFCC kernel, tile table of the delta pass, statistics zeroed -- unless
    // dsp_endpoint_layout_segments_batch has already left all of that in d_work
    if (!(flags & DSP_SEG_TABLES_READY))
        f512_build_group_tables(d_frame_offsets, n_utt, pre.shift, pre.group_off, pre.group_utt, st, tile_off, stats);
    bg.seg = d_segments;
    bg.stats = stats;
    rc = k512 ? fast512_launch(plan, d_wave, wave_dtype, bg, cep, (int64_t)C, st, &pre)
              : fast1536_launch(plan, d_wave, wave_dtype, bg, cep, (int64_t)C, st, &pre);
    if (rc != DSP_OK) return dsp_fail(rc < 0 ? rc : DSP_EHIP, "fused kernel launch failed");
    if (delta_n == 0) return DSP_OK;    // (unit variance: c0 still lacks -ln(var); dsp_model_finalize_segments_batch applies it)
    int64_t tiles;
    const int64_t blocks = delta_tile_blocks(0, n_frames_bound, n_utt, &tiles);
    if (blocks > 0x7fffffff) return dsp_fail(DSP_EINVAL, "too many delta tiles");
    // (the tile -> utterance table exists only when the layout kernel built the tables)
    const int32_t* tile_utt = (flags & DSP_SEG_TABLES_READY) ? reinterpret_cast<const int32_t*>(wp + w.tutt) : nullptr;
    launch_delta_rows(blocks, st, cep, frames_geom(d_frame_offsets, n_utt, n_frames_bound, 0), C, delta_n, d_out, tiles, tile_off,
                      d_segments, stats, tile_utt);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_endpoint_layout_batch(const int32_t* d_endpoints, const int64_t* d_sample_offsets, int32_t n_utt,
                              double cfg_step, double rate, int32_t frame_len, int32_t frame_step,
                              const int64_t* d_jitter, int64_t* d_segments, int64_t* d_dst_offsets,
                              int64_t* d_frame_offsets, void* stream) {
    if (!endpoint_layout_args_ok(d_endpoints, d_sample_offsets, d_segments, d_dst_offsets, d_frame_offsets, n_utt))
        return dsp_fail(DSP_EINVAL, "dsp_endpoint_layout_batch: bad arguments");
    if (!(cfg_step > 0.0) || !(rate > 0.0) || frame_len <= 0 || frame_step <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_endpoint_layout_batch: step, rate, frame_len, frame_step must be > 0");
    endpoint_layout_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(d_endpoints, d_sample_offsets, n_utt, cfg_step, rate,
                                                               frame_len, frame_step, d_jitter, d_segments,
                                                               d_dst_offsets, d_frame_offsets);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_endpoint_layout_segments_batch(const int32_t* d_endpoints, const int64_t* d_sample_offsets, int32_t n_utt,
                                       double cfg_step, double rate, const int64_t* d_jitter, int64_t* d_segments,
                                       int64_t* d_dst_offsets, int64_t* d_frame_offsets, const dsp_plan* plan,
                                       int64_t n_frames_bound, void* d_work, size_t work_bytes, void* stream) {
    if (!endpoint_layout_args_ok(d_endpoints, d_sample_offsets, d_segments, d_dst_offsets, d_frame_offsets, n_utt) || !plan || !d_work)
        return dsp_fail(DSP_EINVAL, "dsp_endpoint_layout_segments_batch: bad arguments");
    if (!(cfg_step > 0.0) || !(rate > 0.0) || n_frames_bound <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_endpoint_layout_segments_batch: step, rate, n_frames_bound must be > 0");
    if ((n_frames_bound >> 2) + n_utt > 0x3fffffff)   // the kernel's group and tile counters are int32 (as dsp_mfcc_delta_segments_batch checks)
        return dsp_fail(DSP_EINVAL, "dsp_endpoint_layout_segments_batch: batch too large");
    const SegWork w = seg_work_layout(n_utt, n_frames_bound, plan->C);
    if (work_bytes < w.total) return dsp_fail(DSP_EINVAL, "work buffer too small (%zu < %zu bytes)", work_bytes, w.total);
    char* wp = static_cast<char*>(d_work);
    endpoint_layout_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(
        d_endpoints, d_sample_offsets, n_utt, cfg_step, rate, plan->L, plan->S, d_jitter, d_segments, d_dst_offsets,
        d_frame_offsets, plan->d_fast ? 3 : 2 /* frames per group: 8 (NFFT = 512 kernel) or 4 (NFFT = 1536) */,
        reinterpret_cast<int32_t*>(wp + w.goff), reinterpret_cast<int32_t*>(wp + w.gutt),
        reinterpret_cast<int64_t*>(wp + w.tile), reinterpret_cast<double*>(wp + w.stats),
        reinterpret_cast<int32_t*>(wp + w.tutt));
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_model_finalize_batch(const float* d_mfcc, int64_t ld_in, const int64_t* d_frame_offsets, int32_t n_utt,
                             int32_t C, int32_t N, int32_t max_len, float* d_out, int32_t* d_len0, void* stream) {
    if (!d_mfcc || !d_frame_offsets || !d_out || !d_len0 || n_utt <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_model_finalize_batch: bad arguments");
    return model_finalize_impl(d_mfcc, ld_in, d_frame_offsets, n_utt, C, N, max_len, d_out, d_len0, nullptr, nullptr,
                               identity_placement(n_utt, 0), stream);
}

int dsp_model_finalize_segments_batch(const float* d_mfcc, int64_t ld_in, const int64_t* d_frame_offsets,
                                      const int64_t* d_segments, const void* d_work, int32_t n_utt, int32_t C, int32_t N,
                                      int32_t max_len, float* d_out, int32_t* d_len0, void* stream) {
    if (!d_mfcc || !d_frame_offsets || !d_segments || !d_work || !d_out || !d_len0 || n_utt <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_model_finalize_segments_batch: bad arguments");
    // the statistics sit at the start of the work buffer of dsp_mfcc_delta_segments_batch (seg_work_layout)
    return model_finalize_impl(d_mfcc, ld_in, d_frame_offsets, n_utt, C, N, max_len, d_out, d_len0, d_segments,
                               static_cast<const double*>(d_work), identity_placement(n_utt, 0), stream);
}

int dsp_model_finalize_placed_batch(const float* d_mfcc, int64_t ld_in, const int64_t* d_frame_offsets,
                                    const int64_t* d_segments, const void* d_work, int32_t n_utt, int32_t C, int32_t N,
                                    int32_t max_len, float* d_out, int32_t* d_len0, const int32_t* d_dst_col, int32_t n_cols,
                                    int32_t row_width, int32_t col_offset, void* stream) {
    if (!d_mfcc || !d_frame_offsets || !d_out || !d_len0 || n_utt <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_model_finalize_placed_batch: NULL argument or n_utt <= 0");
    if ((d_segments == nullptr) != (d_work == nullptr))
        return dsp_fail(DSP_EINVAL, "dsp_model_finalize_placed_batch: d_segments and d_work go together (both, or both NULL)");
    if (row_width <= 0) return dsp_fail(DSP_EINVAL, "dsp_model_finalize_placed_batch: row_width %d must be > 0", row_width);
    return model_finalize_impl(d_mfcc, ld_in, d_frame_offsets, n_utt, C, N, max_len, d_out, d_len0, d_segments,
                               static_cast<const double*>(d_work), OutPlacement{d_dst_col, n_cols, row_width, col_offset}, stream);
}

int dsp_model_timefeat_batch(const double* d_amp_sum, const int64_t* d_frame_offsets, int32_t n_utt,
                             int32_t frame_len, int32_t max_len, float* d_out, void* stream) {
    if (!d_amp_sum || !d_frame_offsets || !d_out || n_utt <= 0 || frame_len <= 0 || max_len <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_model_timefeat_batch: bad arguments");
    timefeat_finalize_kernel<<<n_utt, 64, 0, (hipStream_t)stream>>>(d_amp_sum, d_frame_offsets, n_utt, frame_len, max_len, d_out,
                                                                    identity_placement(n_utt, 2));
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_model_timefeat_placed_batch(const double* d_amp_sum, const int64_t* d_frame_offsets, int32_t n_utt, int32_t frame_len,
                                    int32_t max_len, float* d_out, const int32_t* d_dst_col, int32_t n_cols, int32_t row_width,
                                    int32_t col_offset, void* stream) {
    if (!d_amp_sum || !d_frame_offsets || !d_out || n_utt <= 0 || frame_len <= 0 || max_len <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_model_timefeat_placed_batch: NULL argument, or n_utt, frame_len or max_len <= 0");
    const OutPlacement pl{d_dst_col, n_cols, row_width, col_offset};
    int rc = placement_check(pl, n_utt, 2);
    if (rc != DSP_OK) return rc;
    timefeat_finalize_kernel<<<n_utt, 64, 0, (hipStream_t)stream>>>(d_amp_sum, d_frame_offsets, n_utt, frame_len, max_len, d_out, pl);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_pitch_scores_batch(const float* d_sig, const int64_t* d_sample_offsets, const int64_t* d_frame_offsets,
                           int32_t n_utt, int64_t n_frames_total, int64_t uniform_samples, int32_t frame_len,
                           int32_t frame_step, const float* d_taps, int32_t center_clip, int32_t lag_min,
                           int32_t lag_max, float* d_scores, void* stream) {
    if (!d_taps || !d_scores) return dsp_fail(DSP_EINVAL, "dsp_pitch_scores_batch: NULL taps/output");
    if (frame_len <= 0 || frame_len > PITCH_MAX_L || frame_step <= 0)
        return dsp_fail(DSP_EINVAL, "need 0 < frame_len <= %d and frame_step > 0", PITCH_MAX_L);
    if (lag_min < 0 || lag_max <= lag_min) return dsp_fail(DSP_EINVAL, "need 0 <= lag_min < lag_max");
    int rc = check_geom(d_sig, DSP_WAVE_F32, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples);
    if (rc != DSP_OK) return rc;
    if (n_frames_total > 0x7fffffff) return dsp_fail(DSP_EINVAL, "too many frames for one launch");
    BatchGeom bg = make_geom(d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples, frame_len, frame_step);
    int P = 1;
    while (P < frame_len) P <<= 1;
    // register-blocked kernel (one wave per frame) where its shape constraints hold
    const int n_lags = lag_max - lag_min;
    const int W = frame_len <= 384 ? 3 : (frame_len <= 512 ? 4 : 0);
    const float2* tp = reinterpret_cast<const float2*>(d_taps);
    if (W != 0 && (lag_min % 4) == 0 && n_lags <= 256 && lag_max + 8 <= PITCH2_GUARD && !g_force_generic) {
        dispatch_pitch_v2_width(W, [&](auto w) {
            constexpr int Wc = decltype(w)::value;
            pitch_scores_kernel_v2<Wc><<<(int)n_frames_total, 64, pitch_scores_v2_lds_bytes<Wc>(frame_len), (hipStream_t)stream>>>(
                d_sig, bg, frame_len, frame_step, P, tp, center_clip ? 1 : 0, lag_min, n_lags, d_scores);
        });
        HIP_TRY(hipGetLastError());
        return DSP_OK;
    }
    pitch_scores_kernel<<<(int)n_frames_total, PITCH_THREADS, pitch_scores_lds_bytes(frame_len, P), (hipStream_t)stream>>>(
        d_sig, bg, frame_len, frame_step, P, tp, center_clip ? 1 : 0, lag_min, n_lags, d_scores);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_pitch_track_batch(const float* d_scores, const int64_t* d_frame_offsets, int32_t n_utt, int32_t n_lags,
                          int32_t bias, int32_t degree, double* d_pitch, void* stream) {
    if (!d_scores || !d_frame_offsets || !d_pitch || n_utt <= 0) return dsp_fail(DSP_EINVAL, "dsp_pitch_track_batch: bad arguments");
    if (n_lags <= 0 || n_lags > 256) return dsp_fail(DSP_EINVAL, "need 0 < n_lags <= 256");
    if (degree != 2) return dsp_fail(DSP_EINVAL, "smoothing degree %d is not served on the device (the reference only uses 2)", degree);
    pitch_track_kernel<<<n_utt, 64, 0, (hipStream_t)stream>>>(d_scores, d_frame_offsets, n_lags, bias, d_pitch);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_endpoint_rule_batch(const double* d_amp_sum, const int32_t* d_zcr, const int64_t* d_frame_offsets,
                            int32_t n_utt, int32_t frame_len, double cfg_frame, double cfg_step,
                            int32_t* d_endpoints, void* stream) {
    if (!d_amp_sum || !d_zcr || !d_frame_offsets || !d_endpoints || n_utt <= 0 || frame_len <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_endpoint_rule_batch: bad arguments");
    return endpoint_rule_impl(d_amp_sum, d_zcr, nullptr, d_frame_offsets, n_utt, frame_len, cfg_frame, cfg_step, d_endpoints, stream);
}

int dsp_acr_gate_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                       const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total, int64_t uniform_samples,
                       int32_t frame_len, int32_t frame_step, int32_t lag_lo, int32_t lag_hi, double thresh,
                       uint8_t* d_voiced, void* stream) {
    if (!d_voiced) return dsp_fail(DSP_EINVAL, "dsp_acr_gate_batch: d_voiced is NULL");
    if (frame_len <= 0 || frame_step <= 0) return dsp_fail(DSP_EINVAL, "frame_len / frame_step must be > 0");
    if (lag_lo < 1 || lag_hi <= lag_lo || lag_hi > frame_len)
        return dsp_fail(DSP_EINVAL, "lags [%d, %d) must lie in [1, frame_len = %d]", lag_lo, lag_hi, frame_len);
    const size_t lds = (size_t)4 * frame_len * sizeof(double);
    if (lds > 64 * 1024) return dsp_fail(DSP_EINVAL, "frame_len %d too long for the autocorrelation gate (<= 2048)", frame_len);
    int rc = check_geom(d_wave, wave_dtype, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples);
    if (rc != DSP_OK) return rc;
    BatchGeom bg = make_geom(d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples, frame_len, frame_step);
    if (uniform_samples > 0 && (rc = check_dense_frames(n_frames_total, n_utt, bg.uniform_frames)) != DSP_OK) return rc;
    if (n_frames_total <= 0) return DSP_OK;
    const int64_t blocks = (n_frames_total + 3) / 4;
    if (blocks > 0x7fffffff) return dsp_fail(DSP_EINVAL, "too many frames");
    hipStream_t st = (hipStream_t)stream;
    dsp_dispatch_wave(wave_dtype, [&](auto dt) {
        acr_gate_kernel<decltype(dt)::value><<<(int)blocks, 256, lds, st>>>(d_wave, bg, frame_len, frame_step, lag_lo, lag_hi, thresh, d_voiced);
    });
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_endpoint_rule_acr_batch(const double* d_amp_sum, const int32_t* d_zcr, const uint8_t* d_voiced,
                                const int64_t* d_frame_offsets, int32_t n_utt, int32_t frame_len, double cfg_frame,
                                double cfg_step, int32_t* d_endpoints, void* stream) {
    if (!d_amp_sum || !d_zcr || !d_voiced || !d_frame_offsets || !d_endpoints || n_utt <= 0 || frame_len <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_endpoint_rule_acr_batch: bad arguments");
    return endpoint_rule_impl(d_amp_sum, d_zcr, d_voiced, d_frame_offsets, n_utt, frame_len, cfg_frame, cfg_step, d_endpoints, stream);
}

int dsp_resample_layout_batch(const int64_t* d_src_offsets, int32_t n_utt, int64_t src_rate, int64_t dst_rate,
                              int32_t frame_len, int32_t frame_step, int64_t* d_dst_offsets, int64_t* d_frame_offsets,
                              void* stream) {
    if (!d_src_offsets || !d_frame_offsets || n_utt <= 0 || frame_len <= 0 || frame_step <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_resample_layout_batch: bad arguments");
    if (dst_rate < 0 || (dst_rate > 0 && (src_rate <= 0 || dst_rate >= src_rate || !d_dst_offsets)))
        return dsp_fail(DSP_EINVAL, "dsp_resample_layout_batch: need 0 < dst_rate < src_rate and d_dst_offsets (a decimation), or dst_rate = 0");
    resample_layout_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(d_src_offsets, n_utt, src_rate, dst_rate, frame_len, frame_step,
                                                               d_dst_offsets, d_frame_offsets);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_decimate_batch(const float* d_in, const int64_t* d_src_offsets, const int64_t* d_dst_offsets, int32_t n_utt,
                       int64_t n_out_bound, int64_t src_rate, int64_t dst_rate, float* d_out, void* stream) {
    if (!d_in || !d_src_offsets || !d_dst_offsets || !d_out || n_utt <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_decimate_batch: bad arguments");
    if (src_rate <= 0 || dst_rate <= 0 || dst_rate >= src_rate) return dsp_fail(DSP_EINVAL, "dsp_decimate_batch: need 0 < dst_rate < src_rate");
    if (n_out_bound <= 0) return DSP_OK;
    decimate_gather_kernel<<<grid_for(n_out_bound, 256), 256, 0, (hipStream_t)stream>>>(d_in, d_src_offsets, d_dst_offsets, n_utt,
                                                                                         src_rate, dst_rate, d_out);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_model_pitchfeat_batch(const double* d_pitch, const int64_t* d_frame_offsets, int32_t n_utt, int32_t max_len,
                              float* d_out, void* stream) {
    if (!d_pitch || !d_frame_offsets || !d_out || n_utt <= 0 || max_len <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_model_pitchfeat_batch: bad arguments");
    pitchfeat_finalize_kernel<<<n_utt, 64, 0, (hipStream_t)stream>>>(d_pitch, d_frame_offsets, n_utt, max_len, d_out,
                                                                     identity_placement(n_utt, 2));
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_model_pitchfeat_placed_batch(const double* d_pitch, const int64_t* d_frame_offsets, int32_t n_utt, int32_t max_len,
                                     float* d_out, const int32_t* d_dst_col, int32_t n_cols, int32_t row_width,
                                     int32_t col_offset, void* stream) {
    if (!d_pitch || !d_frame_offsets || !d_out || n_utt <= 0 || max_len <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_model_pitchfeat_placed_batch: NULL argument, or n_utt or max_len <= 0");
    const OutPlacement pl{d_dst_col, n_cols, row_width, col_offset};
    int rc = placement_check(pl, n_utt, 2);
    if (rc != DSP_OK) return rc;
    pitchfeat_finalize_kernel<<<n_utt, 64, 0, (hipStream_t)stream>>>(d_pitch, d_frame_offsets, n_utt, max_len, d_out, pl);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_gather_clips_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets, const int32_t* d_pick,
                           int32_t n_pick, const int64_t* d_dst_offsets, void* d_out, void* stream) {
    if (!d_wave || !d_sample_offsets || !d_pick || !d_dst_offsets || !d_out)
        return dsp_fail(DSP_EINVAL, "dsp_gather_clips_batch: NULL argument");
    if (n_pick < 0) return dsp_fail(DSP_EINVAL, "dsp_gather_clips_batch: n_pick %d is negative", n_pick);
    if (wave_dtype != DSP_WAVE_F32 && wave_dtype != DSP_WAVE_I16)
        return dsp_fail(DSP_EINVAL, "dsp_gather_clips_batch: bad wave_dtype %d", wave_dtype);
    if (int rc = dsp_refuse_dry_run(nullptr)) return rc;
    if (n_pick == 0) return DSP_OK;
    const dim3 grid(GATHER_CHUNKS, (unsigned)n_pick);
    if (wave_dtype == DSP_WAVE_I16)
        gather_clips_kernel<int16_t><<<grid, 256, 0, (hipStream_t)stream>>>(static_cast<const int16_t*>(d_wave), d_sample_offsets,
                                                                            d_pick, d_dst_offsets, static_cast<int16_t*>(d_out));
    else
        gather_clips_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(static_cast<const float*>(d_wave), d_sample_offsets,
                                                                          d_pick, d_dst_offsets, static_cast<float*>(d_out));
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

// Are two of these `n` table pointers the same, or one of them `other`?  (The tables of one kind have one size: equal start = overlap.)
static bool tables_collide(const void* const* t, int n, const void* other) {
    for (int g = 0; g < n; ++g) {
        if (t[g] == other) return true;
        for (int h = 0; h < g; ++h)
            if (t[h] == t[g]) return true;
    }
    return false;
}

int dsp_rate_groups_batch(const int32_t* d_rates, const int64_t* d_sample_offsets_in, const int64_t* d_jitter, int32_t n_utt,
                          int64_t sample_capacity, int32_t n_groups, const int32_t* group_rates, int64_t pad_len,
                          int64_t* d_sample_offsets, int32_t* const* d_pick, int32_t* const* d_dst_col,
                          int64_t* const* d_group_offsets, int64_t* const* d_group_jitter, int32_t* d_count, int32_t* d_status,
                          void* stream) {
    if (!d_rates || !d_sample_offsets_in || !group_rates || !d_sample_offsets || !d_pick || !d_dst_col || !d_group_offsets ||
        !d_count || !d_status)
        return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: NULL argument");
    if ((d_jitter == nullptr) != (d_group_jitter == nullptr))
        return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: d_jitter and d_group_jitter go together (both, or both NULL)");
    if (n_utt <= 0) return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: n_utt %d must be >= 1", n_utt);
    if (sample_capacity <= 0) return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: sample_capacity %lld must be >= 1", (long long)sample_capacity);
    if (n_groups < 1 || n_groups > DSP_MAX_RATE_GROUPS)
        return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: n_groups %d must be in [1, %d]", n_groups, DSP_MAX_RATE_GROUPS);
    if (pad_len < 1) return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: pad_len %lld must be >= 1", (long long)pad_len);
    if (pad_len > (INT64_MAX - sample_capacity) / n_utt)
        return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: sample_capacity + n_utt * pad_len overflows int64");
    if (d_sample_offsets == d_sample_offsets_in)
        return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: the sanitised table must not be the caller's (overlap)");
    RateGroupsArgs A;
    memset(&A, 0, sizeof(A));
    A.n_groups = n_groups;
    for (int g = 0; g < n_groups; ++g) {
        if (group_rates[g] <= 0) return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: group %d: rate %d must be > 0", g, group_rates[g]);
        for (int h = 0; h < g; ++h)
            if (group_rates[h] == group_rates[g])
                return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: groups %d and %d share the rate %d", h, g, group_rates[g]);
        if (!d_pick[g] || !d_dst_col[g] || !d_group_offsets[g] || (d_group_jitter && !d_group_jitter[g]))
            return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: group %d: NULL table", g);
        A.rate[g] = group_rates[g]; A.pick[g] = d_pick[g]; A.dst_col[g] = d_dst_col[g]; A.offsets[g] = d_group_offsets[g];
        A.jitter[g] = d_group_jitter ? d_group_jitter[g] : nullptr;
    }
    const void* i32_tabs[2 * DSP_MAX_RATE_GROUPS];
    const void* i64_tabs[2 * DSP_MAX_RATE_GROUPS + 1];
    int n32 = 0, n64 = 0;
    for (int g = 0; g < n_groups; ++g) {
        i32_tabs[n32++] = d_pick[g]; i32_tabs[n32++] = d_dst_col[g];
        i64_tabs[n64++] = d_group_offsets[g];
        if (d_group_jitter) i64_tabs[n64++] = d_group_jitter[g];
    }
    i64_tabs[n64++] = d_sample_offsets;
    if (tables_collide(i32_tabs, n32, d_rates) || tables_collide(i32_tabs, n32, d_count) || tables_collide(i32_tabs, n32, d_status) ||
        tables_collide(i64_tabs, n64, d_sample_offsets_in) || tables_collide(i64_tabs, n64, d_jitter) || d_count == d_status)
        return dsp_fail(DSP_EINVAL, "dsp_rate_groups_batch: two tables share their memory (overlap)");
    if (int rc = dsp_refuse_dry_run("dsp_rate_groups_batch")) return rc;
    rate_groups_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(d_rates, d_sample_offsets_in, d_jitter, n_utt, sample_capacity, pad_len, A,
                                                           d_sample_offsets, d_count, d_status);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_gather_groups_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets, int32_t n_utt, int32_t n_groups,
                            const int32_t* const* d_pick, const int64_t* const* d_group_offsets, int64_t pad_len,
                            void* const* d_out, void* stream) {
    if (!d_wave || !d_sample_offsets || !d_pick || !d_group_offsets || !d_out)
        return dsp_fail(DSP_EINVAL, "dsp_gather_groups_batch: NULL argument");
    if (wave_dtype != DSP_WAVE_F32 && wave_dtype != DSP_WAVE_I16)
        return dsp_fail(DSP_EINVAL, "dsp_gather_groups_batch: bad wave_dtype %d", wave_dtype);
    if (n_utt < 1 || n_utt > 65535) return dsp_fail(DSP_EINVAL, "dsp_gather_groups_batch: n_utt %d must be in [1, 65535]", n_utt);
    if (n_groups < 1 || n_groups > DSP_MAX_RATE_GROUPS)
        return dsp_fail(DSP_EINVAL, "dsp_gather_groups_batch: n_groups %d must be in [1, %d]", n_groups, DSP_MAX_RATE_GROUPS);
    if (pad_len < 1) return dsp_fail(DSP_EINVAL, "dsp_gather_groups_batch: pad_len %lld must be >= 1", (long long)pad_len);
    GatherGroupsArgs A;
    memset(&A, 0, sizeof(A));
    for (int g = 0; g < n_groups; ++g) {
        if (!d_pick[g] || !d_group_offsets[g] || !d_out[g]) return dsp_fail(DSP_EINVAL, "dsp_gather_groups_batch: group %d: NULL table or buffer", g);
        if (!aligned(d_out[g], 16))
            return dsp_fail(DSP_EINVAL, "dsp_gather_groups_batch: group %d: the buffer does not start on a 16-byte vector (alignment)", g);
        A.pick[g] = d_pick[g]; A.offsets[g] = d_group_offsets[g]; A.out[g] = d_out[g];
    }
    if (tables_collide(d_out, n_groups, d_wave))
        return dsp_fail(DSP_EINVAL, "dsp_gather_groups_batch: two wave buffers share their memory (overlap)");
    if (int rc = dsp_refuse_dry_run("dsp_gather_groups_batch")) return rc;
    const dim3 grid(GATHER_CHUNKS, (unsigned)n_utt, (unsigned)n_groups);
    if (wave_dtype == DSP_WAVE_I16)
        gather_groups_kernel<int16_t><<<grid, 256, 0, (hipStream_t)stream>>>(static_cast<const int16_t*>(d_wave), d_sample_offsets, pad_len, A);
    else
        gather_groups_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(static_cast<const float*>(d_wave), d_sample_offsets, pad_len, A);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_scatter_segments_batch(const int64_t* const* d_group_segments, const int32_t* const* d_dst_col, int32_t n_utt,
                               int32_t n_groups, int64_t* d_endpoints, void* stream) {
    if (!d_group_segments || !d_dst_col || !d_endpoints) return dsp_fail(DSP_EINVAL, "dsp_scatter_segments_batch: NULL argument");
    if (n_utt < 1) return dsp_fail(DSP_EINVAL, "dsp_scatter_segments_batch: n_utt %d must be >= 1", n_utt);
    if (n_groups < 1 || n_groups > DSP_MAX_RATE_GROUPS)
        return dsp_fail(DSP_EINVAL, "dsp_scatter_segments_batch: n_groups %d must be in [1, %d]", n_groups, DSP_MAX_RATE_GROUPS);
    ScatterSegmentsArgs A;
    memset(&A, 0, sizeof(A));
    for (int g = 0; g < n_groups; ++g) {
        if (!d_group_segments[g] || !d_dst_col[g]) return dsp_fail(DSP_EINVAL, "dsp_scatter_segments_batch: group %d: NULL table", g);
        A.seg[g] = d_group_segments[g]; A.dst_col[g] = d_dst_col[g];
    }
    if (tables_collide(reinterpret_cast<const void* const*>(d_group_segments), n_groups, d_endpoints))
        return dsp_fail(DSP_EINVAL, "dsp_scatter_segments_batch: the endpoints must not be a group's segment table (overlap)");
    if (int rc = dsp_refuse_dry_run("dsp_scatter_segments_batch")) return rc;
    const dim3 grid((unsigned)((n_utt + 255) / 256), (unsigned)n_groups);
    scatter_segments_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(A, n_utt, d_endpoints);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_scatter_group_rows_batch(const void* const* d_group_rows, const int32_t* const* d_dst_col, int32_t n_utt, int32_t n_groups,
                                 int32_t row_bytes, void* d_out, void* stream) {
    if (!d_group_rows || !d_dst_col || !d_out) return dsp_fail(DSP_EINVAL, "dsp_scatter_group_rows_batch: NULL argument");
    if (n_utt < 1 || n_utt > 65535) return dsp_fail(DSP_EINVAL, "dsp_scatter_group_rows_batch: n_utt %d must be in [1, 65535]", n_utt);
    if (n_groups < 1 || n_groups > DSP_MAX_RATE_GROUPS)
        return dsp_fail(DSP_EINVAL, "dsp_scatter_group_rows_batch: n_groups %d must be in [1, %d]", n_groups, DSP_MAX_RATE_GROUPS);
    if (row_bytes < 4 || row_bytes > 256 || (row_bytes & 3) != 0)
        return dsp_fail(DSP_EINVAL, "dsp_scatter_group_rows_batch: row_bytes %d must be a multiple of 4 in [4, 256]", row_bytes);
    if (!aligned(d_out, 4))
        return dsp_fail(DSP_EINVAL, "dsp_scatter_group_rows_batch: the output does not start on a 4-byte word (alignment)");
    const int64_t table_bytes = (int64_t)n_utt * row_bytes, col_bytes = (int64_t)n_utt * 4;
    const Range out = range_of(d_out, table_bytes);
    ScatterRowsArgs A;
    memset(&A, 0, sizeof(A));
    for (int g = 0; g < n_groups; ++g) {
        if (!d_group_rows[g] || !d_dst_col[g]) return dsp_fail(DSP_EINVAL, "dsp_scatter_group_rows_batch: group %d: NULL table", g);
        if (!aligned(d_group_rows[g], 4) || !aligned(d_dst_col[g], 4))
            return dsp_fail(DSP_EINVAL, "dsp_scatter_group_rows_batch: group %d: a table does not start on a 4-byte word (alignment)", g);
        if (overlap(out, range_of(d_group_rows[g], table_bytes)) || overlap(out, range_of(d_dst_col[g], col_bytes)))
            return dsp_fail(DSP_EINVAL, "dsp_scatter_group_rows_batch: group %d: the output must not share memory with a group's table (overlap)", g);
        A.rows[g] = static_cast<const uint32_t*>(d_group_rows[g]); A.dst_col[g] = d_dst_col[g];
    }
    if (int rc = dsp_refuse_dry_run("dsp_scatter_group_rows_batch")) return rc;
    const int32_t row_words = row_bytes / 4;                 // n_utt * row_words <= 65535 * 64: at most 16384 workgroups a group
    const dim3 grid((unsigned)(((int64_t)n_utt * row_words + 255) / 256), (unsigned)n_groups);
    scatter_group_rows_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(A, n_utt, row_words, static_cast<uint32_t*>(d_out));
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_pitch_rows_batch(double* d_rows, const int64_t* d_frame_offsets, int32_t n_utt, int32_t n_lags, int32_t bias,
                         int32_t degree, int32_t flags, double* d_pitch, void* stream) {
    if (!d_rows || !d_frame_offsets || n_utt <= 0 || n_lags <= 0 || degree < 0)
        return dsp_fail(DSP_EINVAL, "dsp_pitch_rows_batch: bad arguments");
    if ((flags & 4) && !(flags & 2)) return dsp_fail(DSP_EINVAL, "dsp_pitch_rows_batch: the repair sweeps (4) need the arg-max (2)");
    if ((flags & 2) && !d_pitch) return dsp_fail(DSP_EINVAL, "dsp_pitch_rows_batch: d_pitch is NULL");
    pitch_rows_kernel<<<n_utt, 64, 0, (hipStream_t)stream>>>(d_rows, d_frame_offsets, n_lags, bias, degree, flags, d_pitch);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_pitch_cepstrum_batch(const float* d_sig, const int64_t* d_sample_offsets, const int64_t* d_frame_offsets,
                             int32_t n_utt, int64_t n_frames_total, int64_t uniform_samples, int32_t frame_len,
                             int32_t frame_step, const float* d_taps, int32_t center_clip, float* d_rows, double* d_amp,
                             void* stream) {
    if (!d_taps || !d_rows) return dsp_fail(DSP_EINVAL, "dsp_pitch_cepstrum_batch: NULL taps/output");
    if (!cepstrum_frame_len_ok(frame_len))
        return dsp_fail(DSP_EINVAL, "dsp_pitch_cepstrum_batch: frame_len %d is not a power of two in [128, 1024]", frame_len);
    if (frame_step <= 0) return dsp_fail(DSP_EINVAL, "dsp_pitch_cepstrum_batch: frame_step must be > 0");
    int rc = check_geom(d_sig, DSP_WAVE_F32, d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples);
    if (rc != DSP_OK) return rc;
    if (n_frames_total > 0x7fffffff) return dsp_fail(DSP_EINVAL, "too many frames for one launch");
    BatchGeom bg = make_geom(d_sample_offsets, d_frame_offsets, n_utt, n_frames_total, uniform_samples, frame_len, frame_step);
    if (uniform_samples > 0 && (rc = check_dense_frames(n_frames_total, n_utt, bg.uniform_frames)) != DSP_OK) return rc;
    const float2* tp = reinterpret_cast<const float2*>(d_taps);
    const int grid = (int)n_frames_total, clip = center_clip ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    dispatch_cepstrum_frame_len(frame_len, [&](auto len) {
        pitch_cepstrum_kernel<decltype(len)::value><<<grid, 64, 0, st>>>(d_sig, bg, frame_step, tp, clip, d_rows, d_amp);
    });
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_pitch_cepstrum_track_batch(const void* d_rows, int32_t rows_f64, const int64_t* d_frame_offsets, int32_t n_utt,
                                   int32_t frame_len, int32_t flags, double* d_pitch, int32_t* d_scores, void* stream) {
    if (!d_rows || !d_frame_offsets || n_utt <= 0) return dsp_fail(DSP_EINVAL, "dsp_pitch_cepstrum_track_batch: bad arguments");
    if (!cepstrum_frame_len_ok(frame_len))
        return dsp_fail(DSP_EINVAL, "dsp_pitch_cepstrum_track_batch: frame_len %d is not a power of two in [128, 1024]", frame_len);
    if ((flags & ~3) != 0) return dsp_fail(DSP_EINVAL, "dsp_pitch_cepstrum_track_batch: unknown flags %d", flags);
    if ((flags & 2) && !d_pitch) return dsp_fail(DSP_EINVAL, "dsp_pitch_cepstrum_track_batch: d_pitch is NULL");
    if (!(flags & 2) && !d_scores) return dsp_fail(DSP_EINVAL, "dsp_pitch_cepstrum_track_batch: nothing to write (no arg-max, d_scores is NULL)");
    dispatch_cepstrum_frame_len(frame_len, [&](auto len) {
        auto launch = [&](auto row) {   // row: a value of the rows' element type
            pitch_cepstrum_track_kernel<decltype(row), decltype(len)::value><<<n_utt, 64, 0, (hipStream_t)stream>>>(
                static_cast<const decltype(row)*>(d_rows), d_frame_offsets, flags, d_pitch, d_scores);
        };
        if (rows_f64) launch(double()); else launch(float());
    });
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_pitch_feature_batch(const double* d_pitch, const double* d_amp, const int64_t* d_frame_offsets, int32_t n_utt,
                            double* d_seg, double* d_feat, int32_t* d_aux, void* stream) {
    if (!d_amp || !d_frame_offsets || !d_aux || n_utt <= 0) return dsp_fail(DSP_EINVAL, "dsp_pitch_feature_batch: bad arguments");
    if (d_pitch && (!d_seg || !d_feat)) return dsp_fail(DSP_EINVAL, "dsp_pitch_feature_batch: d_pitch needs d_seg and d_feat");
    pitch_feature_kernel<<<n_utt, 64, 0, (hipStream_t)stream>>>(d_pitch, d_amp, d_frame_offsets, d_seg, d_feat, d_aux);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_pitch_smooth_subseq_batch(const double* d_values, const int64_t* d_offsets, int32_t n_utt, int32_t tor,
                                  double thres, double* d_seg, int32_t* d_info, void* stream) {
    if (!d_values || !d_offsets || !d_seg || !d_info || n_utt <= 0)
        return dsp_fail(DSP_EINVAL, "dsp_pitch_smooth_subseq_batch: bad arguments");
    if (tor < 1) return dsp_fail(DSP_EINVAL, "dsp_pitch_smooth_subseq_batch: tor must be >= 1 (got %d)", tor);
    pitch_subseq_kernel<<<n_utt, 64, 0, (hipStream_t)stream>>>(d_values, d_offsets, tor, thres, d_seg, d_info);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // extern "C"
