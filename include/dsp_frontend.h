/*
 * dsp_frontend.h -- C ABI of the MI355X-native speech feature front-end (libdsp_frontend.so).
 *
 * Drop-in boundary.  The reference (AuCson/DSP-Speech-Recognition) is 100 % Python: its "FFI" for
 * this path is the module surface of features/{sigproc,base,endpoint}.py.  Each entry point below
 * names the reference function(s) (file:line, relative to the reference checkout) whose arithmetic
 * it replaces; the Python mirror in dsp-speech-recognition_amd/features/ binds them with ctypes
 * under the reference's own function names.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void*
 *     (NULL = default stream); every pointer prefixed d_ is DEVICE memory, h_ is host memory.
 *   - every function returns DSP_OK (0) or a negative DSP_E* code; dsp_last_error() gives the
 *     thread-local message.  Nothing falls back to a CPU path: without a GPU calls fail.
 *   - waveform buffers may start at any element-aligned address and dense batches may have any
 *     length: what the fused kernels cannot take directly (a start that is not 16-byte aligned, a
 *     dense length that is not a multiple of 4) is viewed as a ragged batch of the aligned buffer
 *     underneath, with offset tables built on the device.
 *   - utterances are concatenated: sample_offsets[B+1] (int64) into the wave buffer,
 *     frame_offsets[B+1] (int64) into the [sum T_b, D] output (row-major, fp32).
 *   - no global mutable state besides the thread-local error string; a plan is immutable after
 *     creation and may be used from several host threads / streams concurrently.
 */
#ifndef DSP_FRONTEND_H
#define DSP_FRONTEND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSP_ABI_VERSION 2

/* status codes */
#define DSP_OK          0
#define DSP_EINVAL     -1   /* bad argument / unsupported configuration */
#define DSP_EHIP       -2   /* HIP runtime error (message has hipGetErrorString) */
#define DSP_ENODEV     -3   /* no usable GPU */

/* waveform sample types */
#define DSP_WAVE_F32    0
#define DSP_WAVE_I16    1   /* what reader.py:80 yields (int16 PCM) */

/* which stage's output dsp_features_batch writes */
#define DSP_OUT_FRAMES   0  /* [sumT, L]        sigproc.framesig      sigproc.py:66-98   */
#define DSP_OUT_MAGSPEC  1  /* [sumT, NFFT/2+1] sigproc.magspec       sigproc.py:136-148 */
#define DSP_OUT_POWSPEC  2  /* [sumT, NFFT/2+1] sigproc.powspec       sigproc.py:151-158 */
#define DSP_OUT_FBANK    3  /* [sumT, M] + energy[sumT]  base.fbank   base.py:18-32      */
#define DSP_OUT_MFCC     4  /* [sumT, C]        base.mfcc             base.py:8-16       */

typedef struct dsp_plan dsp_plan;

/*
 * Host-built tables for one (rate, L, S, NFFT, M, C, preemph, lifter, window) tuple.  The host side
 * evaluates everything the reference evaluates in Python/fp64 per call -- round_half_up of the frame
 * sizes (sigproc.py:55-56,77-78), winfunc(L) (sigproc.py:89), get_filterbanks (base.py:40-58), the
 * DCT-II/ortho matrix (base.py:13, scipy.fftpack.dct) with the lifter (base.py:60-68) folded in --
 * once, in fp64, and hands them over rounded to fp32.
 */
typedef struct dsp_plan_desc {
    int32_t frame_len;        /* L  samples per frame (after round_half_up)                        */
    int32_t frame_step;       /* S  hop in samples                                                 */
    int32_t nfft;             /* NFFT: 2^k or 3*2^k, 16 <= NFFT <= 4096 -- with DSP_PLAN_ANY_NFFT every
                                 integer in that range; frames longer are truncated
                                 (sigproc.py:143-147).  Each of the 17 sizes runs in a device test
                                 against the oracle (tests/test_gpu_generic_configs.py), 24 of the
                                 others in tests/test_gpu_anyfft.py                                */
    int32_t nfilt;            /* M  mel filters (0 if the plan is only used up to POWSPEC)         */
    int32_t numcep;           /* C  cepstra kept, C <= M                                           */
    int32_t append_energy;    /* base.py:15 -- column 0 := log(frame energy)                       */
    float   preemph;          /* base.py:22 -- 0 disables the filter                               */
    const float*   h_window;      /* [L]                                                           */
    const int32_t* h_mel_start;   /* [M] first FFT bin of filter j with a stored weight            */
    const int32_t* h_mel_count;   /* [M] number of stored weights                                  */
    const float*   h_mel_weights; /* [sum count] row after row                                     */
    const float*   h_dct;         /* [C, M] row-major, lifter already multiplied in                */
    /* The fp64 side (ABI 2).  A mel filter that comes out below 7e-10 of its frame's energy -- pre-emphasis and window
       nearly cancel its one or two bins -- is beyond an fp32 spectrum; the MFCC kernels recompute such a filter's bins
       as fp64 DFT sums over the samples, and need window and coefficient as the reference has them. */
    const double*  h_window64;    /* [L] the window before it was rounded to h_window; read only if nfilt > 0 */
    double         preemph64;     /* the coefficient before it was rounded to preemph; checked and read only if nfilt > 0 */
} dsp_plan_desc;

/* ---- library / device plumbing ------------------------------------------------------------- */
int         dsp_abi_version(void);
const char* dsp_last_error(void);
int dsp_device_count(int* n);
int dsp_set_device(int device);
int dsp_get_device(int* device);   /* plans, buffers and workspaces belong to the device current at creation */
int dsp_malloc(void** d_ptr, size_t bytes);
int dsp_free(void* d_ptr);
int dsp_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);
int dsp_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);
int dsp_memset(void* d_dst, int value, size_t bytes, void* stream);
int dsp_stream_synchronize(void* stream);

/* ---- host-side geometry (no GPU needed) ---------------------------------------------------- */
/* T = 1 if n <= L else 1 + ceil((n - L) / S)                       sigproc.py:79-82 */
int dsp_frame_count(int64_t n_samples, int32_t frame_len, int32_t frame_step, int64_t* n_frames);
/* frame_offsets[0]=0, frame_offsets[b+1]=frame_offsets[b]+T_b      (h_ pointers)    */
int dsp_frame_offsets(const int64_t* h_sample_offsets, int32_t n_utt, int32_t frame_len,
                      int32_t frame_step, int64_t* h_frame_offsets);
/* An upper bound on sum_b T_b over EVERY batch of n_utt clips whose lengths sum to at most sample_capacity -- a function of
 * (sample_capacity, n_utt, frame_len, frame_step) alone: sample_capacity / frame_step + n_utt where frame_len >= frame_step
 * (T(n) <= n / S + 1 then), + 2 n_utt otherwise (T(n) <= n / S + 2 always).  What a capacity layout sizes its grids,
 * tables and buffers by.  DSP_EINVAL where the bound does not fit int64. */
int dsp_frames_bound(int64_t sample_capacity, int32_t n_utt, int32_t frame_len, int32_t frame_step, int64_t* n_frames_bound);

/* ---- plans --------------------------------------------------------------------------------- */
int dsp_plan_create(const dsp_plan_desc* desc, dsp_plan** plan);
/* flags = 0: dsp_plan_create.  DSP_PLAN_ANY_NFFT: every integer 16 <= nfft <= 4096 is accepted, as numpy.fft.rfft takes any
   size (sigproc.py:136-148, base.py:40-58); the sizes dsp_plan_create accepts get the plan it builds. */
#define DSP_PLAN_ANY_NFFT 1
int dsp_plan_create_ex(const dsp_plan_desc* desc, uint32_t flags, dsp_plan** plan);
/* How the generic kernel transforms a frame of this plan.  route 0: the pass list of the 17 sizes 2^k and 3*2^k; 1: mixed
   radix (even nfft whose half is 2^a 3^b 5^c: radix 2 / 3 / 4 / 5 passes over the packed real transform); 2: chirp-z
   (every other size), a circular convolution of *conv_len points (the smallest 2^k or 3*2^k >= min(frame_len, nfft) +
   nfft/2).  *conv_len is 0 on routes 0 and 1. */
int dsp_plan_transform(const dsp_plan* plan, int32_t* route, int32_t* conv_len);
/* testing aid: the transform's host tables, also of a plan made under dsp_debug_host_dry_run.  radix[0 .. *n_pass) is the
   pass list (on route 2 that of the convolution transform; radix_cap: the room in radix, 12 always suffices).  Route 2
   only, either may be NULL: h_chirp [nfft][2] = exp(-i pi n^2 / nfft), h_chirp_spec [conv_len][2] = the transform of the
   conjugate chirp as stored -- divided by conv_len, in the order the forward passes leave their output (tools/anyfft_emul.py
   restates it), both rounded to fp32. */
int dsp_debug_plan_transform_tables(const dsp_plan* plan, int32_t* radix, int32_t radix_cap, int32_t* n_pass, float* h_chirp,
                                    float* h_chirp_spec);
int dsp_plan_destroy(dsp_plan* plan);
/* 1 if the plan is served by a specialised fused kernel (NFFT = 512 or 1536), 0 if only by the generic one */
int dsp_plan_has_fast_path(const dsp_plan* plan);
/* testing aid: route the calling THREAD's feature / VAD / pitch calls through the generic kernels even when a
   specialised one applies (thread-local flag: other threads are unaffected; the kernels are independent
   implementations and must agree) */
int dsp_debug_force_generic(int on);
/* The matrix-pipe NFFT = 512 kernel (csrc/kernels_mfma512.h: the DFT, the mel filterbank and the DCT of
   sigproc.py:136-158 / base.py:8-32 as fp16 / bf16 (hi, lo) products on v_mfma_f32_16x16x32) is an OPT-IN path for
   dense batches: on = 1 routes the calling thread's dsp_features_batch(MFCC) / dsp_mfcc_delta_batch calls to it when it
   serves the plan and the batch, 2 to its frame-per-product form (csrc/kernels_mfma512t.h: one register-resident matrix
   per DFT stage, window and twiddle on the vector pipe), 0 keeps them on the vector-pipe kernels, -1 follows the
   environment (DSP_MFMA512=1 / 2). */
int dsp_debug_use_mfma512(int on);
/* bit 0: the plan has tables for kernels_mfma512.h (NFFT = 512, hop 160, <= 47 filters in the supported block pattern);
   bit 1: for kernels_mfma512t.h (NFFT = 512, hop 160, <= 47 filters) */
int dsp_plan_has_mfma512(const dsp_plan* plan);
/* testing aid: device workspaces (index tables, cepstra scratch) the library's pool currently holds */
int dsp_debug_pool_stats(long long* n_buffers, long long* bytes);
/* on = 1: dsp_plan_create on the calling thread runs every host-side table builder (window / twiddle / mel / DCT tables,
   the fused kernels' and the matrix-pipe kernels' operand tables) but keeps the tables in HOST memory and never touches a
   device -- for the sanitizer build (`make -C dsp-speech-recognition_amd/csrc asan`, tests/test_host_asan.py), which runs
   on a machine without a GPU.  Such a plan can only be destroyed; launches with it are refused. */
int dsp_debug_host_dry_run(int on);
/* testing aid: which kernel family dsp_vad_features_batch / dsp_vad_features_layout_batch launch for this framing, sample
   type and use_sq on the calling thread -- the launcher switches on the very function this returns, so the answer cannot
   drift from what runs.  Returns one of the codes below (or DSP_EINVAL for frame_len / frame_step < 1 or an unknown
   wave_dtype) and writes the frames one wavefront takes at a time (1, 4, 8 or 16) to *frames_per_wave (may be NULL).
   Touches no device.  Honours dsp_debug_force_generic.  A batch the vector kernels cannot read (more than 2^30 groups)
   still takes the per-frame kernel; misaligned buffers and dense batches with N % 4 != 0 keep their route (they are
   launched as ragged batches of an aligned buffer). */
#define DSP_VAD_ROUTE_PER_FRAME 0 /* vad_features_kernel: one wavefront per frame, any framing */
#define DSP_VAD_ROUTE_SCAN 1      /* vad_scan_kernel: int16, sum |x|, integer prefix sums */
#define DSP_VAD_ROUTE_SUM 2       /* vad_sum_kernel: frame_len and frame_step multiples of 4 */
#define DSP_VAD_ROUTE_TILE_ABS 3  /* vad_tile_kernel, fp64 sums of |x|: fp32 input */
#define DSP_VAD_ROUTE_TILE_SQ 4   /* vad_tile_kernel, fp64 sums of x^2: either input */
int dsp_debug_vad_route(int32_t frame_len, int32_t frame_step, int wave_dtype, int32_t use_sq, int32_t* frames_per_wave);

/* ---- the hot path -------------------------------------------------------------------------- */
/*
 * y[0]=x[0]; y[n]=x[n]-coeff*x[n-1] per utterance.        sigproc.preemphasis  sigproc.py:178-185
 */
int dsp_preemphasis_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                          int32_t n_utt, int64_t n_samples_total, float coeff, float* d_out,
                          void* stream);

/*
 * Fused pre-emphasis -> framing*window -> rFFT -> |X|^2/NFFT -> mel -> log -> DCT*lifter -> energy
 * swap, stopping at `out_kind`.  Replaces sigproc.preemphasis/framesig/magspec/powspec and
 * base.fbank/mfcc (sigproc.py:66-98,136-158,178-185; base.py:8-32).
 *   uniform_samples > 0: every utterance has exactly that many samples (offsets may then be NULL).
 *   d_out2: energy[sumT] for DSP_OUT_FBANK, else ignored (may be NULL).
 *   ld_out: row stride of d_out in floats (0 = dense).
 */
int dsp_features_batch(const dsp_plan* plan, const void* d_wave, int wave_dtype,
                       const int64_t* d_sample_offsets, const int64_t* d_frame_offsets,
                       int32_t n_utt, int64_t n_frames_total, int64_t uniform_samples,
                       int out_kind, float* d_out, int64_t ld_out, float* d_out2, void* stream);

/*
 * d[t] = sum_{n=-N..N} n * x[clamp(t+n)] / (2 sum i^2), edge-replicated per utterance.
 *                                                                base.delta  base.py:70-79
 * Reads columns [0,D) of d_in (row stride ld_in), writes columns [0,D) of d_out (row stride ld_out).
 * If d_out_dd != NULL also writes delta(delta(x)) there in the same pass (model.py:76-77 pattern).
 *   uniform_frames > 0: every utterance has exactly that many frames (offsets may be NULL).
 */
int dsp_delta_batch(const float* d_in, int64_t ld_in, const int64_t* d_frame_offsets,
                    int32_t n_utt, int64_t n_frames_total, int64_t uniform_frames, int32_t D,
                    int32_t N, float* d_out, int64_t ld_out, float* d_out_dd, int64_t ld_out_dd,
                    void* stream);

/*
 * BASELINE config 2 in one call: out[sumT, 3C] = mfcc | delta_N | delta_N(delta_N).
 *                                        base.mfcc + base.delta x2   base.py:8-16,70-79
 */
int dsp_mfcc_delta_batch(const dsp_plan* plan, const void* d_wave, int wave_dtype,
                         const int64_t* d_sample_offsets, const int64_t* d_frame_offsets,
                         int32_t n_utt, int64_t n_frames_total, int64_t uniform_samples,
                         int32_t delta_n, float* d_out, void* stream);

/* c[:, n] *= lift[n]                                           base.lifter  base.py:60-68 */
int dsp_scale_columns(float* d_x, int64_t rows, int32_t cols, const float* d_scale, void* stream);

/* ---- endpointing (energy / ZCR) ------------------------------------------------------------ */
/*
 * Per frame of length L / hop S (rectangular window, sizes truncated by the caller as
 * sigproc.to_frames does, sigproc.py:11-19):
 *   amp_sum[t] = sum |x| (or sum x^2)   -> endpoint.get_amplitude = amp_sum / L   endpoint.py:109-126
 *   zcr[t]     = #{ i : x[i]*x[i+1] < 0 }, sign-pair test                         endpoint.py:182-198
 * fp64 accumulation; exact for int16 input.
 */
int dsp_vad_features_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                           const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total,
                           int64_t uniform_samples, int32_t frame_len, int32_t frame_step,
                           int32_t use_sq, double* d_amp_sum, int32_t* d_zcr, void* stream);

/*
 * The two-threshold state machine, one utterance per thread, fp64 thresholds:
 * endpoint.amplitude_rule (endpoint.py:133-179, use_acr=False), the mh=0.125 retry and the
 * <50-frame fallbacks of endpoint.basic_endpoint_detection (endpoint.py:42-62), endpoint.zcr_rule
 * (endpoint.py:201-220).  cfg_frame/cfg_step are the reference's cfg.frame / cfg.step.
 * Writes frame indices (left2,right2) per utterance to d_endpoints[2*b .. 2*b+1]; the caller maps
 * them to samples with int(left*cfg.step*rate) in fp64 (endpoint.py:64).
 */
int dsp_endpoint_rule_batch(const double* d_amp_sum, const int32_t* d_zcr,
                            const int64_t* d_frame_offsets, int32_t n_utt, int32_t frame_len,
                            double cfg_frame, double cfg_step, int32_t* d_endpoints, void* stream);

/*
 * endpoint.robust_endpoint_detection (endpoint.py:68-92), batched, in two calls.
 *
 * dsp_acr_gate_batch: the autocorrelation gate acr_rule of endpoint.amplitude_rule (endpoint.py:142-144) for EVERY frame
 * of the rectangular to_frames framing (sigproc.py:11-19): d_voiced[g] = 1 when
 *     max_{n in [lag_lo, lag_hi)} sigproc.acr(frame, n) / sigproc.acr(frame, 0) > thresh        (sigproc.py:48-53)
 * -- the caller passes lag_lo = rate // 500, lag_hi = rate // 50, thresh = 0.55 -- accumulated in fp64 (exact for
 * int16 PCM).  Same batch conventions as dsp_vad_features_batch; lags must not exceed frame_len.
 *
 * dsp_endpoint_rule_acr_batch: dsp_endpoint_rule_batch's state machine in the robust form -- amplitude_rule with
 * mh = 0.5 and use_acr=True (a segment only grows over frames whose d_voiced bit is set, endpoint.py:168-170), one
 * pass (no mh = 0.125 retry), then zcr_rule and the < 50-frame fallback (endpoint.py:73-90).
 */
int dsp_acr_gate_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                       const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total, int64_t uniform_samples,
                       int32_t frame_len, int32_t frame_step, int32_t lag_lo, int32_t lag_hi, double thresh,
                       uint8_t* d_voiced, void* stream);
int dsp_endpoint_rule_acr_batch(const double* d_amp_sum, const int32_t* d_zcr, const uint8_t* d_voiced,
                                const int64_t* d_frame_offsets, int32_t n_utt, int32_t frame_len, double cfg_frame,
                                double cfg_step, int32_t* d_endpoints, void* stream);

/*
 * Batch-layout handle: the index tables a ragged call would otherwise build with a small launch of its own (into a
 * pooled workspace) on EVERY call, built ONCE for a batch shape -- the frame offsets of `frame_len` / `frame_step`
 * framing of n_utt utterances.  dsp_vad_features_layout_batch is dsp_vad_features_batch with those tables: no table
 * launch, no pooled workspace, so the call can be captured into a HIP graph.  (The feature stage of configs[3] has
 * data-dependent offsets -- the trimmed clips -- and keeps its tables in the caller's work buffer instead:
 * dsp_endpoint_layout_segments_batch.)  The tables are built on `stream`; the handle belongs to the current device.
 */
typedef struct dsp_layout dsp_layout;
int dsp_layout_create(const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total, int32_t frame_len,
                      int32_t frame_step, void* stream, dsp_layout** out);
int dsp_layout_destroy(dsp_layout* layout);
int dsp_vad_features_layout_batch(const dsp_layout* layout, const void* d_wave, int wave_dtype,
                                  const int64_t* d_sample_offsets, const int64_t* d_frame_offsets, int32_t use_sq,
                                  double* d_amp_sum, int32_t* d_zcr, void* stream);

/*
 * A batch layout built ON THE DEVICE, so that a recorded launch sequence serves clips of any lengths.
 *
 * dsp_batch_offsets_batch (one launch, one workgroup, no atomics, no memset, capturable) reads the caller's [n_utt + 1]
 * sample offsets from device memory and writes
 *   d_sample_offsets   the sanitised copy: out[0] = 0, out[b + 1] = clamp(in[b + 1], out[b], sample_capacity) -- whatever
 *                      the caller wrote, it is monotone and inside the sample_capacity samples of the wave buffer; later
 *                      kernels read this table only (it must not be the caller's table);
 *   d_frame_offsets[f] per framing f < n_framings <= 4 (frame_len / frame_step / d_frame_offsets are HOST arrays, the
 *                      tables device memory): the exclusive prefix sum of dsp_frame_count over the sanitised lengths,
 *                      equal to dsp_frame_offsets in every integer;
 *   d_status           one int32, overwritten: bit 0 in[0] != 0, bit 1 a decreasing pair, bit 2 an offset above the
 *                      capacity, bit 3 a clip of 0 samples (in[b + 1] == in[b]).
 *
 * dsp_layout_create_capacity allocates the index tables of a dsp_layout for ANY batch of n_utt clips with at most
 * n_frames_bound frames (dsp_frames_bound) and builds nothing; dsp_layout_refresh rebuilds them on `stream` from the frame
 * offsets dsp_batch_offsets_batch wrote for that framing (no allocation, no synchronisation, capturable; a handle from
 * dsp_layout_create is refused).  dsp_vad_features_layout_batch on such a handle sizes its grid by the bound and stops at
 * the true count in the tables; it never touches the pooled workspace, so what would need it -- a wave buffer that does
 * not start on a vector (16 bytes, 8 for int16) where the framing takes a tile kernel -- is DSP_EINVAL.
 */
int dsp_batch_offsets_batch(const int64_t* d_sample_offsets_in, int32_t n_utt, int64_t sample_capacity, int32_t n_framings,
                            const int32_t* frame_len, const int32_t* frame_step, int64_t* d_sample_offsets,
                            int64_t* const* d_frame_offsets, int32_t* d_status, void* stream);
int dsp_layout_create_capacity(int32_t n_utt, int64_t n_frames_bound, int32_t frame_len, int32_t frame_step, dsp_layout** out);
int dsp_layout_refresh(dsp_layout* layout, const int64_t* d_frame_offsets, void* stream);

/*
 * Endpoint-trimmed copy (fp32 out): utterance b keeps samples [segments[2b], segments[2b+1]) relative
 * to its start and lands at d_dst_offsets[b]; with unit_variance != 0 it is divided by its population
 * standard deviation (zero -> 1), i.e. sig[left:right] -> sklearn scale(with_mean=False) as
 * model.py:62-63 does before feature extraction.  fp64 statistics.
 */
int dsp_trim_scale_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets,
                         const int64_t* d_segments, const int64_t* d_dst_offsets, int32_t n_utt,
                         int32_t unit_variance, float* d_out, void* stream);

/*
 * configs[3] without the trimmed copy: MFCC | delta | delta-delta of sig[left:right] for every utterance of a ragged
 * batch, READ IN PLACE -- model.py:113-121 (endpoint_detect -> scale -> feature_extract_mfcc) without writing and
 * re-reading an fp32 copy of every clip.  d_segments = int64 [B, 2] (left, right) relative to each utterance's start
 * (dsp_endpoint_layout_batch writes them), d_frame_offsets = the frame prefix of the TRIMMED clips (same call),
 * n_frames_bound >= their total.  unit_variance != 0: the clip counts as divided by its population standard deviation
 * (sklearn scale(with_mean=False), model.py:62-63) -- computed as what that scaling does to the result: it adds
 * -ln(var) to c0 = log(energy) and leaves every other cepstrum, delta and delta-delta unchanged; var comes from fp64
 * sums the MFCC kernel accumulates while it stages the samples.  d_work: caller-owned scratch of
 * dsp_segments_workspace_bytes() bytes (tables, statistics, dense cepstra): no pooled workspace, no allocation, the call
 * is a fixed sequence of three launches on `stream` and can be captured into a HIP graph.
 * Served by the NFFT = 512 AND the NFFT = 1536 fused kernels (the size model.py:74 uses).  delta_n = 0: cepstra only,
 * written straight to d_out [sum T, C] (model.py:66-88 wants delta(3) of the MEAN-REMOVED cepstra, which is
 * dsp_model_finalize_segments_batch's job); with DSP_SEG_UNIT_VARIANCE the c0 column then still lacks its -ln(var) --
 * the statistics stay at the start of d_work and dsp_model_finalize_segments_batch applies the shift as it reads.
 * Returns 1 (not an error) when the plan / buffer is not served in place (no fused kernel, misaligned buffer,
 * unit variance without appendEnergy): use dsp_trim_scale_batch + dsp_mfcc_delta_batch then.
 */
#define DSP_SEG_UNIT_VARIANCE 1   /* flags: the clips count as divided by their standard deviation (see above) */
#define DSP_SEG_TABLES_READY 2    /* flags: d_work already holds the tables (dsp_endpoint_layout_segments_batch) */
int dsp_segments_workspace_bytes(const dsp_plan* plan, int32_t n_utt, int64_t n_frames_bound, size_t* bytes);
int dsp_mfcc_delta_segments_batch(const dsp_plan* plan, const void* d_wave, int wave_dtype,
                                  const int64_t* d_sample_offsets, const int64_t* d_segments,
                                  const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_bound,
                                  int32_t delta_n, int32_t flags, void* d_work, size_t work_bytes,
                                  float* d_out, void* stream);
/*
 * dsp_endpoint_layout_batch (below) for `plan`'s framing that ALSO leaves, in the same launch, everything
 * dsp_mfcc_delta_segments_batch would otherwise build with a launch of its own (frame-group and delta-tile tables of the
 * trimmed clips, zeroed statistics) in d_work: pass DSP_SEG_TABLES_READY to that call then.
 */
int dsp_endpoint_layout_segments_batch(const int32_t* d_endpoints, const int64_t* d_sample_offsets, int32_t n_utt,
                                       double cfg_step, double rate, const int64_t* d_jitter, int64_t* d_segments,
                                       int64_t* d_dst_offsets, int64_t* d_frame_offsets, const dsp_plan* plan,
                                       int64_t n_frames_bound, void* d_work, size_t work_bytes, void* stream);

/*
 * Device-side glue between dsp_endpoint_rule_batch and dsp_trim_scale_batch / dsp_features_batch, so that
 * the endpoint -> trim -> features pipeline of model.py:113-121 needs no host round trip:
 *   d_segments[2b], [2b+1] = int((left * cfg.step) * rate), int((right * cfg.step) * rate) in fp64, that
 *                            order, truncated (endpoint.py:64), clipped to the clip length as numpy slicing
 *                            sig[left:right] does (model.py:62); with d_jitter != NULL the per-utterance
 *                            offsets d_jitter[2b] (added to left, i.e. -s_l) and d_jitter[2b+1] (+s_r) of
 *                            model.py:54-60 are applied first and negatives raised to 0;
 *   d_dst_offsets[B+1]     = exclusive prefix of the trimmed lengths;
 *   d_frame_offsets[B+1]   = exclusive prefix of their frame counts at (frame_len, frame_step).
 * Ragged feature calls that follow may pass an upper bound as n_frames_total (e.g. the frame count of the
 * untrimmed clips): kernels take the true totals from d_frame_offsets.
 */
int dsp_endpoint_layout_batch(const int32_t* d_endpoints, const int64_t* d_sample_offsets, int32_t n_utt,
                              double cfg_step, double rate, int32_t frame_len, int32_t frame_step,
                              const int64_t* d_jitter, int64_t* d_segments, int64_t* d_dst_offsets,
                              int64_t* d_frame_offsets, void* stream);

/* ---- model.py glue behind the feature call ----------------------------- */
/*
 * What model.py:66-88 does to mfcc0 = mfcc(...) of every utterance, and the [200, B, 39] layout of
 * model.py:35-50,131-135, in one launch:
 *   x  = mfcc0 - mean(mfcc0)             scalar mean of the utterance's [T, C] block   model.py:75
 *   d1 = delta(x, N); d2 = delta(d1, N)  base.delta, edge replicated                  model.py:76-77
 *   z  = (x - mean_c) / std_c            per coefficient, population std, 0 -> 1       model.py:78
 *   d_out[t, b, 0:C | C:2C | 2C:3C] = z | d1 | d2 for t < min(T_b, max_len), zero rows up to max_len
 *   d_len0[b] = min(T_b, max_len)
 * d_mfcc: [sum T_b, C] (row stride ld_in, 0 = dense); d_out: [max_len, n_utt, 3C] fp32.
 * Statistics are accumulated in fp64.
 */
int dsp_model_finalize_batch(const float* d_mfcc, int64_t ld_in, const int64_t* d_frame_offsets,
                             int32_t n_utt, int32_t C, int32_t N, int32_t max_len, float* d_out,
                             int32_t* d_len0, void* stream);

/*
 * Optional amplitude stream of model.py:97-101 (cfg.use_timefeat), batched: d_amp_sum = per-frame sums of
 * |x| of the trimmed, scaled clips (dsp_vad_features_batch at frame_len = int(rate * cfg.frame)), one run of
 * frames per utterance.  Writes d_out[max_len, n_utt, 2]: column 0 = the z-scored frame amplitude
 * (endpoint.amplitude_feature, endpoint.py:128-131, through sklearn scale: population std, 0 -> 1), column 1 =
 * its first difference (model.py:29-33, T - 1 rows), both zero padded / truncated to max_len (model.py:35-50).
 */
/* dsp_model_finalize_batch for cepstra of segments read in place (dsp_mfcc_delta_segments_batch, delta_n = 0, same
   d_segments and d_work): with the unit-variance statistics in d_work, c0 gets its -ln(var) (model.py:62-63) at every
   read -- frames of exactly zero energy keep ln(eps), base.py:26 -- before the mean, the deltas and the z-score. */
int dsp_model_finalize_segments_batch(const float* d_mfcc, int64_t ld_in, const int64_t* d_frame_offsets,
                                      const int64_t* d_segments, const void* d_work, int32_t n_utt, int32_t C, int32_t N,
                                      int32_t max_len, float* d_out, int32_t* d_len0, void* stream);
int dsp_model_timefeat_batch(const double* d_amp_sum, const int64_t* d_frame_offsets, int32_t n_utt,
                             int32_t frame_len, int32_t max_len, float* d_out, void* stream);

/* ---- pitch scores ------------------------------------------------------ */
/*
 * Per frame of the (already 10 kHz) signal, rectangular frames of frame_len / hop frame_step as
 * sigproc.to_frames cuts them:
 *   centre clipping at the median of the non-negative samples (if center_clip != 0)
 *                                                         pitch.center_clip      pitch.py:145-155
 *   y = convolve(frame, taps)[:frame_len], f = |y|        sigproc.window         sigproc.py:22-46
 *   scores[t, n - lag_min] = sum_i f[i] f[i+n] / (frame_len - n), lag_min <= n < lag_max
 *                                                         sigproc.acr            sigproc.py:48-53
 * i.e. pitch.pitch_detect_frame_sr (pitch.py:112-132) for every frame of pitch.pitch_detect_sr
 * (pitch.py:96-107).  d_sig: fp32; d_taps: frame_len complex taps (re, im interleaved), built by the
 * host in fp64; d_scores: [sum T_b, lag_max - lag_min] fp32.  frame_len <= 1024.
 */
int dsp_pitch_scores_batch(const float* d_sig, const int64_t* d_sample_offsets,
                           const int64_t* d_frame_offsets, int32_t n_utt, int64_t n_frames_total,
                           int64_t uniform_samples, int32_t frame_len, int32_t frame_step,
                           const float* d_taps, int32_t center_clip, int32_t lag_min, int32_t lag_max,
                           float* d_scores, void* stream);

/*
 * The tracker behind those scores, for a whole batch (one wavefront per utterance, fp64): pitch.smooth in place
 * (pitch.py:157-164: running mean over rows [i - 2, i + 2) of which the first two are already smoothed; the
 * reference's end-of-utterance window and its empty mean for a one-frame utterance included), pitch.max_pitch
 * (pitch.py:166-172: first arg-max, 1 / (1e-4 (bias + idx))) and the two octave-repair sweeps of
 * pitch.robust_max_pitch (pitch.py:191-206).  d_scores: [sum T_b, n_lags] fp32 as dsp_pitch_scores_batch writes
 * them; d_pitch: [sum T_b] fp64, Hz per frame.  degree must be 2 (the only value the reference uses).
 */
int dsp_pitch_track_batch(const float* d_scores, const int64_t* d_frame_offsets, int32_t n_utt, int32_t n_lags,
                          int32_t bias, int32_t degree, double* d_pitch, void* stream);

/*
 * The tracker's parts on fp64 score rows [sum T_b, n_lags] (what the reference's helpers take): flags bit 0 =
 * pitch.smooth(g, degree) in place (pitch.py:157-164), bit 1 = pitch.max_pitch (pitch.py:166-172) into d_pitch, bit 2 =
 * the octave-repair sweeps of pitch.robust_max_pitch (pitch.py:191-206; needs bit 1).  d_rows is overwritten by the
 * smoothed rows when bit 0 is set.
 */
int dsp_pitch_rows_batch(double* d_rows, const int64_t* d_frame_offsets, int32_t n_utt, int32_t n_lags, int32_t bias,
                         int32_t degree, int32_t flags, double* d_pitch, void* stream);

/*
 * Device-side glue of the optional streams of model.py:90-101 (no clip leaves the device):
 *   dsp_resample_layout_batch  from the sample offsets of a batch: with dst_rate > 0 the lengths preprocess.downsampling
 *                              (preprocess.py:21-28) leaves of every clip and their exclusive prefix d_dst_offsets[B+1];
 *                              always the exclusive prefix d_frame_offsets[B+1] of the frame counts of the (decimated)
 *                              clips at (frame_len, frame_step) (sigproc.py:79-82).  dst_rate = 0: frame offsets only.
 *   dsp_decimate_batch         the kept samples themselves (the k-th kept index is the first i with
 *                              i * dst_rate / src_rate > k - 1 + 1e-8, the reference's fp64 test); n_out_bound is an
 *                              upper bound of the output length (e.g. the input length), the true total is
 *                              d_dst_offsets[n_utt].
 *   dsp_model_pitchfeat_batch  [max_len, B, 2] = pitch / 150 and its first difference, zero padded (model.py:90-95,
 *                              35-50), from dsp_pitch_track_batch's d_pitch.
 */
int dsp_resample_layout_batch(const int64_t* d_src_offsets, int32_t n_utt, int64_t src_rate, int64_t dst_rate,
                              int32_t frame_len, int32_t frame_step, int64_t* d_dst_offsets, int64_t* d_frame_offsets,
                              void* stream);
int dsp_decimate_batch(const float* d_in, const int64_t* d_src_offsets, const int64_t* d_dst_offsets, int32_t n_utt,
                       int64_t n_out_bound, int64_t src_rate, int64_t dst_rate, float* d_out, void* stream);
int dsp_model_pitchfeat_batch(const double* d_pitch, const int64_t* d_frame_offsets, int32_t n_utt, int32_t max_len,
                              float* d_out, void* stream);

/* ---- cepstral pitch and the five pitch features (pitch.pitch_detect, pitch.pitch_feature) --- */
/*
 * Per frame of the (already 10 kHz) signal, rectangular frames as sigproc.to_frames cuts them, one launch:
 *   centre clipping at the median of the non-negative samples, non-binary (if center_clip != 0)
 *                                                                    pitch.center_clip       pitch.py:145-155
 *   y = convolve(frame, taps)[:frame_len], kept complex              sigproc.window          sigproc.py:22-46
 *   d_rows[t] = |ifft(log|fft(y)|)|                                  pitch.pitch_detect_frame pitch.py:135-143
 *   d_amp[t]  = sum |x| of the unclipped frame (fp64, optional)      pitch.sub_endpoint_detect pitch.py:65
 * i.e. the loop body of pitch.pitch_detect (pitch.py:86-90).  Geometry arguments as dsp_pitch_scores_batch; d_taps:
 * frame_len complex taps (re, im interleaved) of the 50 - 1000 Hz band (pitch.py:137); d_rows: [sum T_b, frame_len]
 * fp32.  frame_len must be a power of two in [128, 1024] (0.0512 s at 10 kHz is 512); anything else is DSP_EINVAL.
 * A silent frame gives [inf, nan, nan, ...], as the reference.
 */
int dsp_pitch_cepstrum_batch(const float* d_sig, const int64_t* d_sample_offsets, const int64_t* d_frame_offsets,
                             int32_t n_utt, int64_t n_frames_total, int64_t uniform_samples, int32_t frame_len,
                             int32_t frame_step, const float* d_taps, int32_t center_clip, float* d_rows, double* d_amp,
                             void* stream);

/*
 * The tracker behind those rows (one wavefront per utterance, fp64; pitch.py:91-93).  flags bit 0 = pitch.smooth(rows, 2)
 * with the reference's in-place habits (pitch.py:157-164; d_rows itself is not written); the peak-width scores of
 * pitch.peak_score (pitch.py:227-242: 80 integers per frame, candidates 20 .. 99) are always formed and written to
 * d_scores [sum T_b, 80] when it is not NULL; flags bit 1 = pitch.robust_max_pitch(scores, 20) (pitch.py:166-172,
 * 191-206) into d_pitch [sum T_b] fp64.  With both bits clear only the scores of the rows as given are written.
 * d_rows: [sum T_b, frame_len], fp32 as dsp_pitch_cepstrum_batch writes them, or fp64 when rows_f64 != 0.
 */
int dsp_pitch_cepstrum_track_batch(const void* d_rows, int32_t rows_f64, const int64_t* d_frame_offsets, int32_t n_utt,
                                   int32_t frame_len, int32_t flags, double* d_pitch, int32_t* d_scores, void* stream);

/*
 * The tail of pitch.pitch_feature (pitch.py:34-47), one wavefront per utterance, fp64: p = sub_endpoint_detect
 * (pitch.py:64-81) from d_amp, p_bias = 5 if p > 15 else 0, find_smooth_subsequence (pitch.py:245-279, tor 3, thres 30)
 * on pitch[p_bias:p] and pitch[p:], then slope, quad_params and peakshift (pitch.py:49-62).
 *   d_feat [n_utt, 5] fp64   slope1, slope2, quad1, quad2, peakshift
 *   d_aux  [n_utt, 9] int32  p, p_bias, start1, end1, start2, end2, len1, len2, valid
 *   d_seg  [sum T_b]  fp64   the accepted values: segment 1 from frame p_bias of the utterance, segment 2 from frame p
 * A segment shorter than 3 values (the reference raises, or fits a rank-deficient system) gives valid = 0 and a NaN row.
 * d_pitch == NULL: only p is computed and written (d_aux[b, 0]); d_seg and d_feat may then be NULL.
 */
int dsp_pitch_feature_batch(const double* d_pitch, const double* d_amp, const int64_t* d_frame_offsets, int32_t n_utt,
                            double* d_seg, double* d_feat, int32_t* d_aux, void* stream);

/*
 * pitch.find_smooth_subsequence (pitch.py:245-279) on its own: d_values [sum n_b] fp64 with offsets d_offsets [B+1];
 * the accepted values of the longest segment (the first one on a tie) go to d_seg[d_offsets[b] ..], and
 * d_info[b] = (start, end, count), indices within the sequence.  An empty sequence has count 0.  tor >= 1.
 */
int dsp_pitch_smooth_subseq_batch(const double* d_values, const int64_t* d_offsets, int32_t n_utt, int32_t tor,
                                  double thres, double* d_seg, int32_t* d_info, void* stream);

/* ---- the HMRNN classifier's recurrence (hmrnn.HM_LSTM, the `enc2` of rnn_clf.HMRNN) --------- */
/*
 * Forward pass of hmrnn.HM_LSTM (hmrnn.py:114-154) over its two hmrnn.HM_LSTMCell (hmrnn.py:73-111), fp32, for a whole
 * batch in ONE persistent launch (csrc/kernels_hmlstm.h): a workgroup owns 16 batch columns for all T steps and never
 * waits on another one.
 *
 * The desc carries DEVICE pointers to the seven parameters in the reference's own row-major layout (hmrnn.py:60-64):
 *   cell_1: U_11 [4 H1 + 1, H1], U_21 [4 H1 + 1, H2], W_01 [4 H1 + 1, input_size], bias [4 H1 + 1]
 *   cell_2: U_11 [4 H2 + 1, H2],                      W_01 [4 H2 + 1, H1],         bias [4 H2 + 1]
 * (rows f | i | o | g | z, hmrnn.py:86-90).  input_size, hidden1 and hidden2 are independent, each a multiple of 4 in
 * [4, 256]; anything else is DSP_EINVAL, checked before any device call.  Create repacks the parameters into the
 * kernel's layout on the current device (it waits for the device before and after, so it must not run inside a stream
 * capture); the handle holds its own copy, is immutable afterwards and may be used from several streams.
 */
typedef struct dsp_hmlstm dsp_hmlstm;
typedef struct dsp_hmlstm_desc {
    int32_t input_size, hidden1, hidden2;
    int32_t reserved;
    const float* d_c1_U11;
    const float* d_c1_U21;
    const float* d_c1_W01;
    const float* d_c1_bias;
    const float* d_c2_U11;
    const float* d_c2_W01;
    const float* d_c2_bias;
} dsp_hmlstm_desc;
int dsp_hmlstm_create(const dsp_hmlstm_desc* desc, dsp_hmlstm** out);
int dsp_hmlstm_destroy(dsp_hmlstm* h);
/*
 * d_x [T, B, input_size] fp32, 16-byte aligned.  a: the slope of hard_sigm (hmrnn.py:25-28,90), per call because
 * rnn_clf.HMRNN.adjust_param (rnn_clf.py:163-164) changes it between epochs.  d_len [B] int32 or NULL (= T everywhere;
 * values are clamped to [1, T]).  d_state_in / d_state_out: the reference's `hidden` tuple (hmrnn.py:130-138,153) as one
 * fp32 buffer  h1 [H1, B] | c1 [H1, B] | z1 [B] | h2 [H2, B] | c2 [H2, B] | z2 [B];  d_state_in == NULL means zeros, and
 * the two may be the same buffer.  Every output may be NULL (not all of them):
 *   d_h1 [B, T, H1], d_h2 [B, T, H2]   hmrnn.py:148-149,154
 *   d_z1, d_z2 [B, T] uint8            the boundary bits, hmrnn.py:150-151
 *   d_zhat [T, 2, B] fp32              hard_sigm in front of the threshold (cell 1, cell 2), hmrnn.py:90
 *   d_last_h2 [B, H2]                  h_2[b, len[b] - 1], rnn_clf.py:140-143
 * All T steps are run for every column -- except when d_last_h2 (with d_len) is the ONLY output: nothing behind a column's
 * length reaches it, so each 16-column slice then stops at the longest length among its columns (same bits in d_last_h2).
 * One launch on `stream`, no workspace, no allocation: the call can be captured into a HIP graph.
 */
int dsp_hmlstm_forward(const dsp_hmlstm* h, const float* d_x, int32_t T, int32_t B, float a, const int32_t* d_len,
                       const float* d_state_in, float* d_state_out, float* d_h1, float* d_h2, uint8_t* d_z1,
                       uint8_t* d_z2, float* d_zhat, float* d_last_h2, void* stream);

/*
 * Training mode of the same recurrence: a forward that also saves what the backward pass needs (the "tape"), and the
 * backward recurrence (csrc/kernels_hmlstm_bwd.h, one persistent launch of the same shape).  dsp_hmlstm_create packs a
 * second, transposed copy of the four recurrent / bottom-up matrices for it, so a handle holds about
 * 4 (4 H1 + 1) (input_size + H2 + H1) + 4 (4 H2 + 1) (H1 + H2) bytes for the forward plus, rounded up to whole tiles,
 * 4 (4 H1 + 1) (H1 + H2) + 4 (4 H2 + 1) (H1 + H2) bytes for the backward (1.3 MB + 1.7 MB padded at 200 / 200 / 200).
 *
 * dsp_hmlstm_tape_bytes: the size of the caller's tape buffer at (T, B): ceil(B / 16) T (320 (H1 + H2) + 128) bytes
 * (0.82 GB at T 200, B 512, H 200 / 200).  It holds, per step, cell and (hidden unit, column), the four gates behind
 * their non-linearities and c', and per step, cell and column whether the clamp of hard_sigm passed the gradient.
 *
 * dsp_hmlstm_forward_train: dsp_hmlstm_forward with d_tape (16-byte aligned, at least dsp_hmlstm_tape_bytes; the caller
 * owns it and keeps it and d_h1, d_h2, d_z1, d_z2 -- all four mandatory here -- unchanged until the backward call).
 * Every output is bit for bit what dsp_hmlstm_forward writes.
 *
 * dsp_hmlstm_backward: given the gradients of a loss with respect to h_1 (d_g_h1 [B, T, H1]), h_2 (d_g_h2 [B, T, H2]) and
 * last_h2 (d_g_last [B, H2], added at t = clamp(len[b], 1, T) - 1) -- each may be NULL, not all three -- it runs the steps
 * t = T - 1 .. 0 and writes the gradients of the two cells' pre-activations f_s (hmrnn.py:84, rows f | i | o | g | z):
 *   d_dfs1 [T, B, 4 H1 + 1], d_dfs2 [T, B, 4 H2 + 1]      every element is written; the same bits on every call.
 * T, B, a, d_len and d_state_in must be those of the forward call.  The boundary z = [z_hat > 0.5] hands the gradient
 * through unchanged (hmrnn.py:37-45) and hard_sigm's clamp passes it where 0 <= (a f_s[4H] + 1) / 2 <= 1.  The
 * gradients of x and of the parameters are GEMMs over dfs, left to the caller (K = T B; features/classifier.py::
 * hm_param_grads does them with torch.matmul).  With d1 = dfs1 and d2 = dfs2 as [T B, rows], x as [T B, input_size],
 * h1 / h2 / z1 the forward's outputs of step t and h1' / h2' / z1' those of step t - 1 (d_state_in or zeros at t = 0):
 *   dx       = d1 W_01(1)                                     [T B, input_size]
 *   dW_01(1) = d1^T x          dU_11(1) = d1^T h1'            dU_21    = (z1' d1)^T h2'        dbias(1) = sum of d1's rows
 *   dW_01(2) = d2^T h1         dU_11(2) = (z1 d2)^T h2'                                        dbias(2) = sum of d2's rows
 * Neither call differentiates with respect to the initial state, and z_1 / z_2 / z_hat / state_out are outputs only.
 * Both are one launch on `stream` without allocation (capturable); bad sizes, NULL or misaligned pointers and a short
 * tape are DSP_EINVAL, checked before any device call.
 *
 * dsp_hmlstm_forward_train_rows / dsp_hmlstm_backward_rows: the same pair under a row bound that lives in device memory.
 * d_rows points at one int32 word r, read by the kernels when they run (never by the host, so a captured graph follows
 * the word) and clamped there to [1, T]; d_rows == NULL is the plain call, bit for bit.  The contract: every buffer keeps
 * its shape and strides of T (the tape and dsp_hmlstm_tape_bytes included), and on the rows t < r the call equals the
 * plain call at T = r on the first r rows of d_x with d_len clamped to r -- d_state_out is the state behind step r - 1,
 * d_last_h2 is h_2[b, min(len[b], r) - 1], steps t < r of the tape -- in every bit.  Behind it exact zeros are written:
 * rows t >= r of d_h1, d_h2, d_z1, d_z2, d_zhat and of d_dfs1, d_dfs2, so every element of every output is still written
 * on every call; the tape's steps t >= r are left alone, and d_x, d_g_h1 and d_g_h2 are not read there.  With r >= the
 * longest length and no gradient behind it this is what the plain pair computes in front of r, without the steps behind.
 * Both passes must be given the same word, unchanged in between.  Argument checks are those of the plain pair.
 */
int dsp_hmlstm_tape_bytes(const dsp_hmlstm* h, int32_t T, int32_t B, int64_t* bytes);
int dsp_hmlstm_forward_train(const dsp_hmlstm* h, const float* d_x, int32_t T, int32_t B, float a, const int32_t* d_len,
                             const float* d_state_in, float* d_state_out, float* d_h1, float* d_h2, uint8_t* d_z1,
                             uint8_t* d_z2, float* d_zhat, float* d_last_h2, void* d_tape, int64_t tape_bytes, void* stream);
int dsp_hmlstm_backward(const dsp_hmlstm* h, int32_t T, int32_t B, float a, const int32_t* d_len, const float* d_state_in,
                        const void* d_tape, int64_t tape_bytes, const float* d_h1, const float* d_h2, const uint8_t* d_z1,
                        const uint8_t* d_z2, const float* d_g_h1, const float* d_g_h2, const float* d_g_last, float* d_dfs1,
                        float* d_dfs2, void* stream);
int dsp_hmlstm_forward_train_rows(const dsp_hmlstm* h, const float* d_x, int32_t T, int32_t B, float a, const int32_t* d_len,
                                  const int32_t* d_rows, const float* d_state_in, float* d_state_out, float* d_h1, float* d_h2,
                                  uint8_t* d_z1, uint8_t* d_z2, float* d_zhat, float* d_last_h2, void* d_tape, int64_t tape_bytes,
                                  void* stream);
int dsp_hmlstm_backward_rows(const dsp_hmlstm* h, int32_t T, int32_t B, float a, const int32_t* d_len, const int32_t* d_rows,
                             const float* d_state_in, const void* d_tape, int64_t tape_bytes, const float* d_h1, const float* d_h2,
                             const uint8_t* d_z1, const uint8_t* d_z2, const float* d_g_h1, const float* d_g_h2,
                             const float* d_g_last, float* d_dfs1, float* d_dfs2, void* stream);

/* ---- the classifiers' encoder (layers.DynamicEncoder, the first stage of every head in rnn_clf.py) --------- */
/*
 * Forward pass of layers.DynamicEncoder (layers.py:42-76), fp32: n_layers bidirectional GRU layers over ragged lengths, the
 * two directions of the last layer summed, zero rows behind each utterance's end (csrc/kernels_bigru.h: one launch per layer,
 * a workgroup owns 16 batch columns of one direction for all steps and never waits on another one, plus one summing launch).
 * Per layer and direction, nn.GRU's parameters weight_ih [3 H, in], weight_hh [3 H, H], bias_ih, bias_hh [3 H], rows r | z | n,
 * in = input_size for layer 0 and 2 H above it:
 *   r = sigmoid(W_ir x + b_ir + W_hr h + b_hr),  z = sigmoid(W_iz x + b_iz + W_hz h + b_hz),
 *   n = tanh(W_in x + b_in + r * (W_hn h + b_hn)),  h' = (1 - z) * n + z * h.
 * Both directions start from h = 0; column b is active at step t iff t < len[b]; an inactive column keeps its h and emits a
 * zero row, so the reverse direction starts its recurrence at len[b] - 1.  No column depends on another one: nothing is
 * sorted or packed.
 *
 * d_params holds 8 DEVICE pointers per layer in nn.GRU's order: weight_ih, weight_hh, bias_ih, bias_hh of the forward
 * direction, then the same four of the reverse direction; row-major as torch holds them.  Sizes out of range or a NULL
 * parameter are DSP_EINVAL, checked before any device call.  Create repacks the parameters on the current device (it waits for
 * the device before and after, so it must not run inside a stream capture); the handle holds its own copy, is immutable
 * afterwards and may be used from several streams.
 */
typedef struct dsp_bigru dsp_bigru;
typedef struct dsp_bigru_desc {
    int32_t input_size;   /* 1 .. 512 */
    int32_t hidden;       /* multiple of 4 in [4, 256] */
    int32_t n_layers;     /* 1 .. 4 */
    int32_t reserved;
    const float* d_params[32];
} dsp_bigru_desc;
int dsp_bigru_create(const dsp_bigru_desc* desc, dsp_bigru** out);
int dsp_bigru_destroy(dsp_bigru* h);
/* bytes of the workspace dsp_bigru_forward needs at (T, B): the [T, B, 2 H] rows between the layers */
int dsp_bigru_workspace_bytes(const dsp_bigru* h, int32_t T, int32_t B, int64_t* bytes);
/*
 * d_x [>= T, B, input_size] fp32 (the first T rows are read; no alignment beyond a float's).  d_len [B] int32 or NULL (= T
 * everywhere; values are clamped to [1, T]).  d_y [T, B, hidden] = forward + reverse of the last layer with exact zero rows at
 * t >= len[b]: every element is written on every call.  d_hn [2 n_layers, B, hidden] in nn.GRU's order (layer-major, forward
 * then reverse): the forward direction's h at len - 1 and the reverse direction's at t = 0.  d_y or d_hn may be NULL, not
 * both.  d_work: the caller's buffer of at least dsp_bigru_workspace_bytes bytes, so that the call allocates nothing and can be
 * captured into a HIP graph.  The same arguments give the same bits on every call.
 */
int dsp_bigru_forward(const dsp_bigru* h, const float* d_x, int32_t T, int32_t B, const int32_t* d_len, float* d_y,
                      float* d_hn, void* d_work, int64_t work_bytes, void* stream);

/*
 * Training mode of the same encoder: a forward that also saves what the backward pass needs (the "tape"), and the backward
 * recurrence of one layer (csrc/kernels_bigru_bwd.h, one launch per layer of the forward's shape, run in the opposite order of
 * the forward's steps).  dsp_bigru_create packs a second, transposed copy of every weight_hh for it (rounded up to whole
 * tiles: 4 H * 32 ceil(H / 128) * 4 bytes per layer and direction, 0.4 MB at H = 200).
 *
 * dsp_bigru_tape_bytes: the size of the caller's tape buffer at (T, B):
 *   n_layers * (T B 2 H  +  2 ceil(B / 16) T 64 H) * 4 bytes        (1.6 GB at 2 layers, T 200, B 512, H 200).
 * It holds, per layer, the [T, B, 2 H] output rows (forward | reverse; EVERY row is written, exact zeros at t >= len[b]) --
 * there is no ping-pong here: the backward reads h of the step before from them and the parameter GEMMs read a layer's input
 * from them -- and behind the rows of all layers, per layer, direction, slice of 16 columns, step and (hidden unit, column), r, z, n
 * behind their non-linearities and n_h = W_hn h + b_hn, the factor r multiplied.  Only the steps a slice visits are stored.
 * dsp_bigru_tape_rows: the byte offset of layer `layer`'s output rows in the tape.
 *
 * dsp_bigru_forward_train: dsp_bigru_forward with d_tape (16-byte aligned, at least dsp_bigru_tape_bytes; the caller owns it and
 * keeps it unchanged until the last backward call) in place of the workspace.  d_drop: NULL, or [n_layers - 1, T, B, 2 H] fp32
 * multipliers (0 or 1 / (1 - p), drawn by the caller): d_drop[l - 1] multiplies the input of layer l >= 1 (nn.GRU's inter-layer
 * dropout).  With d_drop == NULL, d_y and d_hn are bit for bit what dsp_bigru_forward writes; either may be NULL.
 *
 * dsp_bigru_backward, for ONE layer: d_g is the gradient of a loss with respect to the layer's output -- for the top layer
 * (layer == n_layers - 1) that of d_y, [T, B, H], read by both directions (y is their sum); below it [T, B, 2 H], forward |
 * reverse, the dx of the layer above.  d_g_hn [2, B, H]: the gradient with respect to this layer's two rows of d_hn.  h_n of the
 * forward direction is h at len - 1 and stays unchanged through the steps behind it, h_n of the reverse direction is h at
 * t = 0, the last step its forward runs: BOTH are the state the backward recurrence starts from, so d_g_hn seeds dh before the
 * first step it visits (t = max len - 1 of the slice for the forward direction, t = 0 for the reverse one).  Either of d_g and
 * d_g_hn may be NULL, not both.  Per step t < len[b], with dh the gradient of h' and h the state in front of the step (the
 * saved row t - 1, 0 at t = 0, for the forward direction; row t + 1 if t + 1 < len[b], else 0, for the reverse one):
 *   dh += g[t];   dn = dh (1 - z);   dz = dh (h - n);   dn_pre = dn (1 - n^2);
 *   da_r = dn_pre n_h r (1 - r);   da_z = dz z (1 - z);   da_nx = dn_pre;   da_nh = dn_pre r;
 *   dh  = dh z + W_hr^T da_r + W_hz^T da_z + W_hn^T da_nh.
 * A column with t >= len[b] does nothing: dh passes through and its row is exact zeros.  It writes
 *   d_da [T, B, 2, 4 H]   per step, column and direction  da_nx | da_r | da_z | da_nh  (H floats each): floats [0, 3 H) are
 *                         (n | r | z) of the input side, floats [H, 4 H) are (r | z | n) of the hidden side, both contiguous.
 * Every element is written on every call, and the same arguments give the same bits.  T, B and d_len must be those of the
 * forward call.  The gradients of the parameters and of the layer's input are GEMMs over d_da, left to the caller (K = T B;
 * features/classifier.py::gru_param_grads does them with torch.matmul).  With A_i = d_da[.., dir, 0 : 3 H] and
 * A_h = d_da[.., dir, H : 4 H] as [T B, 3 H], x_l the layer's input as the kernel read it (multipliers applied) and h' the
 * state in front of each step as above, per direction:
 *   d weight_ih = (A_i^T x_l, rows n | r | z reordered to r | z | n)      d bias_ih = the column sums of A_i, reordered alike
 *   d weight_hh =  A_h^T h'                                              d bias_hh = the column sums of A_h
 *   d x_l       = the sum over the two directions of A_i (weight_ih, rows reordered to n | r | z), times d_drop[l - 1] where
 *                 there are multipliers: the d_g of the layer below, or the gradient of d_x.
 * The caller interleaves the layers, top down, with these GEMMs.  Each call is launches on `stream` without allocation
 * (capturable); bad sizes, a layer out of range, NULL or misaligned pointers, no gradient at all and a short tape are
 * DSP_EINVAL, checked before any device call.
 */
int dsp_bigru_tape_bytes(const dsp_bigru* h, int32_t T, int32_t B, int64_t* bytes);
int dsp_bigru_tape_rows(const dsp_bigru* h, int32_t layer, int32_t T, int32_t B, int64_t* offset_bytes);
int dsp_bigru_forward_train(const dsp_bigru* h, const float* d_x, int32_t T, int32_t B, const int32_t* d_len, const float* d_drop,
                            float* d_y, float* d_hn, void* d_tape, int64_t tape_bytes, void* stream);
int dsp_bigru_backward(const dsp_bigru* h, int32_t layer, int32_t T, int32_t B, const int32_t* d_len, const void* d_tape,
                       int64_t tape_bytes, const float* d_g, const float* d_g_hn, float* d_da, void* stream);

/* ---- the ensemble: pitch SVM and confidence gate (ensemble.EnsembleModel.test ensemble.py:44-67, PitchModel.test_iter pitch_model.py:54-61) ---- */
/*
 * A fitted RobustScaler + SVC(kernel='rbf') pair as its public attributes (pitch_model.py:23-24,59-61: scaler.transform, then
 * clf.predict), two classes.  The desc carries HOST pointers, copied at create (like dsp_plan_desc):
 *   dec(x) = sum_i h_dual[i] exp(-gamma |(x - h_center) / h_scale - h_sv[i]|^2) + intercept
 *   label  = class0 where dec <= 0, class1 where dec > 0                       (SVC.classes_[dec > 0])
 * gamma is the resolved number (SVC._gamma, not the string 'scale').  Sizes out of range, a gamma that is not finite and
 * positive, a scale that is zero or not finite and any other non-finite number are DSP_EINVAL, checked before any device
 * call.  Create stores the support vectors transposed and padded to whole wavefronts on the current device (a blocking
 * copy: it must not run inside a stream capture); the handle is immutable afterwards and may be used from several streams.
 * Under dsp_debug_host_dry_run(1) the tables stay in host memory: such a handle can only be destroyed, launches are refused.
 */
typedef struct dsp_svm dsp_svm;
typedef struct dsp_svm_desc {
    int32_t n_features, n_sv;            /* 1..16, 1..65536 */
    int32_t class0, class1;              /* dec <= 0 -> class0, dec > 0 -> class1 */
    double gamma, intercept;
    const double* h_center;              /* [n_features]; NULL = 0 (RobustScaler(with_centering=False)) */
    const double* h_scale;               /* [n_features]; NULL = 1 */
    const double* h_sv;                  /* [n_sv, n_features] row-major (SVC.support_vectors_) */
    const double* h_dual;                /* [n_sv] (SVC.dual_coef_[0]) */
} dsp_svm_desc;
int dsp_svm_create(const dsp_svm_desc* desc, dsp_svm** out);
int dsp_svm_destroy(dsp_svm* svm);
/*
 * pitch_model.py:59-61 for a batch: row r of d_feat (fp64, row stride ld_feat >= n_features doubles) -> d_decision[r] (fp64)
 * and d_label[r] (int32); either may be NULL, not both.  One wavefront per row, everything in fp64 with a true division by the
 * scale and a fixed summation order: the same arguments give the same bits on every call.  One launch on `stream`, nothing
 * allocated (capturable).
 */
int dsp_svm_decision_batch(const dsp_svm* svm, const double* d_feat, int64_t ld_feat, int32_t n_rows, double* d_decision,
                           int32_t* d_label, void* stream);

/*
 * model.py:156-157 and ensemble.py:49-53 for a batch, one launch, one wavefront per clip:
 *   d_prob[b, :] = softmax(d_logits[b, :])   fp64 arithmetic, max subtracted, rounded to fp32    F.softmax      model.py:156
 *   pred         = the lowest index among the largest logits                                     torch.max      model.py:157
 *   the first rule with pred in {label_a, label_b} and (double)d_prob[b, pred] < threshold fires: its SVM (the arithmetic of
 *   dsp_svm_decision_batch, bit for bit) decides from row b of d_feat                           ensemble.py:50-53
 * d_logits: [n_utt, n_classes] fp32, row stride ld_logits; the logits are assumed finite (with a NaN the row's outputs are
 * unspecified).  d_valid: int32, element b * ld_valid says whether row b of d_feat holds features (dsp_pitch_feature_batch's
 * d_aux[:, 8] with ld_valid = 9); NULL = all valid.  d_feat may be NULL when n_rules = 0.
 *   d_pred [n_utt]             the final label
 *   d_prob [n_utt, n_classes]  dense, or NULL
 *   d_used [n_utt]             0: no rule fired;  r + 1: rule r's SVM decided;  -(r + 1): rule r fired but the features were
 *                              invalid and the classifier's label stands -- the reference raises there (pitch.pitch_feature
 *                              on a segment too short to fit)
 *   d_decision [n_utt]         the SVM's value where one was evaluated, else 0; or NULL
 * The rules (at most 4) are passed by value into the launch: nothing is uploaded or allocated per call (capturable).
 * DSP_EINVAL before any device call: sizes out of range, a label >= n_classes, rules whose label sets overlap, SVMs with
 * different feature counts, ld_feat below that count, a handle of another device or a dry-run one.
 */
typedef struct dsp_ensemble_rule {
    int32_t label_a, label_b;
    double threshold;
    const dsp_svm* svm;
} dsp_ensemble_rule;
int dsp_ensemble_decide_batch(const float* d_logits, int64_t ld_logits, int32_t n_utt, int32_t n_classes,
                              const dsp_ensemble_rule* rules, int32_t n_rules, const double* d_feat, int64_t ld_feat,
                              const int32_t* d_valid, int64_t ld_valid, int32_t* d_pred, float* d_prob, int32_t* d_used,
                              double* d_decision, void* stream);

/*
 * pitch_model.py:55-57 without the host: sig = preemphasis(sig, coeff) over the WHOLE clip (preprocess.py:19), then sig[l:r],
 * as fp32 at d_dst_offsets[b]:
 *   out[i] = (float)(x[l + i] - coeff * x[l + i - 1]),  and x[0] itself where l + i = 0
 * so the first kept sample sees the one in front of the segment.  fp64 with the product and the difference rounded
 * separately, as NumPy does, then one rounding to fp32.  int16 and fp32 input; fp32 samples are promoted to double first,
 * which is what the reference computes on a float64 array holding the same values.  Tables as dsp_trim_scale_batch
 * (d_sample_offsets [n_utt + 1], d_segments [n_utt, 2] relative to each clip and clipped to it, d_dst_offsets [n_utt]).
 */
int dsp_trim_preemph_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets, const int64_t* d_segments,
                           const int64_t* d_dst_offsets, int32_t n_utt, double coeff, float* d_out, void* stream);

/* ---- mixed sample rates in one batch (RNNModel.get_batch_full on a shuffled batch, model.py:114-135) ---------------- */
/*
 * reader.mini_batch_iterator shuffles the file list and yields feat = [(sig, rate), ...] (reader.py:80), and the data set
 * holds 44.1 kHz and 48 kHz recordings: model.py:114-135 runs endpoint_detect(sig, rate) and feature_extract_mfcc(s, r) with
 * each clip's own rate.  Framing, window and mel table differ per rate, so a batch runs as one sub-batch per distinct rate;
 * the entry points below let every sub-batch write its rows straight into the shared [max_len, B, width] tensor of
 * model.py:131-135, and make the clips of one rate contiguous when they are not.
 *
 * The placed forms of the three kernels that write the classifier's input.  Utterance b of the call writes element
 *   (t, dst_col[b], col_offset + k),  k < 3C (finalize) or 2 (the optional streams of model.py:90-101, 125-128),
 * of a [max_len, n_cols, row_width] fp32 tensor, for every t < max_len (zero rows beyond the stream's own length,
 * model.py:35-50); nothing outside those blocks is touched.  d_dst_col: [n_utt] DISTINCT columns in [0, n_cols) -- the
 * caller guarantees it -- or NULL for the identity.  Checked before any launch: n_cols >= n_utt, col_offset >= 0,
 * col_offset + the stream's width <= row_width, and what the unplaced entry point checks.  The values are the unplaced entry
 * points' bit for bit: the kernels are the same, the unplaced calls pass the identity.
 *
 * dsp_model_finalize_placed_batch covers both sources: d_segments / d_work NULL = dsp_model_finalize_batch, both set =
 * dsp_model_finalize_segments_batch.  d_len0 is [n_cols]: utterance b's min(T_b, max_len) goes to d_len0[dst_col[b]].
 * An utterance with d_dst_col[b] < 0 is SKIPPED by this entry point: it writes no rows and no d_len0 entry (the pad slots of a
 * rate group, dsp_rate_groups_batch below).  The two optional-stream entry points below take non-negative columns only.
 */
int dsp_model_finalize_placed_batch(const float* d_mfcc, int64_t ld_in, const int64_t* d_frame_offsets,
                                    const int64_t* d_segments, const void* d_work, int32_t n_utt, int32_t C, int32_t N,
                                    int32_t max_len, float* d_out, int32_t* d_len0, const int32_t* d_dst_col, int32_t n_cols,
                                    int32_t row_width, int32_t col_offset, void* stream);
/* dsp_model_timefeat_batch (model.py:97-101) and dsp_model_pitchfeat_batch (model.py:90-95), placed. */
int dsp_model_timefeat_placed_batch(const double* d_amp_sum, const int64_t* d_frame_offsets, int32_t n_utt, int32_t frame_len,
                                    int32_t max_len, float* d_out, const int32_t* d_dst_col, int32_t n_cols, int32_t row_width,
                                    int32_t col_offset, void* stream);
int dsp_model_pitchfeat_placed_batch(const double* d_pitch, const int64_t* d_frame_offsets, int32_t n_utt, int32_t max_len,
                                     float* d_out, const int32_t* d_dst_col, int32_t n_cols, int32_t row_width,
                                     int32_t col_offset, void* stream);

/*
 * Clip d_pick[i] of the source batch (samples [d_sample_offsets[p], d_sample_offsets[p + 1]) of d_wave, p = d_pick[i]) is
 * copied, sample type kept (int16 stays int16, reader.py:80), to d_out + d_dst_offsets[i] (in samples), i < n_pick.  A plain
 * copy: 16-byte vectors where source and destination are equally aligned, element by element elsewhere; several workgroups
 * per clip.  Needed only when the clips of one rate do not already form one contiguous run of the device buffer.
 * n_pick = 0 is a no-op, n_pick <= 65535 (one grid row per clip); the regions must not overlap d_wave.
 */
int dsp_gather_clips_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets, const int32_t* d_pick,
                           int32_t n_pick, const int64_t* d_dst_offsets, void* d_out, void* stream);

/*
 * The grouping by rate itself as device work, so that ONE recorded launch sequence serves a shuffled epoch of 44.1 / 48 kHz
 * files (reader.py:80, model.py:114-135) whatever the lengths and the rate of each position are: the device form of
 * group_by_rate and _MixedPlan in features/model_glue.py.  Every group g < n_groups <= DSP_MAX_RATE_GROUPS gets tables of
 * n_utt SLOTS: its clips first, in batch order (a stable partition), then pad slots -- clips of pad_len samples of
 * DSP_GROUP_PAD_VALUE that run through the group's pipeline and are written nowhere -- so that each group is a batch of
 * exactly n_utt clips of at most sample_capacity + n_utt * pad_len samples, which is what a capacity layout serves.
 *
 * dsp_rate_groups_batch (one launch, one workgroup, plain stores and fixed scans: no atomics, no memset, the same bits on
 * every run, capturable) reads d_rates [n_utt] (Hz), the caller's d_sample_offsets_in [n_utt + 1] and, unless NULL,
 * d_jitter [n_utt, 2] (model.py:54-60) from device memory; group_rates [n_groups] (distinct, > 0) and the four arrays of
 * n_groups table pointers are HOST arrays.  It writes, every word on every launch,
 *   d_sample_offsets    the sanitised source table, by the rule of dsp_batch_offsets_batch: out[0] = 0, out[b + 1] =
 *                       clamp(in[b + 1], out[b], sample_capacity); the gather reads this table only;
 *   d_pick[g]           [n_utt] the source clip of each slot, -1 for a pad slot;  d_dst_col[g]: the same values, the
 *                       placement columns of dsp_model_finalize_placed_batch;
 *   d_group_offsets[g]  [n_utt + 1] the running sum of the group's sanitised clip lengths, then + pad_len per pad slot:
 *                       the sample offsets of the group's own batch;
 *   d_group_jitter[g]   [n_utt, 2] the jitter rows in slot order, zeros for pad slots (NULL together with d_jitter);
 *   d_count             [n_groups] the clips of each group;
 *   d_status            one int32: bits 0-3 as dsp_batch_offsets_batch, judged on the caller's table; bit 4: a rate that is
 *                       not in group_rates -- that clip goes to group 0, which is defined and memory-safe.
 *
 * dsp_gather_groups_batch (one launch for all groups) copies slot i of group g, clip d_pick[g][i] of d_wave read through
 * the SANITISED d_sample_offsets, to d_out[g] + d_group_offsets[g][i] as dsp_gather_clips_batch copies (sample type kept),
 * and fills a pad slot with pad_len samples of DSP_GROUP_PAD_VALUE.  d_out[g]: that group's own buffer of at least
 * sample_capacity + n_utt * pad_len samples, starting on a 16-byte vector, distinct from d_wave and from each other.
 *
 * dsp_scatter_segments_batch brings the groups' [n_utt, 2] segment tables (slot order, written by each group's endpoint
 * kernels) back to batch order: d_endpoints[d_dst_col[g][k]] = d_group_segments[g][k], pad slots skipped; one launch.
 */
#define DSP_MAX_RATE_GROUPS 4
#define DSP_GROUP_PAD_VALUE 1
int dsp_rate_groups_batch(const int32_t* d_rates, const int64_t* d_sample_offsets_in, const int64_t* d_jitter, int32_t n_utt,
                          int64_t sample_capacity, int32_t n_groups, const int32_t* group_rates, int64_t pad_len,
                          int64_t* d_sample_offsets, int32_t* const* d_pick, int32_t* const* d_dst_col,
                          int64_t* const* d_group_offsets, int64_t* const* d_group_jitter, int32_t* d_count, int32_t* d_status,
                          void* stream);
int dsp_gather_groups_batch(const void* d_wave, int wave_dtype, const int64_t* d_sample_offsets, int32_t n_utt, int32_t n_groups,
                            const int32_t* const* d_pick, const int64_t* const* d_group_offsets, int64_t pad_len,
                            void* const* d_out, void* stream);
int dsp_scatter_segments_batch(const int64_t* const* d_group_segments, const int32_t* const* d_dst_col, int32_t n_utt,
                               int32_t n_groups, int64_t* d_endpoints, void* stream);
/*
 * dsp_scatter_group_rows_batch: the same way back for any small per-slot rows -- the pitch tail's [n_utt, 5] fp64 features (40
 * bytes a row) and [n_utt, 9] int32 details (36 bytes, not 8-byte aligned), which every group computes over all its n_utt
 * slots, pads included.  d_out[d_dst_col[g][k]] = d_group_rows[g][k] for g < n_groups, k < n_utt; rows are row_bytes bytes (a
 * multiple of 4 in [4, 256]) and move as 4-byte words.  A slot whose column is negative (a pad slot) or >= n_utt is skipped
 * WITHOUT reading its row, so the call is memory-safe on tables it did not write and a pad slot's NaN row goes nowhere.
 * d_group_rows and d_dst_col are HOST arrays of n_groups device pointers, each on a 4-byte word, as d_out is; d_out
 * [n_utt, row_bytes] shares no byte with a group's table.  n_utt in [1, 65535].  One launch for all groups, plain stores: no
 * atomics, no memset, the same bits on every run; where the groups partition the batch every row of d_out is written.
 */
int dsp_scatter_group_rows_batch(const void* const* d_group_rows, const int32_t* const* d_dst_col, int32_t n_utt, int32_t n_groups,
                                 int32_t row_bytes, void* d_out, void* stream);

/* ---- the attention blocks: rnn_clf.Transformer's encoder layer and rnn_clf.HRNN_Att's pooling (forward, fp32) ------- */
/*
 * transformer.EncoderLayer with n_head = 1 (transformer.py:16-140: MultiHeadAttention, ScaledDotProductAttention,
 * PositionwiseFeedForward; layers.py:125-143: LayerNormalization) over x [T, B, d_model].  ALL T rows as given take part (no
 * length mask: the zero rows behind short utterances count too).  Per utterance b, with x_b [T, d]:
 *   q = x_b w_qs, k = x_b w_ks, v = x_b w_vs                                        transformer.py:98-100
 *   s[b,t,u] = tanh(q[b,t]) . k[b,u] / sqrt(d_model)                                transformer.py:38,50-52 (tanh on q only)
 *   a[b,t,u] = exp(s[b,t,u]) / sum_b' exp(s[b',t,u])                                transformer.py:41,56: nn.Softmax() without a dim
 *                                                                                   on a 3-D tensor is a softmax over the BATCH axis
 *   o[b,t] = sum_u a[b,t,u] v[b,u];   z1 = LN1(proj(o) + x[b,t])                    transformer.py:58,112-121
 *   y[b,t] = LN2(w_2 relu(w_1 z1 + b_1) + b_2 + z1)                                 transformer.py:134-139
 *   LN(z) = (z - mean) / (std_unbiased + eps) * a_2 + b_2                           layers.py:138-142
 * layers.py:136 returns z unchanged when z.size(1) == 1: LN1 sees [B, T, d] and is skipped when T == 1, LN2 sees [T, B, d]
 * and is skipped when B == 1.  Utterances are coupled through the softmax; at B == 1 every weight is exactly 1.
 *
 * Three launches on `stream` (csrc/kernels_attn.h): a projection, the statistics max_b s and sum_b exp(s - max) for every
 * (t, u), and the output, which recomputes the scores; no [B, T, T] tensor exists.  The maximum is subtracted (scores beyond
 * +-88 do not overflow), the sum over b runs in a fixed order without atomics (the same arguments give the same bits).
 *
 * d_params: DSP_ATTN_PARAMS DEVICE pointers in the module's parameter order, row-major as torch holds them:
 *   slf_attn.w_qs [1, d_model, d_k], w_ks [1, d_model, d_k], w_vs [1, d_model, d_v], slf_attn.layer_norm.a_2, b_2 [d_model],
 *   slf_attn.proj.weight [d_model, d_v], bias [d_model], pos_ffn.w_1.weight [d_inner, d_model, 1], bias [d_inner],
 *   pos_ffn.w_2.weight [d_model, d_inner, 1], bias [d_model], pos_ffn.layer_norm.a_2, b_2 [d_model].
 * Sizes out of range, n_head != 1 or a NULL parameter are DSP_EINVAL, checked before any device call.  Create copies and
 * repacks the parameters on the current device (blocking: it must not run inside a stream capture); the handle is immutable
 * afterwards, belongs to that device and may be used from several streams.  Under dsp_debug_host_dry_run(1) d_params are read as
 * HOST memory and the packed copy stays there: such a handle can only be destroyed, launches are refused.
 */
#define DSP_ATTN_PARAMS 13
typedef struct dsp_attn dsp_attn;
typedef struct dsp_attn_desc {
    int32_t d_model;      /* 1 .. 64; rows of x need no alignment beyond a float's (39 in the shipped head) */
    int32_t d_inner;      /* multiple of 4 in [4, 256] */
    int32_t n_head;       /* 1 */
    int32_t d_k, d_v;     /* multiples of 4 in [4, 128] */
    float eps;            /* layers.py:128: 1e-3 */
    const float* d_params[16];
} dsp_attn_desc;
int dsp_attn_create(const dsp_attn_desc* desc, dsp_attn** out);
int dsp_attn_destroy(dsp_attn* h);
/*
 * bytes of the workspace dsp_attn_forward needs at (T, B), T in [1, 1024], B >= 1: zero-padded copies of x and of the folded
 * queries, 2 B T' D' floats (T', D': T and d_model rounded up to 16), and the two [T', T'] statistics.  No term grows with B T T:
 * 41 MB at (200, 512) and d_model 39, half of one [B, T, T] fp32 tensor.
 */
int dsp_attn_workspace_bytes(const dsp_attn* h, int32_t T, int32_t B, int64_t* bytes);
/*
 * d_x, d_y: [T, B, d_model] fp32, dense; every element of d_y is written on every call, d_x is only read (d_y == d_x is not
 * supported).  d_work: the caller's buffer of at least dsp_attn_workspace_bytes bytes, 16-byte aligned, so that the call
 * allocates nothing and can be captured into a HIP graph.
 */
int dsp_attn_forward(const dsp_attn* h, const float* d_x, int32_t T, int32_t B, float* d_y, void* d_work, int64_t work_bytes,
                     void* stream);

/*
 * Training the encoder layer: dsp_attn_forward_train saves a tape, dsp_attn_backward turns the gradient of y into the gradient
 * of x and into the row gradients from which the 13 parameter gradients are plain GEMMs and column sums
 * (features/classifier.py: attn_param_grads).  Sizes as the forward's, except d_model in [2, 64]: the unbiased std of one
 * element (layers.py:139) is 0 / 0 in the reference as well.  Every entry point below checks its sizes and the byte counts
 * of the caller's buffers before any device call (DSP_EINVAL), allocates nothing and is capturable into a HIP graph.
 *
 * With Qt = tanh(x w_qs), q' = Qt w_ks^T / sqrt(d_model) (so that s[b,t,u] = q'[b,t] . x_b[u]), A the batch-axis softmax of
 * transformer.py:41,56, M[b,t] = sum_u A[b,t,u] x_b[u], o = M w_vs, r1 = proj(o) + x, z1 = LN1(r1), h = relu(w_1 z1 + b_1),
 * r2 = w_2 h + b_2 + z1, y = LN2(r2) (transformer.py:112-121,134-139; layers.py:136-142 with both skips):
 *   row-wise:   g_r2 = LN2'(g_y);  g_pre1 = (g_r2 w_2) [h > 0];  g_z1 = g_r2 + g_pre1 w_1;  g_r1 = LN1'(g_z1);
 *               g_o = g_r1 proj.weight;  g_M = g_o w_vs^T
 *   LN'(g):     c = r - mean, s = std_unbiased + eps, g_n = g a_2:  (g_n - mean(g_n)) / s - c sum(g_n c) / (s^2 std (d - 1));
 *               a skipped LN (layers.py:136) passes g through
 *   coupled:    g_A[b,t,u] = g_M[b,t] . x_b[u];  D[t,u] = sum_b A g_A;  g_S = A (g_A - D);  g_q'[b,t] = sum_u g_S x_b[u];
 *               g_preQ = (g_q' w_ks / sqrt(d_model)) (1 - Qt^2)
 *   dx[b,t]   = g_r1[b,t] + g_preQ[b,t] w_qs^T + sum_t' (A[b,t',t] g_M[b,t'] + g_S[b,t',t] q'[b,t'])
 * Four launches (csrc/kernels_attn_bwd.h): rows, the [T', T'] statistic D, the sums over u, the sums over t (left out when
 * d_gx is NULL).  The score tiles are recomputed from the tape; no [B, T, T] tensor exists.  Sums run in a fixed order without
 * atomics: the same arguments give the same bits.
 *
 * The tape, in floats (T', D': T and d_model rounded up to 16):
 *   x padded [B, T', D'] | q' [B, T', D'] | max_b s [T', T'] | sum_b exp(s - max) [T', T'] | M [B, T', D']
 * i.e. the forward's workspace and the rows M behind it; rows t >= T of M are not meaningful.  61 MB at (200, 512), d_model 39.
 */
int dsp_attn_tape_bytes(const dsp_attn* h, int32_t T, int32_t B, int64_t* bytes);
/*
 * dsp_attn_forward that also fills d_tape (at least dsp_attn_tape_bytes bytes, 16-byte aligned).  d_y is bit for bit the
 * output of dsp_attn_forward: the same three launches, the last of which also stores M.
 */
int dsp_attn_forward_train(const dsp_attn* h, const float* d_x, int32_t T, int32_t B, float* d_y, void* d_tape, int64_t tape_bytes,
                           void* stream);
/*
 * work_bytes: the backward's workspace (padded g_M and row part of dx, 2 B T' D' floats, and D [T', T']).  da_bytes: the
 * row gradients, T B (4 d_model + d_inner + d_v + d_k) floats.
 */
int dsp_attn_backward_bytes(const dsp_attn* h, int32_t T, int32_t B, int64_t* work_bytes, int64_t* da_bytes);
/*
 * d_tape: as dsp_attn_forward_train left it, with the same handle, T and B.  d_gy [T, B, d_model]: the gradient of y, dense.
 * d_gx [T, B, d_model]: the gradient of x, every element written; NULL: not wanted (one launch fewer).  d_da: seven dense
 * tensors one behind the other, every element written:
 *   g_r2 [T, B, d_model] | g_pre1 [T, B, d_inner] | g_z1 [T, B, d_model] | g_r1 [T, B, d_model] | g_o [T, B, d_v] |
 *   g_q' [T, B, d_model] | g_preQ [T, B, d_k]
 * d_tape and d_work are 16-byte aligned.  Nothing behind T rows is written to d_gx or d_da.
 */
int dsp_attn_backward(const dsp_attn* h, int32_t T, int32_t B, const void* d_tape, int64_t tape_bytes, const float* d_gy, float* d_gx,
                      float* d_da, int64_t da_bytes, void* d_work, int64_t work_bytes, void* stream);

/*
 * layers.SelfAttn (layers.py:78-95) over d_y [T, B, H] fp32, dense and 16-byte aligned:
 *   e[t,b] = d_v . tanh(d_W y[t,b] + d_bW) + d_c[0]                  layers.py:88-90 (attn: Linear(H, H), v: Linear(H, 1))
 *   w[.,b] = softmax of e[.,b] over ALL T rows                       layers.py:91 -- the zero rows behind a short utterance get
 *                                                                    e = d_v . tanh(d_bW) + d_c[0] and a non-zero weight
 *   d_out[b] = sum_t w[t,b] y[t,b]                                   layers.py:93-94, [B, H]
 * d_W [H, H] (16-byte aligned), d_bW [H], d_v [H] and d_c [1] are torch's own parameter tensors (attn.weight, attn.bias,
 * v.weight, v.bias), read in place: there is no handle.  One launch on `stream`, one wavefront per column, sums in a fixed
 * order; nothing is allocated (capturable).  T in [1, 1024], B >= 1, H a multiple of 4 in [4, 256]; anything else, a NULL or
 * misaligned pointer is DSP_EINVAL, checked before any device call.
 */
int dsp_selfattn_pool_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW, const float* d_v,
                            const float* d_c, float* d_out, void* stream);
/*
 * dsp_selfattn_pool_batch over the first rows = clamp(*d_rows, 1, T) rows of d_y only, the count read from device memory (one
 * wave-uniform read per workgroup): the softmax of a batch whose padded row count ceil(max(len0) / hir) only the device
 * knows (dsp_head_lengths_batch: d_info + 1).  T stays the row count of the buffer and the bound of every loop; d_out is bit for
 * bit dsp_selfattn_pool_batch's on d_y[:rows].  d_rows NULL is DSP_EINVAL; every other check as dsp_selfattn_pool_batch.
 */
int dsp_selfattn_pool_rows_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW, const float* d_v,
                                 const float* d_c, float* d_out, const int32_t* d_rows, void* stream);
/*
 * dsp_selfattn_pool_batch that also writes the weights w [T, B] to d_w; d_out is bit for bit dsp_selfattn_pool_batch's.
 */
int dsp_selfattn_pool_train_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW, const float* d_v,
                                  const float* d_c, float* d_out, float* d_w, void* stream);
/*
 * The backward of layers.py:88-94 given d_w (the saved weights) and d_gout [B, H] (16-byte aligned), the gradient of d_out:
 *   g_w[t] = g_out[b] . y[t,b];   g_e = w (g_w - sum_t w g_w);   g_pre = g_e v (1 - tanh^2(W y + b_W));   g_y = w g_out + g_pre W
 * One launch, one wavefront per column; the pre-activations are recomputed on the matrix pipe; sums over t and over the lanes
 * of a row run in a fixed order.  Written, every element: d_gpre [T, B, H], d_ge [T, B], d_gvpart [B, H] = sum_t g_e tanh(.)
 * per column, and d_gy [T, B, H] unless it is NULL (not wanted).  The parameter gradients are sums over these:
 * attn.weight: g_pre^T y, attn.bias: sum g_pre, v.weight: sum_b d_gvpart, v.bias: sum g_e.  Sizes, alignment and checks as the
 * forward's; nothing is allocated (capturable).
 */
int dsp_selfattn_pool_backward_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW, const float* d_v,
                                     const float* d_w, const float* d_gout, float* d_gy, float* d_gpre, float* d_ge, float* d_gvpart,
                                     void* stream);

/* ---- the classifier heads with the lengths on the device (csrc/kernels_head.h) ----
 *
 * The row counts of a batch, one launch of one workgroup: d_len0 [B] int32 (e.g. the len0 dsp_model_finalize_*_batch wrote) ->
 *   d_len0c[b] = clamp(d_len0[b], 1, T)          (d_len0c may be d_len0 itself)
 *   d_len1[b]  = ceil(d_len0c[b] / hir)          rnn_clf.py:52
 *   d_info[0]  = max_b d_len0c[b]                the rows pad_packed_sequence leaves (rnn_clf.py:31, 146)
 *   d_info[1]  = ceil(d_info[0] / hir)           the rows of the second level (rnn_clf.py:68, 113)
 *   d_info[2]  = number of entries outside [1, T] (the host-length path asserts; the device path counts)
 *   d_info[3]  = 0
 * B in [1, 65535], T >= 1, hir >= 1; anything else or a NULL pointer is DSP_EINVAL before any device call.  Nothing is
 * allocated or synchronised (capturable).
 */
int dsp_head_lengths_batch(const int32_t* d_len0, int32_t B, int32_t T, int32_t hir, int32_t* d_len0c, int32_t* d_len1, int32_t* d_info,
                           void* stream);
/*
 * The pooling of the heads (rnn_clf.py:29-31, 68-72, 113-115, 146) over d_y [T, B, H] fp32, dense, whose rows t >= len are
 * exact zeros in the reference and are NEVER READ here: with len = clamp(d_len[b], 1, T) and rows = d_rows ? min(*d_rows, T) : T
 *   d_feat[b * ld_feat + col_avg + h] = (sum_{t < len} d_y[t, b, h]) / (float)len        skipped when col_avg < 0
 *   d_feat[b * ld_feat + col_max + h] = max_{t < len} d_y[t, b, h], and where len < rows the maximum of that and 0.0f
 * i.e. y[:rows].sum(0) / n and y[:rows].max(0).values of a y with zero rows behind each end.  A NaN in an active row makes
 * the column's results NaN (torch.max / sum).  Only d_feat[b, col .. col + H) is written.  One launch; a column's rows are
 * split over four waves whose partial sums and maxima are combined in a fixed order: the same bits on every run.  16-byte
 * loads when H is a multiple of 4 and d_y is 16-byte aligned.  T, B >= 1, H in [1, 65535 * 64], col_max >= 0, the two column
 * ranges disjoint and inside ld_feat; anything else or a NULL d_y / d_len / d_feat is DSP_EINVAL before any device call.
 * Nothing is allocated or synchronised (capturable).
 */
int dsp_head_pool_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const int32_t* d_len, const int32_t* d_rows, float* d_feat,
                        int64_t ld_feat, int32_t col_avg, int32_t col_max, void* stream);

/* ---- training with the lengths on the device: the backward of the pieces above, and handles that survive an optimiser step ----
 *
 * dsp_head_pool_batch that also writes d_arg [B, H] int32, the row the max column came from: the smallest t < len whose value
 * the maximum returned (torch.max's first occurrence; the first NaN row if there is one), and -1 where the padding's 0.0f won
 * (len < rows and 0 > the maximum over the active rows; a tie between an active 0.0 and the padding goes to the active row).
 * d_feat is bit for bit dsp_head_pool_batch's.  d_arg NULL is DSP_EINVAL; every other check as dsp_head_pool_batch.
 */
int dsp_head_pool_train_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const int32_t* d_len, const int32_t* d_rows, float* d_feat,
                              int64_t ld_feat, int32_t col_avg, int32_t col_max, int32_t* d_arg, void* stream);
/*
 * The backward of the pooling given d_gfeat [B, ld_g], the gradient of d_feat (columns col_avg / col_max as in the forward), the
 * lengths and d_arg of dsp_head_pool_train_batch.  EVERY element of d_gy [T, B, H] is written exactly once, with
 * len = clamp(d_len[b], 1, T):
 *   t <  len:  (col_avg >= 0 ? d_gfeat[b, col_avg + h] / (float)len : 0) + (d_arg[b, h] == t ? d_gfeat[b, col_max + h] : 0)
 *   t >= len:  0.0f
 * The quotient is formed once per (b, h).  The gradient of a padding win (d_arg = -1) is dropped: those rows are constants of
 * the encoders.  One streaming launch, no atomics, no reduction: the same bits on every run; 16-byte stores when H is a
 * multiple of 4 and d_gy is 16-byte aligned.  Sizes and column checks as dsp_head_pool_batch (against ld_g); anything else or a
 * NULL pointer is DSP_EINVAL before any device call.  Nothing is allocated or synchronised (capturable).
 */
int dsp_head_pool_backward_batch(const float* d_gfeat, int64_t ld_g, int32_t col_avg, int32_t col_max, const int32_t* d_len,
                                 const int32_t* d_arg, int32_t T, int32_t B, int32_t H, float* d_gy, void* stream);
/*
 * The training twins of dsp_selfattn_pool_rows_batch: dsp_selfattn_pool_train_batch / dsp_selfattn_pool_backward_batch over the
 * first rows = clamp(*d_rows, 1, T) rows of the [T, ..] buffers, the count read from device memory (one wave-uniform read per
 * workgroup).  Results are bit for bit those of the plain calls on d_y[:rows] (and d_w[:rows]); every element of d_w, d_gy,
 * d_gpre and d_ge at t >= rows is written as 0.0f.  d_rows NULL is DSP_EINVAL; every other check as the plain calls.
 */
int dsp_selfattn_pool_rows_train_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW,
                                       const float* d_v, const float* d_c, float* d_out, float* d_w, const int32_t* d_rows, void* stream);
int dsp_selfattn_pool_rows_backward_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW,
                                          const float* d_v, const float* d_w, const float* d_gout, float* d_gy, float* d_gpre, float* d_ge,
                                          float* d_gvpart, const int32_t* d_rows, void* stream);
/*
 * Repack the parameters `desc` points to into the handle's EXISTING packed buffer, with launches on `stream`: what a training
 * loop calls after the optimiser wrote the parameters, instead of destroy + create.  Nothing is allocated or synchronised
 * (capturable).  The sizes of the descriptor must equal the handle's; anything else, a NULL pointer or (dsp_attn) a dry-run
 * handle is DSP_EINVAL before any device call.  The two recurrent handles run create's pack kernels; dsp_attn_refresh gathers
 * the 12 matrices and 7 vectors on the device into the layout create packed on the host (pure data movement: the same bytes;
 * the zero padding written at create stays).  After a refresh every call through the handle gives the bits a freshly created
 * handle on the same parameters gives.
 * ORDERING: the refresh writes the buffer every call through the handle reads.  Work enqueued on `stream` is ordered by the
 * stream; the caller orders the refresh after earlier uses of the handle on OTHER streams (and later uses there after the
 * refresh), and after whatever wrote the parameters.
 */
int dsp_bigru_refresh(dsp_bigru* h, const dsp_bigru_desc* desc, void* stream);
int dsp_hmlstm_refresh(dsp_hmlstm* h, const dsp_hmlstm_desc* desc, void* stream);
int dsp_attn_refresh(dsp_attn* h, const dsp_attn_desc* desc, void* stream);

/* ---- device-resident Adam: the optimiser step of model.py:140-149 (torch.optim.Adam, weight_decay = 0, amsgrad off), capturable ----
 *
 * A handle owns, in ONE device allocation, the step count, the hyper-parameters (fp64), the pointer tables of n fp32 tensors
 * (parameter p, first moment m, second moment v, gradient g) and a chunk table.  dsp_adam_step is two launches on `stream`:
 *   1. one thread: t = ++step; step_size = lr / (1 - beta1^t) and bc2 = sqrt(1 - beta2^t), formed in fp64, rounded to fp32 once;
 *   2. every tensor in one launch, per element (fp32, every product, sum, quotient and root rounded to nearest):
 *        m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;  p = p - step_size * (m / (sqrt(v) / bc2 + eps))
 *      zero_grads != 0 also writes 0.0f over each gradient after reading it (zero_grad(set_to_none=False)).
 * A workgroup takes chunks of dsp_adam_chunk_elems() elements of ONE tensor (the table is built at create) and reads its
 * descriptor wave-uniformly; a lane does 16-byte loads and stores where p, g, m and v of the tensor are all 16-byte aligned,
 * 4-byte ones for any other tensor and for the tail numel % 4: alignment changes the route, never the bits.  No atomics, no
 * LDS, no memset; every element belongs to exactly one lane: the same bits on every run.  Everything the two launches read
 * -- tables, hyper-parameters, step count -- is read from device memory when they RUN: a recorded dsp_adam_step follows
 * dsp_adam_set_hyper / dsp_adam_set_step / dsp_adam_bind_grads calls made between replays.
 *
 * dsp_adam_create allocates and uploads (blocking, like every create here); the step count starts at 0.  bind_grads, set_hyper,
 * set_step and step only launch on `stream`: nothing is allocated, copied from host memory or synchronised (capturable).
 * dsp_adam_get_state reads step and hyper[4] = {lr, beta1, beta2, eps} back and synchronises `stream`.
 * DSP_EINVAL with a message before any device call: a NULL argument or pointer, n <= 0, numel <= 0, beta outside [0, 1),
 * eps < 0, a non-finite lr or eps, a pointer that is not 4-byte aligned, a negative step, p / m / v (and, in bind_grads, g)
 * ranges that overlap each other, a step before any bind_grads, a handle of another device.  Under dsp_debug_host_dry_run(1)
 * the tables stay in host memory: such a handle can only be destroyed, launches are refused.
 *
 * dsp_adam_chunk_table is the table builder alone, host only (no device): chunk k covers elements
 * [offset[k], min(offset[k] + dsp_adam_chunk_elems(), numel[tensor[k]])) of tensor[k]; tensors in order, offsets ascending, every
 * element of every tensor in exactly one chunk.  *n_chunks is always written; tensor and offset both NULL asks for the count alone,
 * otherwise capacity must hold it.
 */
typedef struct dsp_adam dsp_adam;
int dsp_adam_chunk_elems(void);
int dsp_adam_chunk_table(int32_t n, const int64_t* numel, int64_t capacity, int32_t* tensor, int64_t* offset, int64_t* n_chunks);
int dsp_adam_create(int32_t n, const int64_t* numel, float* const* d_p, float* const* d_m, float* const* d_v, double lr, double beta1,
                    double beta2, double eps, dsp_adam** out);
int dsp_adam_destroy(dsp_adam* h);
int dsp_adam_bind_grads(dsp_adam* h, float* const* d_g, void* stream);
int dsp_adam_set_hyper(dsp_adam* h, double lr, double beta1, double beta2, double eps, void* stream);
int dsp_adam_set_step(dsp_adam* h, int64_t step, void* stream);
int dsp_adam_get_state(const dsp_adam* h, int64_t* step, double* hyper, void* stream);
int dsp_adam_step(dsp_adam* h, int32_t zero_grads, void* stream);

/* ---- the products between the recurrent backward kernels, bounded by a row count read on the device (csrc/kernels_wgrad.h) ----
 *
 * The parameter and input gradients behind dsp_bigru_backward and dsp_hmlstm_backward are sums over the [T, B, ..] buffers those
 * kernels leave.  A library GEMM takes its extents from the host; these take R = d_rows ? clamp(*d_rows, 1, T) : T from device
 * memory when they RUN, read nothing at t >= R, and are fp32 on v_mfma_f32_16x16x4_f32 (exact f32: every element an fmaf chain
 * in a fixed order).  No atomics, no memset, no grid barrier: the same bits on every run, capturable.
 *
 * An operand is a [T, B, cols] fp32 view with a unit column stride: element (t, b, c) at d_ptr[t stride_t + b stride_b + c],
 * strides in floats and not negative (so da[:, :, d, :3 H] of a [T, B, 2, 4 H] buffer is d_ptr = da + d 4 H, stride_t = 8 H B,
 * stride_b = 8 H, cols = 3 H, and a [B, T, H] buffer is stride_t = H, stride_b = T H).  reserved must be 0.
 *
 * dsp_rows_wgrad:   d_c[m, n] = sum_{t < R, b < B} s[t, b] a[t, b, m] xs[t, b, n]     m = a->cols, n = x->cols, d_c dense
 *                   d_colsum[m] = sum_{t < R, b < B} a[t, b, m]                        unscaled; skipped when d_colsum is NULL
 *   xs[t, b, :] = x[t + shift, b, :] where 0 <= t + shift < R; for t + shift < 0 the row d_x_init[b init_stride_b + ..] (zeros
 *   when d_x_init is NULL; d_x_init needs shift = -1 and init_stride_b >= n); for t + shift >= R zeros, which is what a buffer
 *   whose rows behind R are zero gives.  s = d_scale [T, B] dense, or 1 when NULL.  READ: rows t < R of a, x and d_scale, the
 *   initial row, *d_rows.  NEVER READ: any row t >= R.  WRITTEN: every element of d_c (and d_colsum), and scratch.
 *   Two launches: workgroups over (128 x 128 output tile) x (chunk of dsp-fixed whole time steps counted from t = 0, a function
 *   of B alone) write partial tiles to d_scratch -- a chunk that starts at or behind R exits at once --, then one thread per
 *   element adds the chunks below ceil(R / chunk) in index order.  The bits depend on (m, n, B, R) and the data, not on T: a
 *   call bounded at R in a T-row buffer equals the unbounded call on the first R rows, bit for bit.
 *   d_scratch: 16-byte aligned, at least the bytes dsp_rows_wgrad_scratch_bytes gives for (T, B, m, n).
 *
 * dsp_rows_product: d_y[t, b, :] = a0[t, b, :] d_w0 (+ a1[t, b, :] d_w1)   for t < R;   exact +0.0f for R <= t < T
 *   d_w0 [a0->cols, n], d_w1 [a1->cols, n] dense; a1 and d_w1 both NULL for one product.  d_y [T, B, n] dense; EVERY element is
 *   written on every call.  READ: rows t < R of a0 / a1, the matrices, *d_rows.  NEVER READ: any row t >= R.  One launch.
 *
 * 16-byte loads and stores are taken where a pointer and its strides allow them; a 4-byte-aligned view gives the same bits.
 * LIMITS: T, B >= 1, T B < 2^31, at most 65535 chunks; cols and n in [1, 2048]; shift in {-1, 0, 1}; every pointer 4-byte
 * aligned; outputs and scratch must not overlap anything read nor each other.  Anything else or a NULL mandatory pointer is
 * DSP_EINVAL with a message before any launch.  Nothing is allocated or synchronised; everything runs on `stream`.
 */
typedef struct dsp_rows_operand {
    const float* d_ptr;
    int64_t stride_t, stride_b;
    int32_t cols;
    int32_t reserved;
} dsp_rows_operand;
int dsp_rows_wgrad_scratch_bytes(int32_t T, int32_t B, int32_t m, int32_t n, int64_t* out_bytes);
int dsp_rows_wgrad(const dsp_rows_operand* a, const dsp_rows_operand* x, int32_t shift, const float* d_x_init, int64_t init_stride_b,
                   const float* d_scale, int32_t T, int32_t B, const int32_t* d_rows, float* d_c, float* d_colsum, void* d_scratch,
                   int64_t scratch_bytes, void* stream);
int dsp_rows_product(const dsp_rows_operand* a0, const float* d_w0, const dsp_rows_operand* a1, const float* d_w1, int32_t n, int32_t T,
                     int32_t B, const int32_t* d_rows, float* d_y, void* stream);

/* ---- fitting the pitch model: RobustScaler.fit and SVC(kernel='rbf').fit (PitchModel.train pitch_model.py:48-50; csrc/kernels_svmfit.h) ----
 *
 * Everything is fp64.  No atomics, no memset, no communication between workgroups, nothing allocated or synchronised: every
 * launch goes to `stream` (capturable), every reduction is a fixed tree, the same arguments give the same bits on every call.
 * A matrix d_X is [n, F] fp64 with row stride ld >= F doubles.  LIMITS: F in [1, 16]; n in [1, 8192] for the scaler and the
 * variance, [2, 8192] for the solver; P in [1, 65535]; strides at most 2^32; every pointer aligned to its element size, the
 * workspace to 16 bytes; outputs (and the workspace) must not overlap anything read nor each other.  Anything else or a NULL
 * mandatory pointer is DSP_EINVAL with a message before any device call; under dsp_debug_host_dry_run(1) what passed every
 * check is refused instead of launched.
 *
 * dsp_robust_scale_fit_batch: scaler.fit(X)                                                              pitch_model.py:48
 *   d_valid: int32, element r * ld_valid says whether row r counts (dsp_pitch_feature_batch's d_aux[:, 8] with ld_valid = 9);
 *   NULL = every row.  (q_lo, q_hi): the quantile pair in percent, 0 <= q_lo <= q_hi <= 100 (RobustScaler: 25, 75).
 *   One workgroup per feature sorts the valid values in LDS and takes the percentiles as np.nanpercentile does (method
 *   'linear': virtual index (m q + (1 - q)) - 1, the two-sided lerp a + (b - a) t below t = 0.5, b - (b - a)(1 - t) from
 *   there, no contraction) and, with centering, np.nanmedian ((a + b) / 2 of the two middle values).
 *   d_scale [F] = q_hi - q_lo value, 1 where that is below 10 DBL_EPSILON (sklearn's _handle_zeros_in_scale);
 *   d_center [F]: written only with with_centering != 0 (may be NULL otherwise);
 *   d_info [2] = {valid rows, status}: 0 = fitted; 1 = no valid row; 2 = a valid row holds a non-finite value.  With a
 *   status other than 0 nothing but d_info is written.
 *
 * dsp_var_all: np.var of all entries of the rows (d_X - d_center) / d_scale (NULL: 0 / 1) that d_mask keeps (int8 [n],
 *   non-zero = kept; NULL = every row), two passes: d_out[0] = the variance, d_out[1] = the number of entries.  It is what
 *   SVC's gamma='scale' = 1 / (F var) needs.  One workgroup.
 *
 * dsp_svm_fit_batch: X = scaler.transform(X); clf.fit(X, y)                                              pitch_model.py:49-50
 *   P independent two-class C-SVC duals with the RBF kernel over ONE matrix, one workgroup per problem:
 *     min 1/2 a' Q a - e' a,  0 <= a <= C[p],  y' a = 0,   Q[s, t] = y_s y_t exp(-gamma[p] |x_s - x_t|^2)
 *   on the rows x = (d_X - d_center) / d_scale (a true division, as dsp_svm_decision_batch; NULL: 0 / 1) whose label
 *   d_Y[p, row] (int8, row stride ld_y >= n) is not 0: +1 / -1 are the classes, 0 takes the row out of problem p (label pairs,
 *   folds and invalid rows alike).  The solver is libsvm's (working-set selection by second-order information, the
 *   two-variable update with its four clipping cases, calculate_rho) without shrinking and without a kernel cache, in fp64,
 *   on positions in the ascending list of the problem's rows: a masked problem is bit for bit the problem on the compacted
 *   matrix.  Ties in both selections go to the lowest position.  It stops when m - M < tol (m = max of -y G over I_up, M =
 *   min over I_low) or after max_iter updates (1 .. 10 000 000): the launch always ends.  d_C, d_gamma: [P] on the device.
 *     d_coef [P, ld_coef >= n]  y a per row: exact +0 for rows outside the problem and non-support rows (SVC.dual_coef_ is
 *                               its non-zero entries, class -1 rows first for classes_[0])
 *     d_rho [P]                 SVC.intercept_ = -rho
 *     d_info [P, 5]             n_iter, status, n_sv, n_bounded (a = C), n_active
 *   status: 0 = converged; 1 = max_iter reached (the solution so far is written, as sklearn does under its
 *   ConvergenceWarning); 2 = a row of the problem is not finite after scaling; 3 = fewer than one row in either class;
 *   4 = C[p] or gamma[p] is not finite and positive.  Checked in the order 2, 4, 3.  With 2, 3 or 4 only d_info[p] is written.
 *   d_work: at least dsp_svm_fit_workspace_bytes(n, F, P) bytes (the scaled matrix and the row lists).
 */
#define DSP_SVMFIT_MAX_ROWS 8192
int dsp_robust_scale_fit_batch(const double* d_X, int64_t ld, int32_t n, int32_t F, const int32_t* d_valid, int64_t ld_valid,
                               double q_lo, double q_hi, int32_t with_centering, double* d_scale, double* d_center, int32_t* d_info,
                               void* stream);
int dsp_var_all(const double* d_X, int64_t ld, int32_t n, int32_t F, const double* d_center, const double* d_scale,
                const int8_t* d_mask, double* d_out, void* stream);
int dsp_svm_fit_workspace_bytes(int32_t n, int32_t F, int32_t P, int64_t* out_bytes);
int dsp_svm_fit_batch(const double* d_X, int64_t ld, int32_t n, int32_t F, const double* d_center, const double* d_scale,
                      const int8_t* d_Y, int64_t ld_y, int32_t P, const double* d_C, const double* d_gamma, double tol,
                      int32_t max_iter, double* d_coef, int64_t ld_coef, double* d_rho, int32_t* d_info, void* d_work,
                      int64_t work_bytes, void* stream);

/* ---- reproducible dropout: the F.dropout calls and nn.GRU's inter-layer dropout of rnn_clf.py, drawn on the device (csrc/kernels_dropout.h) ----
 *
 * A counter-based generator whose whole state is d_state = {seed, step}: two int64 words in device memory, 8-byte aligned,
 * read when a launch RUNS.  A multiplier is a pure function of (seed, step, site, element_index):
 *   Philox4x32 with 10 rounds (Salmon et al., SC'11: multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85);
 *   key = (seed_lo, seed_hi);  counter = (block, step_lo, step_hi, site),  block = element_index / 4;  the four output words
 *   serve elements 4 block .. 4 block + 3 in order.  element_index is the row-major index into the logical tensor, whatever
 *   the row bound, the alignment or the launch shape.  site: a small integer >= 0 that names the draw site.
 *   An element is kept iff (word >> 8) < thr, thr = llrint((1 - p) 2^24) in double; a kept element is multiplied by
 *   scale = (float)(1.0 / (1.0 - (double)p)), a dropped one becomes exact +0.0f.  p in [0, 1); p = 0 returns the input's bits.
 * The eager step and a graph replay therefore draw the same bits, a backward regenerates the mask instead of storing it, and
 * the state is 16 bytes of a checkpoint.  No atomics, no LDS, no memset, no allocation, nothing synchronised: every launch goes
 * to `stream` and is capturable; every element belongs to exactly one lane.
 *
 * dsp_rng_advance:         one thread: step += 1.
 * dsp_dropout_apply:       d_y[i] = d_x[i] * m[i], i < n.  16-byte accesses where d_x and d_y are both 16-byte aligned, 4-byte
 *                          ones for any other view and for the tail n % 4: the route never changes the bits.  d_y == d_x is
 *                          served; a partial overlap is refused.  d_key_out: NULL, or 16 bytes (8-byte aligned, apart from
 *                          every other argument) that receive the {seed, step} the launch used.
 * dsp_dropout_apply_key:   the same arithmetic keyed by a saved d_key (what d_key_out received): a backward multiplies the
 *                          incoming gradient by the forward's mask even when the state has advanced since.
 * dsp_dropout_multipliers: the fp32 multipliers d_m [L, T, B, C] (0 or scale) that dsp_bigru_forward_train takes as d_drop
 *                          (L = n_layers - 1, C = 2 H): layer l draws at site site_base + l with element_index over [T, B, C].
 *                          Rows t < R = clamp(d_rows[0], 1, T) are drawn (d_rows NULL: all T rows); every element of the rows
 *                          behind is written as exact +0.0f by a plain store and draws nothing.  EVERY element of d_m is
 *                          written on every call; the rows t < R are bit for bit those of the unbounded call.
 *
 * LIMITS: n in [0, 2^34) and T B C < 2^34 (block is one 32-bit word); L in [1, 64]; T, B, C >= 1; site and site_base + L below
 * 2^31; tensors 4-byte aligned, d_state / d_key / d_key_out 8-byte aligned; an output must not overlap d_state or d_rows.
 * Anything else or a NULL mandatory pointer is DSP_EINVAL with a message before any launch; under dsp_debug_host_dry_run(1)
 * what passed every check is refused instead of launched.
 */
int dsp_rng_advance(int64_t* d_state, void* stream);
int dsp_dropout_apply(const float* d_x, float* d_y, int64_t n, double p, int32_t site, const int64_t* d_state, int64_t* d_key_out,
                      void* stream);
int dsp_dropout_apply_key(const float* d_g, float* d_dx, int64_t n, double p, int32_t site, const int64_t* d_key, void* stream);
int dsp_dropout_multipliers(float* d_m, int32_t L, int32_t T, int32_t B, int32_t C, double p, int32_t site_base, const int64_t* d_state,
                            const int32_t* d_rows, void* stream);

/* ---- loss, its gradient and the epoch metrics on the device (csrc/kernels_loss.h) ----------------------------------------
 *
 * dsp_xent_metrics_batch turns [n_utt, n_classes] logits and labels into F.cross_entropy at its defaults (model.py:141-147),
 * its gradient, the prediction of model.py:156-157 and the metrics RNNModel.test / EnsembleModel.test collect on the host
 * (model.py:162-187, ensemble.py:44-64), accumulated in one caller-owned block.  At most TWO launches on `stream`: one wavefront
 * per clip for the per-clip outputs (only if one of them is asked for), then one workgroup, one clip per thread, for d_loss and
 * d_state (only if one of them is given; it forms the clips' values again, in the first launch's summation order).  n_scored is an integer count over the labels alone; every workgroup of the first launch counts it for itself,
 * so it is known before d_dlogits is scaled and nothing is stored between the launches.  No atomics, no memset, no allocation,
 * nothing synchronised: capturable.  The arithmetic is fp64 with the row maximum subtracted.
 *
 *   d_logits    fp32 [n_utt, n_classes], row stride ld_logits >= n_classes (finite; with a NaN the row's outputs are unspecified)
 *   d_labels    int64 [n_utt].  -100 is ignored (torch's ignore_index); any other label outside [0, n_classes) is ignored too
 *               and counted as bad_label.  A clip is SCORED iff its label lies in [0, n_classes).
 *   d_pred_in   int32 [n_utt] or NULL: the labels to score (the ensemble's final pred); NULL scores the arg-max of the logits.
 *               A value outside [0, n_classes) counts as wrong and is listed, but has no confusion cell.
 *   d_grad_out  fp32 [1] or NULL (= 1): the upstream gradient of the loss.
 * Per-call outputs, each may be NULL:
 *   d_nll       fp32 [n_utt]             logsumexp(row) - row[label]; 0 where the clip is not scored
 *   d_loss      fp32 [1]                 the sum of the unrounded fp64 nll over the scored clips -- thread t of the workgroup's
 *                                        512 adds the clips t, t + 512, ... in ascending order, the 64 lanes of a wave are added by
 *                                        a fixed butterfly and the 8 wave sums in order -- divided by n_scored and rounded once;
 *                                        NaN when nothing is scored, as torch's
 *   d_pred      int32 [n_utt]            the lowest index among the largest logits
 *   d_prob      fp32 [n_utt, n_classes]  the softmax, dense.  d_pred and d_prob are dsp_ensemble_decide_batch's with
 *                                        n_rules = 0 in every bit (one device function serves both)
 *   d_dlogits   fp32 [n_utt, n_classes], row stride ld_dlogits: (softmax - onehot(label)) * grad_out / n_scored, formed in fp64
 *               and rounded once; exact zeros in every clip that is not scored.  Only the n_classes columns are written.
 *
 * The epoch state, d_state or NULL: dsp_metrics_bytes(n_classes, wrong_capacity) bytes, 8-byte aligned, updated in place:
 *   int64  counts[8]      seen, scored, correct, ignored, bad_label, wrong_total, calls, reserved
 *                         (seen = scored + ignored; ignored counts the -100 labels AND the bad ones; correct + wrong_total = scored)
 *   fp64   loss_sum       the sum of the unrounded nll
 *   int64  confusion[n_classes][n_classes]   rows the true label, columns the scored label
 *                                            (sklearn.metrics.confusion_matrix with labels=range(n_classes))
 *   int32  wrong[wrong_capacity][3]          (index of the clip in the epoch = seen before this call + b, scored label, true
 *                                            label), appended in clip order; entries behind the capacity are counted in
 *                                            wrong_total and stored nowhere
 * padded to a multiple of 8 bytes.  A clip that is not scored moves only seen, ignored and bad_label.  Every confusion cell is
 * written by the one thread that owns it, the wrong list by a fixed prefix scan.  dsp_metrics_reset zeroes the block with a
 * kernel (a recorded memset of more than 4 bytes is not relied upon).  The same wrong_capacity must be passed on every call.
 *
 * LIMITS: n_utt in [1, 16384]; n_classes in [2, 64]; wrong_capacity in [0, 2^24]; fp32 / int32 tensors 4-byte aligned, d_labels
 * and d_state 8-byte aligned; no output (d_state included) may overlap another output or an input.  Anything else, NULL logits
 * or labels, or a call with nothing to write is DSP_EINVAL with a message before any device call; under
 * dsp_debug_host_dry_run(1) what passed every check is refused instead of launched.  The pointers carry no device: the caller
 * makes the device of the tensors current (features/metrics.py does).
 */
int dsp_metrics_bytes(int32_t n_classes, int32_t wrong_capacity, int64_t* out_bytes);
int dsp_metrics_reset(void* d_state, int32_t n_classes, int32_t wrong_capacity, void* stream);
int dsp_xent_metrics_batch(const float* d_logits, int64_t ld_logits, int32_t n_utt, int32_t n_classes, const int64_t* d_labels,
                           const int32_t* d_pred_in, const float* d_grad_out, float* d_nll, float* d_loss, int32_t* d_pred,
                           float* d_prob, float* d_dlogits, int64_t ld_dlogits, void* d_state, int32_t wrong_capacity, void* stream);

/* ---- the speaker discriminator of adv_clf.AdvHRNN: forward, loss and every gradient in one call (csrc/kernels_adv.h) ------
 *
 * adv_clf.py:34-38 behind the pooled feature: a gradient reversal (identity forward, -gamma times the gradient backward),
 * a = tanh(feat W1^T + b1), z = a W2^T + b2, trained with F.cross_entropy(z, speakers) (adv_model.py:45-47).  The loss is
 * terminal, so one call forms the forward, the loss and every gradient; an autograd node over it launches nothing in backward.
 * All arithmetic is fp32 on v_mfma_f32_16x16x4_f32, every element an fmaf chain in a fixed order that does not depend on B; the
 * loss and dz are dsp_xent_metrics_batch's in every bit (the same two kernels); dW / db come from the row-reduction kernels of
 * dsp_rows_wgrad with T = 1.  No atomics, no memset, no grid barrier, no allocation, nothing synchronised: capturable, and the
 * same arguments give the same bits on every run.
 *
 *   d_feat      fp32 [B, F], row stride ld_feat >= F        d_W1 [H, F], d_b1 [H], d_W2 [S, H], d_b2 [S]: dense
 *   d_speakers  int64 [B]; -100 and labels outside [0, S) are ignored exactly as dsp_xent_metrics_batch ignores them
 *   d_grad_out  fp32 [1] or NULL (= 1): the upstream gradient of the loss
 *   gamma       the reversal's factor by value; d_gamma (fp32 [1], device) replaces it when not NULL, so a schedule can move it
 *               between graph replays without a new capture.  By value it is rounded to fp32 once: both routes give the same bits.
 *
 * dsp_adv_disc_forward: ONE launch over tiles of 16 batch rows.  a -> d_a [B, H] (dense; may be NULL), z -> d_logits2 [B, S] with
 * row stride ld_logits2.  a stays in LDS between the two products.
 *
 * dsp_adv_disc_train: at most EIGHT launches on `stream`:
 *   1  the forward above (d_a is mandatory here; z goes to the workspace when d_logits2 is NULL);
 *   2  the two scoring launches: d_loss2 [1], d_dz [B, S] dense = (softmax - onehot) grad_out / n_scored with exact zeros in
 *      every row that is not scored, and the optional d_state metrics block (n_classes = S) with wrong_capacity;
 *   1  the backward over the same row tiles: da = dz W2, dpre = da (1 - a^2) -> workspace [B, H],
 *      d_dfeat [B, F] (row stride ld_dfeat) = -gamma (dpre W1) with gamma applied as one final multiply;
 *   2 + 2  d_dW2 [S, H] = dz^T a with d_db2 [S] its column sum, d_dW1 [H, F] = dpre^T feat with d_db1 [H] its column sum.
 * Every element of every output is written on every call.  Each of d_dW1, d_db1, d_dW2, d_db2, d_dfeat and d_logits2 may be NULL;
 * a NULL output is skipped together with the launches only it needs, and the other outputs keep their bits.
 * d_work: dsp_adv_disc_work_bytes(B, F, H, S) bytes, 16-byte aligned, contents unspecified before and after.
 *
 * LIMITS: B in [1, 16384], F in [1, 2048], H in [1, 512], S in [2, 64]; strides >= the columns; fp32 tensors 4-byte aligned,
 * d_speakers and d_state 8-byte aligned, d_work 16-byte aligned; no output (d_state and d_work included) may overlap another
 * output or anything that is read.  Anything else or a NULL mandatory pointer is DSP_EINVAL with a message before any device
 * call; under dsp_debug_host_dry_run(1) what passed every check is refused instead of launched.  The pointers carry no device:
 * the caller makes the device of the tensors current (features/adversarial.py does).
 */
int dsp_adv_disc_work_bytes(int32_t B, int32_t F, int32_t H, int32_t S, int64_t* out_bytes);
int dsp_adv_disc_forward(const float* d_feat, int64_t ld_feat, int32_t B, int32_t F, int32_t H, int32_t S, const float* d_W1,
                         const float* d_b1, const float* d_W2, const float* d_b2, float* d_a, float* d_logits2, int64_t ld_logits2,
                         void* stream);
int dsp_adv_disc_train(const float* d_feat, int64_t ld_feat, int32_t B, int32_t F, int32_t H, int32_t S, const float* d_W1,
                       const float* d_b1, const float* d_W2, const float* d_b2, const int64_t* d_speakers, const float* d_grad_out,
                       double gamma, const float* d_gamma, float* d_a, float* d_logits2, int64_t ld_logits2, float* d_loss2, float* d_dz,
                       float* d_dfeat, int64_t ld_dfeat, float* d_dW1, float* d_db1, float* d_dW2, float* d_db2, void* d_state,
                       int32_t wrong_capacity, void* d_work, int64_t work_bytes, void* stream);

/* ---- the column sums of the training step, bounded by a row count read on the device (csrc/kernels_reduce.h) --------------
 *
 * The sums over all rows that the heads' backward passes form beside their GEMMs: a.sum(0).sum(0) of a [T, B, n] buffer,
 * (g * n1).sum(0).sum(0), g.sum(0) of a [B, n] buffer (T = 1), g.sum() of a [T, B] buffer (cols = 1, stride_t = B,
 * stride_b = 1).  A library reduction of these shapes spreads one sum over workgroups that meet through counters a memset
 * zeroes; these are two plain launches.  fp32, a fixed order.  No atomics, no memset, no grid barrier, nothing allocated or
 * synchronised: the same bits on every run, capturable.
 *
 * dsp_rows_colsum:  d_out[c] = sum_{t < R, b < B} a[t, b, c] * (x ? x[t, b, c] : 1)     c < a->cols,
 *                   R = d_rows ? clamp(*d_rows, 1, T) : T, read from device memory when the kernels RUN.
 *   a and x are dsp_rows_operand views (above) with the same cols; x may be NULL.  With x, each product is rounded to fp32 and
 *   then added (never fused).  READ: rows t < R of a and x, *d_rows.  NEVER READ: any row t >= R.  WRITTEN: every element of
 *   d_out [cols], and scratch.
 *   Two launches: workgroups over (column block) x (chunk of whole time steps counted from t = 0, the chunk of dsp_rows_wgrad: a
 *   function of B alone) write one partial per (chunk, column) to d_scratch -- a chunk that starts at or behind R exits at
 *   once --, then one thread per column adds the chunks below ceil(R / chunk) in index order.  cols >= 64: lanes along the
 *   columns, 16 row groups added in index order; cols < 64: lanes along the rows, a fixed xor tree per wave, the 4 waves in
 *   index order.  The partition is a function of (B, cols) alone, so the bits depend on (cols, B, R) and the data, not on T: a
 *   call bounded at R in a T-row buffer equals the unbounded call on the first R rows, bit for bit.  tools/rows_sum_emul.py
 *   restates partition and order in NumPy.
 *   d_scratch: 16-byte aligned, at least the bytes dsp_rows_colsum_scratch_bytes gives for (T, B, cols).
 *
 * 16-byte loads are taken where a pointer and its strides allow them; a 4-byte-aligned view gives the same bits.
 * LIMITS: T, B >= 1, T B < 2^31, at most 65535 chunks; cols in [1, 2048]; every pointer 4-byte aligned; the output and the
 * scratch must not overlap anything read nor each other.  Anything else or a NULL mandatory pointer is DSP_EINVAL with a
 * message before any launch; under dsp_debug_host_dry_run(1) what passed every check is refused instead of launched.
 */
int dsp_rows_colsum_scratch_bytes(int32_t T, int32_t B, int32_t cols, int64_t* out_bytes);
int dsp_rows_colsum(const dsp_rows_operand* a, const dsp_rows_operand* x, int32_t T, int32_t B, const int32_t* d_rows, float* d_out,
                    void* d_scratch, int64_t scratch_bytes, void* stream);

/* ---- a census of a recorded graph (csrc/dsp_reduce.hip) -------------------------------------------------------------------
 *
 * Host only: walks a hipGraph_t (hipGraphGetNodes, hipGraphNodeGetType, hipGraphMemsetNodeGetParams, hipGraphGetRootNodes,
 * hipGraphNodeGetDependentNodes) and launches nothing.  What a recorded step is made of can then be looked at, not assumed:
 * n_roots = 1 and max_fanout = 1 is a chain; a memset node of more than 4 bytes (n_wide_memset) is what has been seen to replay
 * wrong on this stack.  `names` (may be NULL with names_bytes 0) receives the kernel nodes' names as the runtime gives them
 * (hipKernelNameRefByPtr on the node's function; "?" where it gives none), each followed by a newline, NUL-terminated; names
 * that do not fit are left out whole, and names_bytes in the result is what all of them need.
 * A NULL graph or result, or NULL names with a size, is DSP_EINVAL with a message.
 */
typedef struct dsp_graph_census_t {
    int32_t n_nodes, n_kernel, n_memset, n_memcpy, n_other; /* n_other: every other node type */
    int32_t n_wide_memset;                                  /* memset nodes of more than 4 bytes */
    int32_t n_roots, max_fanout;                            /* nodes without a predecessor; the most successors of one node */
    int64_t widest_memset_bytes;                            /* 0 without a memset node */
    int64_t names_bytes;                                    /* bytes every kernel name needs, terminator included */
} dsp_graph_census_t;
int dsp_graph_census(void* hip_graph, dsp_graph_census_t* out, char* names, size_t names_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DSP_FRONTEND_H */
