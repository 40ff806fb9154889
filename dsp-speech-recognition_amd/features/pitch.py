"""Drop-in for the reference's ``features/pitch.py``: both pitch trackers and the five pitch features.

* ``pitch_detect_sr``, the autocorrelation tracker ``model.py:92`` calls when ``cfg.use_pitch``
  is set.  Per frame of the 10 kHz signal the reference clips at the median (pitch.py:145-155), band-passes with a
  complex FIR built from an ideal band (sigproc.py:22-46), takes the magnitude and evaluates 180 autocorrelation lags
  (pitch.py:112-132).  Here that is one launch for all frames (``dsp_pitch_scores_batch``) and one for the sequential
  tail (``dsp_pitch_track_batch``).
* ``pitch_detect`` (pitch.py:83-94), the cepstral tracker, and ``pitch_feature`` (pitch.py:26-81, 227-279) built on it,
  which ``pitch_model.py`` calls once per clip.  Three launches: ``dsp_pitch_cepstrum_batch`` (clip, complex FIR at
  50 - 1000 Hz, FFT, log|.|, inverse FFT per frame), ``dsp_pitch_cepstrum_track_batch`` (in-place smoothing,
  peak-width scores, arg-max, octave repair per utterance) and ``dsp_pitch_feature_batch`` (sub-endpoint, the two
  smooth subsequences, slopes, quadratic terms, median shift).  ``pitch_feature_batch`` / ``pitch_features_device``
  are the batched forms.

``from features.pitch import *`` also yields what the reference's module re-exports through its own imports and
``pitch_model.py`` relies on (``basic_endpoint_detection``, ``preemphasis``, ``to_frames``, ``pickle``, ...).

The SVM these features feed (pitch_model.py:54-61) and the ensemble's gate are in ``features/ensemble.py``.

Out of scope: ``greedy_max_pitch`` and ``dp_max_pitch`` (no caller anywhere), the ``__main__`` experiment of the
reference's module (fitting stays with sklearn; nothing here imports it or matplotlib), and frame lengths that are not a
power of two in [128, 1024] on the cepstral path (``winlen = 0.0512`` gives 512, the only size a reference caller uses):
those raise ``ValueError``.
"""
from __future__ import annotations

import pickle  # noqa: F401  (re-exported: pitch.py:23, pitch_model.py:46-47)
import types

import numpy as np

from . import _native as nat
from .batch import _stream_ptr
from .endpoint import basic_endpoint_detection, get_amplitude, robust_endpoint_detection  # noqa: F401  (pitch.py:17)
from .preprocess import downsampling, preemphasis  # noqa: F401  (pitch.py:13,24)
from .sigproc import acr, to_frames  # noqa: F401  (pitch.py:14)

MIN_SHIFT, MAX_SHIFT = 20, 200        # pitch.py:126-127: 50 .. 500 Hz on the 10 kHz lag grid
_taps_cache = {}


def bandpass_taps(N, rate, low_freq=0, high_freq=500, wintype='square'):
    """The complex FIR of sigproc.window (sigproc.py:35-45), fp64."""
    Hd = np.zeros(N)
    Hd[int(N * low_freq / rate):int(N * high_freq / rate)] = 1
    w = np.hamming(N) if wintype == 'hamming' else np.ones(N)
    return 2 * np.pi * w * np.fft.ifft(Hd, N)


def window(sig, rate, low_freq=0, high_freq=500, wintype='square'):
    """sigproc.window (sigproc.py:22-46): API-surface helper on the host; the scoring kernel applies
    the same filter on the device."""
    sig = np.asarray(sig, dtype=np.float64)
    return np.convolve(sig, bandpass_taps(len(sig), rate, low_freq, high_freq, wintype))[:len(sig)]


def center_clip(frame, binary=True):
    """pitch.py:145-155 (API-surface helper; fused into the scoring kernel on the device)."""
    frame = np.asarray(frame, dtype=np.float64)
    pos = frame[frame >= 0]
    med = np.median(pos) if len(pos) else np.nan
    up, dn = frame > med, frame < -med
    if binary:
        return np.where(up, 1, np.where(dn, -1, 0))
    return np.where(up, frame - med, np.where(dn, frame + med, 0.0))


def _device_taps(L, rate, high_freq=900, arena=None):
    """The FIR taps on the device: from the module's cache, or -- with an ``arena`` -- a copy the arena owns."""
    key = (nat.current_device(), int(L), int(rate), int(high_freq))
    cache = _taps_cache if arena is None else arena
    key = key if arena is None else ('taps',) + key
    buf = cache.get(key)
    if buf is None:
        h = bandpass_taps(L, rate, 50, high_freq, 'hamming')
        arr = np.stack([h.real, h.imag], axis=1).astype(np.float32)
        buf = nat.DeviceBuffer(arr.nbytes).upload(arr)
        cache[key] = buf
    return buf


def _slot(arena, name, nbytes):
    """A named device buffer of ``nbytes``: this thread's library scratch slot -- which a later, larger call frees and
    replaces, so a pointer into it must not outlive the call -- or, with an ``arena`` (a dict its caller owns, e.g. a captured
    graph), a buffer of the arena: allocated on first use (an eager call) and never replaced; a later request that does not
    fit is an error, not a reallocation."""
    if arena is None:
        return nat.SCRATCH.get(name, nbytes)
    buf = arena.get(name)
    if buf is None:
        buf = arena[name] = nat.DeviceBuffer(max(int(nbytes), 4))
    elif buf.nbytes < nbytes:
        raise ValueError(f'arena buffer {name!r} holds {buf.nbytes} bytes, {nbytes} are needed: an arena serves one batch shape')
    return buf


def _upload_10k(sig10k, sample_offsets, L, S):
    so = np.ascontiguousarray(sample_offsets, dtype=np.int64)
    fo = nat.frame_offsets(so, L, S)
    x = np.ascontiguousarray(sig10k, dtype=np.float32).reshape(-1)
    d_x = nat.device_array('pitch_sig', x if x.size else np.zeros(1, dtype=np.float32))
    return d_x, nat.device_array('pitch_so', so), nat.device_array('pitch_fo', fo), so, fo


def frame_scores_batch(sig10k, sample_offsets, L, S, rate=10000, clip=True):
    """[sum T_b, 180] fp32 scores for concatenated 10 kHz signals; returns (scores, frame_offsets)."""
    nat.require_device()
    lib = nat.load()
    d_x, d_so, d_fo, so, fo = _upload_10k(sig10k, sample_offsets, L, S)
    n_lags = MAX_SHIFT - MIN_SHIFT
    d_out = nat.SCRATCH.get('pitch_scores', int(fo[-1]) * n_lags * 4)
    nat.check(lib.dsp_pitch_scores_batch(d_x.ptr, d_so.ptr, d_fo.ptr, len(so) - 1, int(fo[-1]), 0, int(L), int(S),
                                         _device_taps(L, rate).ptr, 1 if clip else 0, MIN_SHIFT, MAX_SHIFT,
                                         d_out.ptr, None))
    return d_out.download((int(fo[-1]), n_lags), np.float32).astype(np.float64), fo


def pitch_detect_frame_sr(frame, rate):
    """pitch.py:112-132 for one (already clipped) frame -> list of 180 scores."""
    frame = np.asarray(frame, dtype=np.float64).reshape(-1)
    scores, _ = frame_scores_batch(frame, [0, len(frame)], len(frame), len(frame), rate=rate, clip=False)
    return list(scores[0])


def _rows_on_device(g, flags, bias=MIN_SHIFT, degree=2):
    """Score rows [T, n_lags] (fp64) through dsp_pitch_rows_batch as a batch of one -> (rows after the call, pitch)."""
    nat.require_device()
    lib = nat.load()
    rows = np.ascontiguousarray(np.asarray(g, dtype=np.float64))
    if rows.ndim != 2:
        rows = rows.reshape(len(rows), -1)
    T, n = rows.shape
    if T == 0 or n == 0:
        return rows, np.zeros(0)
    d_rows = nat.device_array('pitch_rows', rows)
    d_fo = nat.device_array('pitch_rows_fo', np.array([0, T], dtype=np.int64))
    d_pitch = nat.SCRATCH.get('pitch_rows_out', T * 8)
    nat.check(lib.dsp_pitch_rows_batch(d_rows.ptr, d_fo.ptr, 1, n, int(bias), int(degree), int(flags), d_pitch.ptr, None))
    return (d_rows.download((T, n), np.float64) if flags & 1 else rows), (d_pitch.download((T,), np.float64) if flags & 2 else None)


def smooth(g, degree=2):
    """pitch.py:157-164 (in-place running mean over rows [i - degree, i + degree), the rows before i already
    smoothed), on the device."""
    rows, _ = _rows_on_device(g, 1, degree=degree)
    return rows.tolist()


def max_pitch(g, bias=20):
    """pitch.py:166-172: 1 / (1e-4 (bias + first arg-max)) per row, on the device."""
    return list(_rows_on_device(g, 2, bias=bias)[1])


def robust_max_pitch(g, bias=20):
    """pitch.py:191-206: max_pitch, then the two octave-repair sweeps, on the device."""
    return list(_rows_on_device(g, 2 | 4, bias=bias)[1])


def pitch_tracks_batch(sig10k, sample_offsets, L, S, rate=10000):
    """pitch.pitch_detect_sr's whole per-utterance chain for concatenated 10 kHz signals, on the device: frame scores
    (dsp_pitch_scores_batch), then smoothing in place, arg-max and the two octave-repair sweeps
    (dsp_pitch_track_batch; pitch.py:157-206).  Returns (pitch [sum T_b] in Hz, fp64, frame_offsets)."""
    nat.require_device()
    lib = nat.load()
    d_x, d_so, d_fo, so, fo = _upload_10k(sig10k, sample_offsets, L, S)
    n_lags = MAX_SHIFT - MIN_SHIFT
    d_scores = nat.SCRATCH.get('pitch_scores', int(fo[-1]) * n_lags * 4)
    d_pitch = nat.SCRATCH.get('pitch_track', int(fo[-1]) * 8)
    nat.check(lib.dsp_pitch_scores_batch(d_x.ptr, d_so.ptr, d_fo.ptr, len(so) - 1, int(fo[-1]), 0, int(L), int(S),
                                         _device_taps(L, rate).ptr, 1, MIN_SHIFT, MAX_SHIFT, d_scores.ptr, None))
    nat.check(lib.dsp_pitch_track_batch(d_scores.ptr, d_fo.ptr, len(so) - 1, n_lags, MIN_SHIFT, 2, d_pitch.ptr, None))
    return d_pitch.download((int(fo[-1]),), np.float64), fo


def _to_10k_on_device(d_clips, d_src_off, n_utt, n_samples_bound, rate, L, S, stream, arena=None):
    """preprocess.downsampling to 10 kHz for clips on the device (dsp_resample_layout_batch + dsp_decimate_batch) and the
    frame offsets of the result at (L, S) -> (p_x, p_so, d_fo): signal and sample offsets as pointers, frame offsets as
    a scratch buffer (``arena``: a buffer of the caller's arena instead, see ``_slot``)."""
    lib = nat.load()
    d_fo = _slot(arena, 'pitch_fo10', (n_utt + 1) * 8)
    if rate <= 10000:           # downsampling keeps every sample when the clip is at 10 kHz or below (preprocess.py:21-28)
        nat.check(lib.dsp_resample_layout_batch(d_src_off, n_utt, int(rate), 0, int(L), int(S), None, d_fo.ptr, stream))
        return d_clips, d_src_off, d_fo
    d_so10 = _slot(arena, 'pitch_so10', (n_utt + 1) * 8)
    d_x10 = _slot(arena, 'pitch_x10', max(4, int(n_samples_bound) * 4))
    nat.check(lib.dsp_resample_layout_batch(d_src_off, n_utt, int(rate), 10000, int(L), int(S), d_so10.ptr, d_fo.ptr, stream))
    nat.check(lib.dsp_decimate_batch(d_clips, d_src_off, d_so10.ptr, n_utt, int(n_samples_bound), int(rate), 10000, d_x10.ptr, stream))
    return d_x10.ptr, d_so10.ptr, d_fo


def pitch_tracks_device(d_clips, d_src_off, n_utt, n_samples_bound, rate, L, S, stream=None):
    """pitch.pitch_detect_sr for clips that are already on the device (fp32, concatenated, `rate` Hz): decimation to
    10 kHz, scores, smoothing, arg-max and octave repair, nothing leaves the device.  `stream` is None, a raw handle or
    a torch stream.  Returns (d_pitch [fp64, one per frame], d_frame_off [B+1]) as library scratch buffers."""
    lib = nat.load()
    stream = _stream_ptr(stream)
    p_x, p_so, d_fo = _to_10k_on_device(d_clips, d_src_off, n_utt, n_samples_bound, rate, L, S, stream)
    frames_bound = int(n_samples_bound) // int(S) + n_utt + 1
    n_lags = MAX_SHIFT - MIN_SHIFT
    d_scores = nat.SCRATCH.get('pitch_scores', frames_bound * n_lags * 4)
    d_pitch = nat.SCRATCH.get('pitch_track', frames_bound * 8)
    nat.check(lib.dsp_pitch_scores_batch(p_x, p_so, d_fo.ptr, n_utt, frames_bound, 0, int(L), int(S), _device_taps(L, 10000).ptr, 1,
                                         MIN_SHIFT, MAX_SHIFT, d_scores.ptr, stream))
    nat.check(lib.dsp_pitch_track_batch(d_scores.ptr, d_fo.ptr, n_utt, n_lags, MIN_SHIFT, 2, d_pitch.ptr, stream))
    return d_pitch, d_fo


def pitch_detect_sr(sig, rate, winlen=0.0512, step=0.01):
    """pitch.py:96-110 -> (pitch per frame in Hz, frames of the 10 kHz signal)."""
    s = downsampling(np.asarray(sig).reshape(-1), rate, 10000)
    L, S = int(10000 * winlen), int(step * 10000)          # to_frames truncates (sigproc.py:19)
    pitch, _ = pitch_tracks_batch(s, [0, len(s)], L, S)
    frames = to_frames(s, 10000, winlen, step)
    return list(pitch), frames


# ---- the cepstral tracker (pitch.py:83-94, 135-143, 227-242) and the pitch features (pitch.py:26-81, 245-279) ----

CEP_MIN, CEP_MAX = 20, 100            # pitch.py:232: peak-score candidates on the 10 kHz quefrency grid
N_AUX = 9                             # p, p_bias, start1, end1, start2, end2, len1, len2, valid


def _check(rc):
    """nat.check, but a rejected argument (a frame length the kernels do not serve) is the caller's ValueError."""
    if rc == nat.EINVAL:
        msg = nat.load().dsp_last_error()
        raise ValueError(msg.decode() if msg else 'invalid argument')
    nat.check(rc)


def _cepstrum_chain(p_x, p_so, p_fo, n_utt, frames_bound, L, S, stream=None, clip=True, want_scores=False, flags=3,
                    tail=True, d_feat=None, d_aux=None, arena=None):
    """The three launches behind the 10 kHz signal, on library scratch buffers (nothing is allocated once they exist).
    ``d_feat`` / ``d_aux``: the caller's own device memory ([n_utt, 5] fp64, [n_utt, 9] int32, raw pointers) for the two
    results instead of scratch.  ``arena``: a dict the caller owns -- every buffer of the chain, the FIR taps included, is
    then the arena's (``_slot``): what a captured graph needs, since a scratch slot may be freed by any later, larger call."""
    lib = nat.load()
    frames_bound = max(int(frames_bound), 1)
    out = types.SimpleNamespace(scores=None, feat=None, aux=None, seg=None)
    out.rows = _slot(arena, 'cep_rows', frames_bound * int(L) * 4)
    out.amp = _slot(arena, 'cep_amp', frames_bound * 8)
    out.pitch = _slot(arena, 'cep_pitch', frames_bound * 8)
    if want_scores:
        out.scores = _slot(arena, 'cep_scores', frames_bound * (CEP_MAX - CEP_MIN) * 4)
    _check(lib.dsp_pitch_cepstrum_batch(p_x, p_so, p_fo, n_utt, frames_bound, 0, int(L), int(S),
                                        _device_taps(L, 10000, 1000, arena).ptr, 1 if clip else 0, out.rows.ptr, out.amp.ptr, stream))
    _check(lib.dsp_pitch_cepstrum_track_batch(out.rows.ptr, 0, p_fo, n_utt, int(L), int(flags), out.pitch.ptr,
                                              out.scores.ptr if want_scores else None, stream))
    if tail:
        out.seg = _slot(arena, 'cep_seg', frames_bound * 8)
        out.feat = _slot(arena, 'cep_feat', n_utt * 5 * 8) if d_feat is None else types.SimpleNamespace(ptr=int(d_feat))
        out.aux = _slot(arena, 'cep_aux', n_utt * N_AUX * 4) if d_aux is None else types.SimpleNamespace(ptr=int(d_aux))
        _check(lib.dsp_pitch_feature_batch(out.pitch.ptr, out.amp.ptr, p_fo, n_utt, out.seg.ptr, out.feat.ptr, out.aux.ptr, stream))
    return out


def cepstrum_rows_batch(sig10k, sample_offsets, L, S, clip=True):
    """|cepstrum| rows [sum T_b, L] (fp64 copies of the kernel's fp32) and the per-frame sums of |x| for concatenated
    10 kHz signals; returns (rows, amp, frame_offsets)."""
    nat.require_device()
    d_x, d_so, d_fo, so, fo = _upload_10k(sig10k, sample_offsets, L, S)
    n = int(fo[-1])
    r = _cepstrum_chain(d_x.ptr, d_so.ptr, d_fo.ptr, len(so) - 1, n, L, S, clip=clip, want_scores=True, flags=0, tail=False)
    return r.rows.download((n, int(L)), np.float32).astype(np.float64), r.amp.download((n,), np.float64), fo


def pitch_detect_frame(frame, rate, gender='male'):
    """pitch.py:135-143 for one (already clipped) frame -> |cepstrum|, float64 [len(frame)]: a batch of one, clipping off."""
    frame = np.asarray(frame, dtype=np.float64).reshape(-1)
    L = len(frame)
    nat.require_device()
    d_x, d_so, d_fo, so, fo = _upload_10k(frame, [0, L], max(L, 1), max(L, 1))
    d_rows = nat.SCRATCH.get('cep_rows', max(L, 1) * 4)
    d_taps = nat.DeviceBuffer(max(L, 1) * 8)
    h = bandpass_taps(L, rate, 50, 1000, 'hamming') if L else np.zeros(0, dtype=complex)
    d_taps.upload(np.stack([h.real, h.imag], axis=1).astype(np.float32))
    try:
        _check(nat.load().dsp_pitch_cepstrum_batch(d_x.ptr, d_so.ptr, d_fo.ptr, 1, 1, 0, L, L, d_taps.ptr, 0, d_rows.ptr, None, None))
        return d_rows.download((L,), np.float32).astype(np.float64)
    finally:
        d_taps.free()


def _scores_on_device(rows, flags):
    """fp64 rows [T, n] through dsp_pitch_cepstrum_track_batch as a batch of one -> (scores [T, 80] int32, pitch or None).
    A row that is not a served length is padded with +inf: the walk up stops there exactly as it stops at the row's end."""
    nat.require_device()
    rows = np.asarray(rows, dtype=np.float64)
    T, n = rows.shape
    if n < CEP_MAX:
        raise IndexError(f'a row of {n} values has no candidate {CEP_MAX - 1}')          # as the reference's sig[i]
    L = 128
    while L < n:
        L <<= 1
    if L > 1024:
        raise ValueError(f'rows of {n} values are not served on the device (<= 1024)')
    if L != n:
        rows = np.concatenate([rows, np.full((T, L - n), np.inf)], axis=1)
    d_rows = nat.device_array('cep_rows64', np.ascontiguousarray(rows))
    d_fo = nat.device_array('pitch_rows_fo', np.array([0, T], dtype=np.int64))
    d_scores = nat.SCRATCH.get('cep_scores', T * (CEP_MAX - CEP_MIN) * 4)
    d_pitch = nat.SCRATCH.get('cep_pitch', T * 8)
    _check(nat.load().dsp_pitch_cepstrum_track_batch(d_rows.ptr, 1, d_fo.ptr, 1, L, int(flags), d_pitch.ptr, d_scores.ptr, None))
    return (d_scores.download((T, CEP_MAX - CEP_MIN), np.int32),
            d_pitch.download((T,), np.float64) if flags & 2 else None)


def peak_score(sig, gender='male'):
    """pitch.py:227-242: for i in [20, 100) the distance to the nearest larger value on either side -> list of 80 ints."""
    scores, _ = _scores_on_device(np.asarray(sig, dtype=np.float64).reshape(1, -1), 0)
    return [int(v) for v in scores[0]]


def _so_of(clips):
    return np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)


def pitch_cepstrum_tracks_batch(sig10k, sample_offsets, L, S):
    """pitch.pitch_detect's chain behind the decimation for concatenated 10 kHz signals.  Returns (pitch [sum T_b] in Hz,
    scores [sum T_b, 80] int32, frame_offsets)."""
    nat.require_device()
    d_x, d_so, d_fo, so, fo = _upload_10k(sig10k, sample_offsets, L, S)
    n = int(fo[-1])
    r = _cepstrum_chain(d_x.ptr, d_so.ptr, d_fo.ptr, len(so) - 1, n, L, S, want_scores=True, tail=False)
    return r.pitch.download((n,), np.float64), r.scores.download((n, CEP_MAX - CEP_MIN), np.int32), fo


def pitch_detect(sig, rate, winlen=0.0512, step=0.01, gender='male'):
    """pitch.py:83-94 -> (pitch per frame in Hz, frames of the 10 kHz signal)."""
    s = downsampling(np.asarray(sig).reshape(-1), rate, 10000)
    L, S = int(10000 * winlen), int(step * 10000)          # to_frames truncates (sigproc.py:19)
    pitch, _, _ = pitch_cepstrum_tracks_batch(s, [0, len(s)], L, S)
    return list(pitch), to_frames(s, 10000, winlen, step)


def sub_endpoint_detect(frames):
    """pitch.py:64-81: the frame where the amplitude dips most between two syllables (len // 2 when there is none);
    the search is dsp_pitch_feature_batch without a pitch track, as a batch of one."""
    amp = np.array([np.abs(f).sum() for f in frames], dtype=np.float64)
    T = len(amp)
    if T == 0:
        return 0
    nat.require_device()
    d_amp = nat.device_array('cep_amp', amp)
    d_fo = nat.device_array('pitch_rows_fo', np.array([0, T], dtype=np.int64))
    d_aux = nat.SCRATCH.get('cep_aux', N_AUX * 4)
    _check(nat.load().dsp_pitch_feature_batch(None, d_amp.ptr, d_fo.ptr, 1, None, None, d_aux.ptr, None))
    return int(d_aux.download((1,), np.int32)[0])


def find_smooth_subsequence(pitch, base_tor=3, base_thres=30, bias=0):
    """pitch.py:245-279 -> (accepted values of the longest smooth run, (start + bias, end + bias)), on the device."""
    v = np.ascontiguousarray(np.asarray(pitch, dtype=np.float64).reshape(-1))
    if len(v) == 0:
        raise ValueError('not enough values to unpack (expected 2, got 0)')           # what the reference's zip(*[]) raises
    nat.require_device()
    d_v = nat.device_array('cep_pitch', v)
    d_off = nat.device_array('pitch_rows_fo', np.array([0, len(v)], dtype=np.int64))
    d_seg = nat.SCRATCH.get('cep_seg', len(v) * 8)
    d_info = nat.SCRATCH.get('cep_aux', N_AUX * 4)
    _check(nat.load().dsp_pitch_smooth_subseq_batch(d_v.ptr, d_off.ptr, 1, int(base_tor), float(base_thres), d_seg.ptr, d_info.ptr, None))
    start, end, count = (int(x) for x in d_info.download((3,), np.int32))
    return list(d_seg.download((count,), np.float64)), (start + bias, end + bias)


def slope(seq):
    """pitch.py:49-52"""
    return np.polyfit(np.arange(0, len(seq)), seq, 1)[0]


def quad_params(seq):
    """pitch.py:54-57"""
    return np.polyfit(np.arange(0, len(seq)), seq, 2)[0]


def peakshift(seq1, seq2):
    """pitch.py:59-62"""
    return np.median(seq2) - np.median(seq1)


def pitch_features_device(d_clips, d_src_off, n_utt, n_samples_bound, rate, stream=None, L=512, S=100, d_feat=None, d_aux=None,
                          arena=None):
    """pitch.pitch_feature for clips that are already on the device (fp32, concatenated, `rate` Hz): decimation to 10 kHz,
    then the three launches of the cepstral path; nothing leaves the device.  `stream` is None, a raw handle or a torch
    stream.  Returns library scratch buffers as attributes: feat [B, 5] fp64, aux [B, 9] int32 (p, p_bias, start1,
    end1, start2, end2, len1, len2, valid), pitch and seg [one per frame] fp64, frame_off [B + 1] int64.  With ``d_feat`` /
    ``d_aux`` (raw device pointers) those two results go to the caller's memory, which the next call does not overwrite.
    With ``arena`` (a dict the caller owns and keeps alive, one per batch shape) every other buffer and the FIR taps are the
    arena's instead of library scratch: after one eager call that fills it, the launches can be captured in a graph."""
    stream = _stream_ptr(stream)
    p_x, p_so, d_fo = _to_10k_on_device(d_clips, d_src_off, n_utt, n_samples_bound, rate, L, S, stream, arena)
    # a clip of n samples keeps at most n * 10000 / rate + 2 of them and has at most 2 + kept / S frames
    kept_bound = int(n_samples_bound) if rate <= 10000 else int(n_samples_bound) * 10000 // int(rate) + 2 * n_utt
    frames_bound = kept_bound // int(S) + 2 * n_utt + 1
    out = _cepstrum_chain(p_x, p_so, d_fo.ptr, n_utt, frames_bound, L, S, stream=stream, d_feat=d_feat, d_aux=d_aux, arena=arena)
    out.frame_off = d_fo
    return out


def pitch_feature_batch(clips, sample_offsets, rate, details=False):
    """pitch.pitch_feature for a batch of host clips (concatenated, `rate` Hz, offsets [B + 1]) -> (feat [B, 5] fp64,
    valid [B] bool); rows of clips the reference raises on (a segment too short for the fits) are NaN with valid False.
    The clips are uploaded as fp32 and go through pitch_features_device.  details=True adds a dict with the per-frame
    pitch, the frame offsets, aux [B, 9] and the accepted values `seg`."""
    nat.require_device()
    so = np.ascontiguousarray(sample_offsets, dtype=np.int64)
    B = len(so) - 1
    x = np.ascontiguousarray(np.asarray(clips).reshape(-1), dtype=np.float32)
    d_x = nat.device_array('cep_clips', x if x.size else np.zeros(1, dtype=np.float32))
    d_so = nat.device_array('cep_clips_so', so)
    r = pitch_features_device(d_x.ptr, d_so.ptr, B, int(so[-1]), rate)
    feat = r.feat.download((B, 5), np.float64)
    aux = r.aux.download((B, N_AUX), np.int32)
    valid = aux[:, 8] != 0
    if not details:
        return feat, valid
    fo = r.frame_off.download((B + 1,), np.int64)
    n = int(fo[-1])
    return feat, valid, dict(pitch=r.pitch.download((n,), np.float64), frame_off=fo, aux=aux,
                             seg=r.seg.download((n,), np.float64))


def pitch_feature(sig, rate, gender='male'):
    """pitch.py:26-47 -> (slope1, slope2, quad1, quad2, peakshift), five numpy.float64."""
    sig = np.asarray(sig).reshape(-1)
    feat, valid = pitch_feature_batch(sig, [0, len(sig)], rate)
    if not valid[0]:
        raise ValueError('pitch_feature: a smooth pitch segment shorter than 3 frames cannot be fitted')
    return tuple(feat[0])
