"""The per-utterance glue model.py wraps around the feature path ("next" row f-1 of SURVEY 8f):
endpoint trim -> unit-variance scaling -> MFCC (with the (1, N) no-pre-emphasis quirk) -> global
mean removal -> delta(3) / delta-delta(3) -> per-coefficient z-score -> pad to 200 frames.

Round-1 form: composed from the GPU entry points of this package plus O(N) host reductions
(std of the trimmed clip, mean/std of the [T, 13] matrix).  Citations are file:line of the
reference's model.py.
"""
from __future__ import annotations

import numpy as np

from . import _native as nat
from . import endpoint as _endpoint
from .base import delta, mfcc
from .batch import _capture, _is_device_tensor, _stream_ptr, _wave_dtype_of
from .pipeline import VadMfccPipeline
from .pitch import pitch_detect_sr, pitch_tracks_device


def endpoint_detect(sig, rate, augment=False, rng=None):
    """model.py:52-64: trim to the detected endpoints (with augment=True widened by two draws of
    randint(0, int(0.1 * rate)) from ``rng`` -- a ``random.Random``, default the global generator the
    reference uses) and divide by the population standard deviation (sklearn
    ``scale(with_mean=False)``; a zero std divides by 1)."""
    left, right = _endpoint.basic_endpoint_detection(sig, rate)
    if augment:
        import random
        gen = rng if rng is not None else random
        hi = int(0.1 * rate)
        s_l, s_r = gen.randint(0, hi), gen.randint(0, hi)
        left, right = max(left - s_l, 0), max(right + s_r, 0)
    clip = np.asarray(sig[left:right], dtype=np.float64).reshape(-1, 1)
    sd = clip.std(axis=0)
    sd[sd == 0.0] = 1.0
    return clip / sd


def feature_extract_mfcc(sound, rate, nfft=1536):
    """model.py:66-88 -> ((mfcc0, mfcc1, mfcc2), min(T, 200))."""
    cfg = _endpoint.cfg
    m0 = mfcc(np.asarray(sound).reshape(1, -1), rate, winlen=cfg.frame, winstep=cfg.step, nfft=nfft,
              winfunc=np.hamming)
    m0 = m0 - np.mean(m0)
    m1 = delta(m0, 3)
    m2 = delta(m1, 3)
    mu, sd = m0.mean(axis=0), m0.std(axis=0)
    sd[sd == 0.0] = 1.0
    m0 = (m0 - mu) / sd
    return (m0, m1, m2), min(len(m0), 200)


def deviation(arr, smooth=1):
    """model.py:29-33: first difference at distance ``smooth``."""
    arr = np.asarray(arr, dtype=np.float64)
    return arr[smooth:] - arr[:len(arr) - smooth]


def feature_extract_pitch(sound, rate):
    """model.py:90-95, the optional pitch stream (cfg.use_pitch): pitch track / 150 and its
    first difference, both [T, 1]."""
    cfg = _endpoint.cfg
    pitch0, _ = pitch_detect_sr(np.asarray(sound).reshape(-1), rate, winlen=cfg.frame, step=cfg.step)
    pitch0 = np.array(pitch0).reshape(-1, 1) / 150
    return [pitch0.reshape(-1, 1), deviation(pitch0).reshape(-1, 1)]


def feature_extract_timespace(sound, rate):
    """model.py:97-101, the optional amplitude stream (cfg.use_timefeat): z-scored frame amplitude
    (population std, zero -> 1 as sklearn.scale) and its first difference, both [T, 1]."""
    cfg = _endpoint.cfg
    a = np.asarray(_endpoint.amplitude_feature(np.asarray(sound).reshape(-1), rate, winlen=cfg.frame, step=cfg.step),
                   dtype=np.float64)
    sd = a.std()
    amp0 = ((a - a.mean()) / (sd if sd != 0 else 1.0)).reshape(-1, 1)
    return [amp0, deviation(amp0).reshape(-1, 1)]


def pad200(b):
    """model.py:35-39: zero-pad or truncate a [T, D] stream to exactly 200 frames."""
    b = np.asarray(b)
    if len(b) < 200:
        return np.pad(b, ((0, 200 - len(b)), (0, 0)), 'constant', constant_values=0)
    return np.array(b[:200])


def model_pipeline(sig, rate, augment=False, rng=None):
    """Raw int16 clip -> ((mfcc0, mfcc1, mfcc2), n) exactly as RNNModel.get_batch_full feeds the
    classifier per utterance (model.py:113-124; augment=True is the training call of model.py:144)."""
    return feature_extract_mfcc(endpoint_detect(sig, rate, augment=augment, rng=rng), rate)


def model_pipeline_aug(sig, rate, seed):
    """The training path with the jitter drawn from ``random.Random(seed)`` (test hook: what the
    reference computes after ``random.seed(seed)``)."""
    import random
    return model_pipeline(sig, rate, augment=True, rng=random.Random(seed))


def batch_to_rnn_input(features, frame_offsets, max_len=200):
    """[sum T_b, D] device (torch) features + frame offsets -> ([max_len, B, D], len0) exactly as
    model.py:35-50,131-135 lays a batch out for the classifiers (`inp[T, B, 39]`, zero padded or
    truncated to 200 frames).  Stays on the device: no host round trip between the HIP front-end and
    the PyTorch-ROCm RNN."""
    import torch
    fo = torch.as_tensor(np.asarray(frame_offsets), device=features.device)
    B = fo.numel() - 1
    lens = (fo[1:] - fo[:-1]).clamp(max=max_len)
    t = torch.arange(max_len, device=features.device)[:, None]            # [max_len, 1]
    src = (fo[:-1][None, :] + t).clamp(max=features.shape[0] - 1)          # [max_len, B]
    inp = features[src]                                                     # [max_len, B, D]
    inp = inp * (t < lens[None, :]).unsqueeze(-1).to(features.dtype)
    return inp, lens.cpu().numpy()


def model_finalize(mfcc0, frame_offsets, delta_n=3, max_len=200):
    """Host-array form of dsp_model_finalize_batch: ``mfcc0`` [sum T_b, C] (the raw MFCCs of a
    batch) -> (inp [max_len, B, 3C] fp32, len0 [B]) as model.py:75-78 + 35-50 build them."""
    nat.require_device()
    lib = nat.load()
    m = np.ascontiguousarray(mfcc0, dtype=np.float32)
    fo = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    B, C = len(fo) - 1, m.shape[1]
    d_in = nat.device_array('fin_in', m)
    d_fo = nat.device_array('fin_fo', fo)
    d_out = nat.SCRATCH.get('fin_out', max_len * B * 3 * C * 4)
    d_len = nat.SCRATCH.get('fin_len', B * 4)
    nat.check(lib.dsp_model_finalize_batch(d_in.ptr, C, d_fo.ptr, B, C, int(delta_n), int(max_len), d_out.ptr,
                                           d_len.ptr, None))
    return d_out.download((max_len, B, 3 * C), np.float32), d_len.download((B,), np.int32)


class ModelFeatureBatch:
    """Batched, device-resident form of RNNModel.get_batch_full (model.py:113-135): endpointing ->
    (optional endpoint jitter, model.py:54-60) -> trim -> unit variance -> MFCC on the (1, N) view (no
    pre-emphasis, sigproc.py:185) -> minus the utterance's scalar mean -> delta(3), delta(delta, 3) ->
    z-score of the static coefficients -> [200, B, 39] zero padded.  Every step is a kernel behind the C
    ABI, queued on one stream with no host round trip in between (features/pipeline.py).  ``run``, ``enqueue`` and
    ``enqueue_placed`` are one launch sequence: ``pipe.launch``, then ``_after_launch``."""

    def __init__(self, rate, frame=0.03, step=0.01, nfft=1536, delta_n=3, max_len=200):
        self.rate = rate
        self.pipe = VadMfccPipeline(rate=rate, frame=frame, step=step, unit_variance=True, winlen=frame,
                                    winstep=step, nfft=nfft, preemph=0.0, winfunc=np.hamming)
        self.delta_n, self.max_len = delta_n, max_len

    def draw_jitter(self, n_utt, rng):
        """The augmentation of model.py:54-60 for a whole batch: (-randint(0, 0.1 rate), +randint(0, 0.1
        rate)) per utterance from ``rng`` (a random.Random, consumed in the reference's order: s_l then
        s_r, utterance by utterance)."""
        return MixedRateFeatureBatch.draw_jitter([self.rate] * n_utt, rng)

    def run(self, waves, sample_offsets=None, jitter=None, layout=None, use_pitch=False, use_timefeat=False, capacity=None):
        """-> (inp [max_len, B, 39 (+2) (+2)] torch tensor on the library's device, len0 [B], endpoints [B, 2]).
        ``capacity=N``: the eager, sync-free form on a capacity layout (``_run_capacity``): ``waves`` is a contiguous device
        tensor of exactly N samples, ``sample_offsets`` ([B + 1], host array or device tensor) any B lengths >= 1 that sum to
        at most N, and all three results stay on the device (len0 int32, endpoints int64).
        ``jitter``: int [B, 2] endpoint offsets (see draw_jitter) for the training path (augment=True);
        None = test path.  ``use_timefeat`` / ``use_pitch`` append the optional streams of model.py:125-128
        in the reference's order (pitch, then amplitude), both computed on the device from one trimmed, scaled
        fp32 copy of the clips (dsp_trim_scale_batch) and written into their columns of ``inp`` in place -- no clip and
        no track crosses PCIe.  ``waves`` may be any view of a device tensor: a non-contiguous one is copied once on
        torch's current stream (the stream of every launch here), and that copy is held until the call's last kernel has
        finished.  torch only owns the result tensor."""
        import torch
        if capacity is not None:
            if layout is not None or use_pitch or use_timefeat:
                raise NotImplementedError('run(capacity=) serves the default call: no layout=, no optional streams')
            return self._run_capacity(waves, sample_offsets, jitter, capacity)
        dev = waves.device if _is_device_tensor(waves) else torch.device('cuda', nat.current_device())
        stream = torch.cuda.current_stream(dev)
        if layout is None:       # this call consumes the layout's tables before it returns: a cached one is safe
            layout = self.pipe._cached_layout(sample_offsets, 0)
        # the clips are read where they lie (no trimmed fp32 copy): the MFCC kernel accumulates the unit-variance
        # statistics, the finalize kernel applies them to c0 as it reads
        (d_m0, lay), _, _ = self.pipe.run(waves, delta_n=0, download=False, layout=layout, jitter=jitter, defer_c0_shift=True)
        B = lay.n_utt
        width = 3 * self.pipe.features.C + (2 if use_pitch else 0) + (2 if use_timefeat else 0)
        inp = torch.empty((self.max_len, B, width), dtype=torch.float32, device=dev)
        len0 = torch.empty(B, dtype=torch.int32, device=dev)
        # host input: the pipeline ran on the legacy default stream, which orders against `stream`
        st = _stream_ptr(stream) if _is_device_tensor(waves) else None
        wave = d_m0.wave                      # the buffer pipe.run launched on, alive until d_m0 goes
        hold = self._after_launch(wave.ptr, wave.dtype, lay, d_m0.ptr, inp.data_ptr(), len0.data_ptr(), None, B, width, st, dev,
                                  use_pitch, use_timefeat)
        seg = lay.d_seg.download((B, 2), np.int64, st)       # first host synchronisation of the default call
        nat.check(nat.load().dsp_stream_synchronize(st))     # d_m0, its wave buffer and `hold` go on return: their consumers have finished
        del hold
        return inp, len0.cpu().numpy(), seg

    def _run_capacity(self, waves, sample_offsets, jitter, capacity):
        """``run(..., capacity=N)``: the launches ``capture(..., capacity=N)`` records, queued eagerly on torch's current
        stream on a capacity layout cached per (B, N) -- no layout build, upload or synchronisation per batch shape.  The
        padded grids make this a route of its own beside the exact-shape ``run``.  -> (inp, len0 int32 [B], endpoints int64
        [B, 2]), device tensors, valid after the stream's work; ``self.capacity_status`` is the layout's status word."""
        import torch
        from .pipeline import check_capacity_wave
        nat.require_device()
        check_capacity_wave(waves, capacity)
        dev, dtype = waves.device, _wave_dtype_of(waves)
        B = int(sample_offsets.shape[0] if torch.is_tensor(sample_offsets) else len(sample_offsets)) - 1
        lay = self.pipe._capacity_layout(B, capacity, 0)
        lay.write_offsets(sample_offsets)
        self.capacity_status = lay.status
        C = self.pipe.features.C
        m0 = torch.empty((max(lay.frames_bound, 1), C), dtype=torch.float32, device=dev)
        inp = torch.empty((self.max_len, B, 3 * C), dtype=torch.float32, device=dev)
        len0 = torch.empty(B, dtype=torch.int32, device=dev)
        d_jit = None
        if jitter is not None:
            j = jitter if torch.is_tensor(jitter) else torch.from_numpy(np.ascontiguousarray(jitter, dtype=np.int64))
            d_jit = j.to(device=dev, dtype=torch.int64).reshape(B, 2).contiguous()
        from .ensemble import _segments_tensor
        seg = _segments_tensor(lay, dev)          # the segment table as a torch tensor, swapped in BEFORE the launches write it
        self.enqueue(waves.data_ptr(), dtype, lay, m0.data_ptr(), inp.data_ptr(), len0.data_ptr(), torch.cuda.current_stream(dev),
                     d_jitter=None if d_jit is None else d_jit.data_ptr())
        return inp, len0, seg.clone()

    def enqueue(self, d_wave, wave_dtype, lay, d_m0, d_inp, d_len0, stream, d_jitter=None):
        """The default call (no optional streams) as launches only -- raw device pointers, nothing allocated,
        nothing synchronised: endpointing, the layout glue, the feature kernel on the clips in place and the finalize
        kernel.  ``d_m0``: [lay.frames_bound, C] fp32 scratch, ``d_inp``: [max_len, B, 3 C] fp32, ``d_len0``: [B] int32.
        ``d_jitter``: the endpoint offsets of the augmented front end (model.py:54-60; ``draw_jitter``) as a raw pointer to
        [B, 2] int64 in device memory, read in place by the launches; None = the test path."""
        self.enqueue_placed(d_wave, wave_dtype, lay, d_m0, d_inp, d_len0, None, lay.n_utt, 3 * self.pipe.features.C, stream, None,
                            d_jitter=d_jitter)

    def enqueue_placed(self, d_wave, wave_dtype, lay, d_m0, d_inp, d_len0, d_dst_col, n_cols, row_width, stream, dev,
                       d_jitter=None, use_pitch=False, use_timefeat=False):
        """``enqueue`` for a sub-batch of a larger one (MixedRateFeatureBatch): utterance b's rows go to
        ``d_inp[:, dst_col[b], 0:3 C]`` of a [max_len, n_cols, row_width] tensor and its length to ``d_len0[dst_col[b]]``
        (dsp_model_finalize_placed_batch; ``d_dst_col`` None = identity), the optional streams of ``run`` to the columns
        behind, in the reference's order (model.py:125-128).  Launches only; returns the temporaries the optional streams
        read, which the caller keeps until ``stream`` has finished.  Without optional streams nothing is allocated."""
        self.pipe.launch(d_wave, wave_dtype, lay, d_m0, stream, d_jitter, defer_c0_shift=True)
        return self._after_launch(d_wave, wave_dtype, lay, d_m0, d_inp, d_len0, d_dst_col, n_cols, row_width, _stream_ptr(stream), dev,
                                  use_pitch, use_timefeat)

    def _after_launch(self, d_wave, wave_dtype, lay, d_m0, d_inp, d_len0, d_dst_col, n_cols, row_width, st, dev,
                      use_pitch, use_timefeat):
        """Everything behind ``pipe.launch(..., defer_c0_shift=True)``, queued on the raw stream ``st``, always in placed form
        (``d_dst_col`` None, ``n_cols`` = B, ``row_width`` = the tensor's own width: the identity): the finalize kernel, then
        the optional streams at their column offsets.  Returns the temporaries to hold until ``st`` has finished."""
        lib = nat.load()
        B, C = lay.n_utt, self.pipe.features.C
        seg, work = (lay.d_seg.ptr, lay.d_work.ptr) if lay.c0_shift_pending else (None, None)
        nat.check(lib.dsp_model_finalize_placed_batch(d_m0, C, lay.d_frame_off.ptr, seg, work, B, C, self.delta_n, self.max_len,
                                                      d_inp, d_len0, d_dst_col, n_cols, row_width, 0, st))
        hold, col = [], 3 * C
        if (use_pitch or use_timefeat) and lay.c0_shift_pending:      # the trimmed, scaled clips themselves (model.py:62-63)
            nat.check(lib.dsp_trim_scale_batch(d_wave, wave_dtype, lay.vad.p_sample, lay.d_seg.ptr, lay.d_dst_off.ptr,
                                               B, 1, lay.d_trim.ptr, st))
        if use_pitch:
            self._pitch_streams(lay, st, (d_inp, d_dst_col, n_cols, row_width, col))
            col += 2
        if use_timefeat:
            hold += self._timefeat_streams(lay, st, dev, (d_inp, d_dst_col, n_cols, row_width, col))
        return hold

    def capture(self, waves, layout, capacity=None, census=False):
        """``census=True`` attaches ``g.census``, the node census of the recorded graph (features/graphcheck.py); the default records
        exactly as before.  A HIP graph of ``enqueue`` over device-resident ``waves`` (torch tensor, int16 / float32) and a prepared layout:
        ``g = mfb.capture(waves, lay)``; put new clips into ``waves`` -- of the same lengths, unless the layout is a capacity
        layout -- and call ``g.replay()`` ->
        (inp [max_len, B, 39], len0 [B] int32), both on the device, valid after the current stream's work (no host
        synchronisation).  One eager call runs first (it builds the layout's long-lived index tables).
        The graph reads ``waves`` at its address, sample after sample: a non-contiguous view cannot be served (a copy
        would not see what the caller writes later) and raises ValueError; a contiguous view at any offset is fine.

        ``capacity=N``: ``g = mfb.capture(waves, so, capacity=N)`` with ``waves`` a contiguous tensor of exactly N samples
        (ValueError otherwise) and ``so`` the [B + 1] sample offsets of the batch it holds now (or a layout from
        ``pipe.prepare_capacity(B, N, 0)``).  The graph then serves ANY B clips whose lengths are >= 1 and sum to at most N:
        write the clips into ``waves`` and their offsets into ``g.sample_offsets`` (int64 [B + 1] device tensor), replay;
        samples behind ``offsets[B]`` are ignored and ``g.status`` (int32 [1]) is 0 for a valid table (``CapacityLayout``).
        The result also carries the endpoints: (inp, len0, endpoints int64 [B, 2])."""
        if capacity is None and getattr(layout, 'capacity', None) is None:
            def prepare():
                import torch
                dev, dtype = waves.device, _wave_dtype_of(waves)
                C, B = self.pipe.features.C, layout.n_utt
                m0 = torch.empty((max(layout.frames_bound, 1), C), dtype=torch.float32, device=dev)
                inp = torch.empty((self.max_len, B, 3 * C), dtype=torch.float32, device=dev)
                len0 = torch.empty(B, dtype=torch.int32, device=dev)

                def queue():
                    self.enqueue(waves.data_ptr(), dtype, layout, m0.data_ptr(), inp.data_ptr(), len0.data_ptr(),
                                 torch.cuda.current_stream(dev))
                    return inp, len0
                return queue, [m0, layout]
            return _capture(waves, prepare, census)

        from .pipeline import CapacityLayout, check_capacity_wave
        lay_box = []

        def prepare_capacity():
            import torch
            from .ensemble import _segments_tensor
            lay = layout
            if not isinstance(lay, CapacityLayout):
                so = np.ascontiguousarray(layout, dtype=np.int64).reshape(-1)
                lay = self.pipe.prepare_capacity(len(so) - 1, capacity, 0)      # the graph's own
                lay.write_offsets(so)
            elif capacity is not None and int(capacity) != lay.capacity:
                raise ValueError(f'capacity = {capacity}, the layout was prepared for {lay.capacity}')
            check_capacity_wave(waves, lay.capacity)
            lay_box.append(lay)
            dev, dtype = waves.device, _wave_dtype_of(waves)
            C, B = self.pipe.features.C, lay.n_utt
            m0 = torch.empty((max(lay.frames_bound, 1), C), dtype=torch.float32, device=dev)
            inp = torch.empty((self.max_len, B, 3 * C), dtype=torch.float32, device=dev)
            len0 = torch.empty(B, dtype=torch.int32, device=dev)
            seg = _segments_tensor(lay, dev)

            def queue():
                self.enqueue(waves.data_ptr(), dtype, lay, m0.data_ptr(), inp.data_ptr(), len0.data_ptr(),
                             torch.cuda.current_stream(dev))
                return inp, len0, seg
            return queue, [m0, lay]
        g = _capture(waves, prepare_capacity, census)
        g.sample_offsets, g.status = lay_box[0].sample_offsets_in, lay_box[0].status
        return g

    def _timefeat_streams(self, lay, st, dev, place):
        """Z-scored frame amplitude of the trimmed, scaled clips and its first difference (model.py:97-101), on the
        device -- at the amplitude stream's OWN framing (int(rate * cfg.frame), int(cfg.step * rate): to_frames truncates,
        sigproc.py:19; the MFCC framing rounds half up, so the two differ at e.g. 22.05 kHz): its frame offsets come from
        one small launch over the trimmed offsets.  ``place`` = (d_out, d_dst_col, n_cols, row_width, col_offset): where the
        two columns go (dsp_model_timefeat_placed_batch).  Returns the temporaries for the caller to hold."""
        import torch
        lib = nat.load()
        ep, fp = self.pipe.endpoint, self.pipe.features
        L2, S2 = int(self.rate * ep.frame), int(ep.step * self.rate)       # to_frames truncation, sigproc.py:19
        B = lay.n_utt
        d_fo2 = None
        if (L2, S2) == (fp.L, fp.S):
            p_fo, frames_bound = lay.d_frame_off.ptr, lay.frames_bound
        else:
            d_fo2 = torch.empty(B + 1, dtype=torch.int64, device=dev)
            nat.check(lib.dsp_resample_layout_batch(lay.d_dst_off.ptr, B, int(self.rate), 0, L2, S2, None, d_fo2.data_ptr(), st))
            p_fo, frames_bound = d_fo2.data_ptr(), int(lay.total_samples) // S2 + B + 1
        d_amp = torch.empty(max(frames_bound, 1), dtype=torch.float64, device=dev)
        d_zcr = torch.empty(max(frames_bound, 1), dtype=torch.int32, device=dev)
        nat.check(lib.dsp_vad_features_batch(lay.d_trim.ptr, nat.WAVE_F32, lay.d_dst_off.ptr, p_fo, B,
                                             frames_bound, 0, L2, S2, 0, d_amp.data_ptr(), d_zcr.data_ptr(), st))
        nat.check(lib.dsp_model_timefeat_placed_batch(d_amp.data_ptr(), p_fo, B, L2, self.max_len, *place, st))
        return [d_amp, d_zcr, d_fo2]

    def _pitch_streams(self, lay, st, place):
        """Pitch track / 150 and its first difference (model.py:90-95) of the trimmed, scaled clips, on the device:
        decimation to 10 kHz (an index selection, preprocess.py:21-28), frame scores, smoothing, arg-max, octave repair
        (pitch.py:96-206) and the two columns at ``place`` (as in _timefeat_streams; dsp_model_pitchfeat_placed_batch) --
        six launches, no clip and no track crosses PCIe.  The track is library scratch that later launches on the same
        stream may reuse, so there is nothing to hold."""
        cfg = _endpoint.cfg
        L, S = int(10000 * cfg.frame), int(cfg.step * 10000)
        d_pitch, d_fo = pitch_tracks_device(lay.d_trim.ptr, lay.d_dst_off.ptr, lay.n_utt, int(lay.total_samples), self.rate, L, S, st)
        nat.check(nat.load().dsp_model_pitchfeat_placed_batch(d_pitch.ptr, d_fo.ptr, lay.n_utt, self.max_len, *place, st))


# ---- mixed sample rates in one batch ---------------------------------------------------------------------------------
# reader.mini_batch_iterator shuffles the file list and yields feat = [(sig, rate), ...] (reader.py:80); the recordings are
# at 44.1 kHz and 48 kHz, and model.py:114-135 treats every clip at its own rate.  Framing, window, mel table and the VAD
# frames differ per rate, so a mixed batch runs as one sub-batch per distinct rate, one after the other on one stream, each
# writing its rows straight into the shared [200, B, width] tensor (the placed entry points of include/dsp_frontend.h).


class RateGroup:
    """The clips of one sample rate in a batch: ``index`` (int32, ascending batch positions -- the sub-batch's order, its
    pick list and its destination columns at once) and whether they are one contiguous run of the batch."""

    def __init__(self, rate, index):
        self.rate = int(rate)
        self.index = np.ascontiguousarray(index, dtype=np.int32)
        self.contiguous = bool(self.index[-1] - self.index[0] + 1 == len(self.index))


def group_by_rate(rates):
    """[B] rates -> RateGroups in order of first appearance, batch order kept inside a group; their ``index`` arrays
    partition range(B)."""
    rates = np.asarray(rates).reshape(-1)
    seen = {}
    for b, r in enumerate(rates.tolist()):
        seen.setdefault(int(r), []).append(b)
    return [RateGroup(r, idx) for r, idx in seen.items()]


def _as_rates(rates):
    r = np.asarray(rates).reshape(-1)
    if r.size and not np.issubdtype(r.dtype, np.integer):
        if not np.all(r == np.floor(r)):
            raise ValueError('sample rates must be whole numbers')
        r = r.astype(np.int64)
    if np.any(r <= 0):
        raise ValueError(f'sample rates must be positive, got {r[r <= 0].tolist()}')
    return r.astype(np.int64)


def _no_mixed_capacity(capacity):
    if capacity is not None:
        raise NotImplementedError('capacity= is not served for mixed-rate batches by this class: its grouping by rate is host logic over '
                                  'the rates (group_by_rate), so the layout of a mixed batch cannot be rebuilt on the device here; use '
                                  'MixedRateCapacityBatch (features, default call), train.MixedRateTrainBatch or '
                                  'ensemble.MixedRateCapacityEnsembleBatch, which group on the device, or the single-rate classes')


class _MixedPlan:
    """Everything about a mixed-rate batch that depends only on its sample offsets and rates: the groups, each group's
    rebased offsets and pipeline layout, and the small device tables of the placement and the gather."""

    def __init__(self, owner, so, rates, dev, device_input):
        import torch
        self.so, self.B = so, len(so) - 1
        self.groups = group_by_rate(rates)
        identity = len(self.groups) == 1
        self.d_so = None
        lens = np.diff(so)
        for g in self.groups:
            g.so = np.concatenate(([0], np.cumsum(lens[g.index]))).astype(np.int64)
            g.lay = owner._mfb(g.rate).pipe.prepare(g.so, 0)
            g.d_index = None if identity else torch.from_numpy(g.index).to(dev)
            g.d_dst_off = None
            if device_input and not g.contiguous:           # interleaved clips on the device: dsp_gather_clips_batch
                if self.d_so is None:
                    self.d_so = torch.from_numpy(so).to(dev)
                g.d_dst_off = torch.from_numpy(g.so).to(dev)
        self.order = np.concatenate([g.index for g in self.groups])


class MixedRateFeatureBatch:
    """RNNModel.get_batch_full (model.py:113-135) for a batch whose clips have different sample rates: one
    ModelFeatureBatch per rate seen (created on first use), the rate groups processed in order of first appearance on one
    stream, every group's rows -- and the optional streams of model.py:125-128 -- written in place into one
    [max_len, B, width] tensor in batch order.  No torch.cat, no permutation pass, one host synchronisation at the end."""

    def __init__(self, frame=0.03, step=0.01, nfft=1536, delta_n=3, max_len=200):
        import threading
        self.frame, self.step, self.nfft, self.delta_n, self.max_len = frame, step, nfft, delta_n, max_len
        self._by_rate = {}
        self._tls = threading.local()   # per thread: the plans of the last few batch shapes (VadMfccPipeline._cached_layout)

    def _mfb(self, rate):
        mfb = self._by_rate.get(int(rate))
        if mfb is None:
            mfb = self._by_rate[int(rate)] = ModelFeatureBatch(int(rate), frame=self.frame, step=self.step, nfft=self.nfft,
                                                               delta_n=self.delta_n, max_len=self.max_len)
        return mfb

    @staticmethod
    def draw_jitter(rates, rng):
        """The augmentation of model.py:54-60 in the reference's consumption order (model.py:55-58): for b in batch order
        -rng.randint(0, int(0.1 * rates[b])), then +rng.randint(0, int(0.1 * rates[b])) -> int64 [B, 2]."""
        rates = np.asarray(rates).reshape(-1)
        j = np.empty((len(rates), 2), dtype=np.int64)
        for b, r in enumerate(rates.tolist()):
            hi = int(0.1 * r)
            j[b, 0] = -rng.randint(0, hi)
            j[b, 1] = rng.randint(0, hi)
        return j

    # ---- inputs ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _inputs(waves, sample_offsets, rates):
        """-> (clips, so, rates): ``clips`` a 1-D device tensor, or a list of B host arrays; ValueError before any device
        work for a rate list of the wrong length or a non-positive rate."""
        rates = _as_rates(rates)
        if isinstance(waves, (list, tuple)):
            clips = [np.asarray(c).reshape(-1) for c in waves]
            so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
        else:
            if sample_offsets is None:
                raise ValueError('concatenated waves need sample_offsets')
            so = np.ascontiguousarray(sample_offsets, dtype=np.int64).reshape(-1)
            if _is_device_tensor(waves):
                if waves.dim() != 1:
                    raise ValueError('device waves must be 1-D (a view such as buf[:, 0] is fine)')
                clips = waves
            else:
                flat = np.asarray(waves).reshape(-1)
                clips = [flat[so[b]:so[b + 1]] for b in range(len(so) - 1)]
        if len(so) < 2:
            raise ValueError('an empty batch')
        if len(rates) != len(so) - 1:
            raise ValueError(f'{len(rates)} rates for {len(so) - 1} clips')
        return clips, so, rates

    def _plan(self, so, rates, dev, device_input):
        cache = getattr(self._tls, 'plans', None)
        if cache is None:
            cache = self._tls.plans = {}
        key = (dev.index, bool(device_input), so.tobytes(), rates.tobytes())
        plan = cache.pop(key, None)
        if plan is None:
            plan = _MixedPlan(self, so, rates, dev, device_input)
            while len(cache) >= 4:
                cache.pop(next(iter(cache)))
        cache[key] = plan              # most recently used last
        return plan

    @staticmethod
    def _group_wave(clips, plan, g, dev, st):
        """The clips of group ``g`` as one contiguous 1-D device tensor: a view of a device batch where they form one run,
        one gather launch where they do not, one upload of the host clips concatenated per rate."""
        import torch
        if not _is_device_tensor(clips):
            parts = [nat.as_wave(clips[b]) for b in g.index]
            if any(dt != nat.WAVE_I16 for _, dt in parts):
                parts = [(np.asarray(a, dtype=np.float32), nat.WAVE_F32) for a, _ in parts]
            return torch.from_numpy(np.concatenate([a for a, _ in parts])).to(dev)
        if g.contiguous:
            lo = int(plan.so[g.index[0]])
            return clips[lo:lo + int(g.so[-1])]
        out = torch.empty(max(int(g.so[-1]), 1), dtype=clips.dtype, device=dev)
        nat.check(nat.load().dsp_gather_clips_batch(clips.data_ptr(), _wave_dtype_of(clips), plan.d_so.data_ptr(), g.d_index.data_ptr(),
                                                    len(g.index), g.d_dst_off.data_ptr(), out.data_ptr(), st))
        return out

    # ---- the call ----------------------------------------------------------------------------------------------------
    def _launch(self, waves, sample_offsets, rates, jitter=None, use_pitch=False, use_timefeat=False, plan=None):
        """Queue the whole batch on torch's current stream -> a namespace (inp, len0 on the device, plan, waves per group,
        hold: every temporary a launch reads).  Nothing is synchronised once the plan of the batch shape exists."""
        import types
        import torch
        clips, so, rates = self._inputs(waves, sample_offsets, rates)
        nat.require_device()
        B = len(so) - 1
        on_device = _is_device_tensor(clips)
        if on_device and clips.device.index != nat.current_device():
            raise nat.DspError(f'waveforms live on cuda:{clips.device.index}, the library is on device '
                               f'{nat.current_device()} (dsp_set_device)')
        dev = clips.device if on_device else torch.device('cuda', nat.current_device())
        stream = torch.cuda.current_stream(dev)
        st = _stream_ptr(stream)
        hold = []
        if on_device:
            _wave_dtype_of(clips)                    # TypeError for anything but int16 / float32
            if not clips.is_contiguous():            # a strided view: one copy on the stream of the launches, held to the end
                clips = clips.contiguous()
            hold.append(clips)
        if plan is None:
            plan = self._plan(so, rates, dev, on_device)
        C = plan.groups[0].lay.D
        width = 3 * C + (2 if use_pitch else 0) + (2 if use_timefeat else 0)
        inp = torch.empty((self.max_len, B, width), dtype=torch.float32, device=dev)
        len0 = torch.empty(B, dtype=torch.int32, device=dev)
        d_jit = None
        if jitter is not None:                       # one upload, rows in group order: each group reads its own slice
            j = np.ascontiguousarray(jitter, dtype=np.int64).reshape(B, 2)
            d_jit = torch.from_numpy(np.ascontiguousarray(j[plan.order])).to(dev)
            hold.append(d_jit)
        group_waves, row = [], 0
        for g in plan.groups:
            wave = self._group_wave(clips, plan, g, dev, st)
            m0 = torch.empty(max(g.lay.frames_bound, 1) * C, dtype=torch.float32, device=dev)
            group_waves.append(wave)
            hold += [wave, m0]
            hold += self._mfb(g.rate).enqueue_placed(
                wave.data_ptr(), _wave_dtype_of(wave), g.lay, m0.data_ptr(), inp.data_ptr(), len0.data_ptr(),
                None if g.d_index is None else g.d_index.data_ptr(), B, width, stream, dev,
                d_jitter=None if d_jit is None else d_jit.data_ptr() + 16 * row, use_pitch=use_pitch, use_timefeat=use_timefeat)
            row += len(g.index)
        return types.SimpleNamespace(inp=inp, len0=len0, plan=plan, group_waves=group_waves, hold=hold, st=st, dev=dev)

    @staticmethod
    def _finish(ctx):
        """Endpoints [B, 2] (samples of each clip's own rate, endpoint.py:64) and len0 to the host: the call's one
        synchronisation; afterwards the temporaries of the launches may go."""
        plan = ctx.plan
        endpoints = np.zeros((plan.B, 2), dtype=np.int64)
        for g in plan.groups:
            endpoints[g.index] = g.lay.d_seg.download((len(g.index), 2), np.int64, ctx.st)
        nat.check(nat.load().dsp_stream_synchronize(ctx.st))
        len0 = ctx.len0.cpu().numpy()
        ctx.hold = []
        return len0, endpoints

    def run(self, waves, sample_offsets=None, rates=None, jitter=None, use_pitch=False, use_timefeat=False, capacity=None):
        """``capacity=``: NotImplementedError -- see ``capture`` (``MixedRateCapacityBatch.run`` serves it).
        ``waves``: concatenated clips as a host 1-D array or a 1-D device tensor (int16 / float32, any view) with
        ``sample_offsets`` [B + 1], or a list of B host arrays; ``rates``: [B] sample rates.  -> (inp [max_len, B, 39 (+2)
        (+2)] on the library's device, len0 [B], endpoints [B, 2]), all in batch order; ``jitter`` / ``use_pitch`` /
        ``use_timefeat`` as ModelFeatureBatch.run, each clip at its own rate's framings and decimation (model.py:90-101).
        A batch with a single rate is ModelFeatureBatch(rate).run."""
        _no_mixed_capacity(capacity)
        ctx = self._launch(waves, sample_offsets, rates, jitter, use_pitch, use_timefeat)
        len0, endpoints = self._finish(ctx)
        return ctx.inp, len0, endpoints

    def capture(self, waves, sample_offsets, rates, capacity=None):
        """A HIP graph of the default call over device-resident ``waves`` (contiguous 1-D tensor, int16 / float32):
        ``g = mr.capture(waves, so, rates)``; write new clips of the same lengths and rates into ``waves`` and call
        ``g.replay()`` -> (inp [max_len, B, 39], len0 [B] int32), on the device, valid after the current stream's work (no
        host synchronisation).  The sub-pipelines are queued one after the other on the capture stream: the graph is one
        chain, no forked branches.  One eager call runs first (it builds the layouts' long-lived index tables).
        ``capacity=`` raises NotImplementedError: which clips form a rate group, each group's offsets and its share of the
        samples are host logic over the rates (``group_by_rate``), so a mixed-rate graph of THIS class stays bound to its lengths
        AND rates; ``MixedRateCapacityBatch`` groups on the device and takes ``capacity=``, as the single-rate classes do."""
        _no_mixed_capacity(capacity)

        def prepare():
            _, so, r = self._inputs(waves, sample_offsets, rates)
            plan = _MixedPlan(self, so, r, waves.device, True)     # the graph's own: nothing else writes its tables
            hold = [plan]

            def queue():
                ctx = self._launch(waves, so, r, plan=plan)
                hold[1:] = [ctx.hold]          # the captured call's temporaries (the warm call's go)
                return ctx.inp, ctx.len0
            return queue, hold
        return _capture(waves, prepare)


# ---- mixed sample rates through one recorded launch sequence: the grouping itself on the device ------------------------
# group_by_rate and _MixedPlan above are host logic over the rates, so a graph of MixedRateFeatureBatch is bound to its
# lengths AND rates.  Here the stable partition, each group's rebased offsets, the gather, the placement columns and the
# endpoints' way back to batch order are launches over device tables (dsp_rate_groups_batch, dsp_gather_groups_batch,
# dsp_scatter_segments_batch): every rate of a fixed table gets a group of exactly B slots -- its clips, then pad clips of
# PAD_SAMPLES samples that are computed and written nowhere -- on a capacity layout of its own.

PAD_SAMPLES = 1      # the shortest clip a capacity layout declares valid (status 0): one VAD frame, one MFCC frame, zero variance
MAX_RATE_GROUPS = 4  # DSP_MAX_RATE_GROUPS


def _rate_table(rates):
    """The table of known rates of a MixedRateCapacityBatch: 1 .. 4 distinct positive whole numbers; ValueError otherwise."""
    table = tuple(int(r) for r in _as_rates(rates))
    if not 1 <= len(table) <= MAX_RATE_GROUPS:
        raise ValueError(f'a rate table holds 1 .. {MAX_RATE_GROUPS} rates, got {len(table)}')
    if len(set(table)) != len(table):
        raise ValueError(f'a rate table holds distinct rates, got {list(table)}')
    if max(table) > 2 ** 31 - 1:
        raise ValueError(f'sample rates must fit int32, got {list(table)}')
    return table


class _MixedCapacityArena:
    """Everything one (B, N, sample type) of a MixedRateCapacityBatch launches on: the tensors the caller's batch is written
    into (``sample_offsets``, ``rates``, ``jitter``), the sanitised source table, and per table rate a capacity layout for B
    clips of N + B * PAD_SAMPLES samples, its wave buffer, cepstra and small tables.  The host arrays of table pointers the
    three grouping entry points take are kept here too."""

    def __init__(self, owner, B, N, dev, torch_dtype):
        import ctypes as C
        import torch
        from .ensemble import _segments_tensor
        self.B, self.N, self.dev = B, N, dev
        G = self.G = len(owner.rates)
        self.sample_offsets = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        self.rates = torch.full((B,), owner.rates[0], dtype=torch.int32, device=dev)
        self.jitter = torch.zeros((B, 2), dtype=torch.int64, device=dev)
        self.sanitised = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        self.count = torch.zeros(G, dtype=torch.int32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        cap = N + B * PAD_SAMPLES
        self.lays, self.waves, self.m0, self.pick, self.dst_col, self.group_jitter, self.seg = [], [], [], [], [], [], []
        for mfb in owner.groups:
            lay = mfb.pipe.prepare_capacity(B, cap, 0)
            self.lays.append(lay)
            # whole 16-byte vectors, and one to spare behind the last sample: the vector kernels load aligned vectors that may
            # reach past a clip's end (they mask what they loaded), and the capacity handles need the aligned start
            self.waves.append(torch.zeros((cap + 15) // 8 * 8 + 8, dtype=torch_dtype, device=dev))
            self.m0.append(torch.empty((max(lay.frames_bound, 1), mfb.pipe.features.C), dtype=torch.float32, device=dev))
            self.pick.append(torch.full((B,), -1, dtype=torch.int32, device=dev))
            self.dst_col.append(torch.full((B,), -1, dtype=torch.int32, device=dev))
            self.group_jitter.append(torch.zeros((B, 2), dtype=torch.int64, device=dev))
            self.seg.append(_segments_tensor(lay, dev))

        def ptrs(tensors):
            return (C.c_void_p * G)(*[t.data_ptr() for t in tensors])
        self.h_rates = (C.c_int32 * G)(*owner.rates)
        self.p_pick, self.p_dst_col, self.p_jitter = ptrs(self.pick), ptrs(self.dst_col), ptrs(self.group_jitter)
        self.p_offsets = ptrs([lay.sample_offsets_in for lay in self.lays])
        self.p_waves, self.p_seg = ptrs(self.waves), ptrs(self.seg)

    def write(self, sample_offsets, rates, jitter):
        """Copy a batch's tables ([B + 1] offsets, [B] rates, [B, 2] jitter or None: host arrays or device tensors) into the
        tensors the launches read, on torch's current stream; ValueError for a table of another shape (the values are the
        device's to check: ``status``)."""
        import torch

        def put(dst, src, np_dtype, what):
            t = src if torch.is_tensor(src) else torch.from_numpy(np.ascontiguousarray(src, dtype=np_dtype))
            if tuple(t.shape) != tuple(dst.shape):
                raise ValueError(f'{what} must be {list(dst.shape)}, got {list(t.shape)}')
            dst.copy_(t)
        put(self.sample_offsets, sample_offsets, np.int64, 'sample_offsets')
        put(self.rates, rates, np.int32, 'rates')
        if jitter is not None:
            put(self.jitter, jitter, np.int64, 'jitter')


class MixedRateCapacityBatch:
    """RNNModel.get_batch_full (model.py:113-135) for ANY batch of B clips at the rates of a fixed table (reader.py:80 yields
    44.1 and 48 kHz files in shuffled order) whose lengths are >= 1 and sum to at most N, as one launch sequence that reads
    lengths, rates and jitter from device memory -- the default call (no optional streams), capacity routes only:

      dsp_rate_groups_batch     the source table sanitised, the stable partition by rate (``group_by_rate``'s order), each group's
                                rebased offsets straight into its CapacityLayout.sample_offsets_in, pick / placement / jitter tables
      dsp_gather_groups_batch   every clip to its group's wave buffer, pad slots filled; one launch for all groups
      per table rate            ``ModelFeatureBatch.enqueue_placed`` unchanged, on the group's buffer, with its dst_col and jitter
      dsp_scatter_segments_batch  the endpoints back to batch order

    One chain, no forked branches, no memset, no pooled workspace, no scratch slot: ``capture`` records exactly what ``run``
    queues.  A group has B slots whatever the rates are; the slots behind its clips hold pad clips of PAD_SAMPLES samples,
    whose rows the finalize kernel skips (negative column).  ``status`` (int32 [1]): bits 0-3 as ``CapacityLayout.status``,
    judged on the caller's table; bit 4: a rate outside the table -- that clip ran at ``rates[0]``."""

    def __init__(self, rates=(44100, 48000), frame=0.03, step=0.01, nfft=1536, delta_n=3, max_len=200):
        self.rates = _rate_table(rates)
        self.groups = [ModelFeatureBatch(r, frame=frame, step=step, nfft=nfft, delta_n=delta_n, max_len=max_len) for r in self.rates]
        self.max_len = max_len
        self.C = self.groups[0].pipe.features.C
        self._arenas = {}

    draw_jitter = staticmethod(MixedRateFeatureBatch.draw_jitter)

    def prepare(self, n_utt, capacity, waves):
        """An arena of its own for (n_utt, capacity) and the sample type and device of ``waves``."""
        nat.require_device()
        _wave_dtype_of(waves)
        n_utt, capacity = int(n_utt), int(capacity)
        if n_utt < 1 or capacity < 1:
            raise ValueError(f'need n_utt >= 1 and capacity >= 1, got {n_utt}, {capacity}')
        return _MixedCapacityArena(self, n_utt, capacity, waves.device, waves.dtype)

    def _arena(self, n_utt, capacity, waves):
        """``run``: one arena per (device, B, N, sample type), a few kept, the most recently used last."""
        key = (waves.device.index, int(n_utt), int(capacity), str(waves.dtype))
        arena = self._arenas.pop(key, None)
        if arena is None:
            arena = self.prepare(n_utt, capacity, waves)
            while len(self._arenas) >= 4:
                self._arenas.pop(next(iter(self._arenas)))
        self._arenas[key] = arena
        return arena

    @staticmethod
    def _n_utt(sample_offsets):
        import torch
        n = int(sample_offsets.shape[0] if torch.is_tensor(sample_offsets) else len(sample_offsets)) - 1
        if n < 1:
            raise ValueError('an empty batch')
        return n

    def enqueue(self, waves, arena, inp, len0, endpoints, use_jitter, stream):
        """The whole sequence as launches on ``stream`` (a torch stream): nothing allocated, nothing synchronised.  ``waves``:
        the [N] source tensor; ``inp`` [max_len, B, 3 C] fp32, ``len0`` [B] int32, ``endpoints`` [B, 2] int64: every element
        of all three is written, since the groups partition the batch."""
        lib, st, B, G = nat.load(), _stream_ptr(stream), arena.B, arena.G
        dtype = _wave_dtype_of(waves)
        nat.check(lib.dsp_rate_groups_batch(arena.rates.data_ptr(), arena.sample_offsets.data_ptr(),
                                            arena.jitter.data_ptr() if use_jitter else None, B, arena.N, G, arena.h_rates, PAD_SAMPLES,
                                            arena.sanitised.data_ptr(), arena.p_pick, arena.p_dst_col, arena.p_offsets,
                                            arena.p_jitter if use_jitter else None, arena.count.data_ptr(), arena.status.data_ptr(), st))
        nat.check(lib.dsp_gather_groups_batch(waves.data_ptr(), dtype, arena.sanitised.data_ptr(), B, G, arena.p_pick, arena.p_offsets,
                                              PAD_SAMPLES, arena.p_waves, st))
        for g, mfb in enumerate(self.groups):
            mfb.enqueue_placed(arena.waves[g].data_ptr(), dtype, arena.lays[g], arena.m0[g].data_ptr(), inp.data_ptr(), len0.data_ptr(),
                               arena.dst_col[g].data_ptr(), B, 3 * self.C, stream, arena.dev,
                               d_jitter=arena.group_jitter[g].data_ptr() if use_jitter else None)
        nat.check(lib.dsp_scatter_segments_batch(arena.p_seg, arena.p_dst_col, B, G, endpoints.data_ptr(), st))

    def _outputs(self, B, dev):
        import torch
        return (torch.empty((self.max_len, B, 3 * self.C), dtype=torch.float32, device=dev),
                torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int64, device=dev))

    def run(self, waves, sample_offsets, rates, jitter=None, capacity=None):
        """Eager and sync-free: ``waves`` a contiguous device tensor of exactly ``capacity`` = N samples (int16 / float32;
        ValueError otherwise), ``sample_offsets`` [B + 1], ``rates`` [B] and ``jitter`` ([B, 2], ``draw_jitter``; None = the test
        path) host arrays or device tensors.  -> (inp [max_len, B, 39], len0 int32 [B], endpoints int64 [B, 2], status int32
        [1]): device tensors in batch order, valid after the current stream's work.  Exactly the launches ``capture`` records,
        on an arena cached per (B, N)."""
        import torch
        from .pipeline import check_capacity_wave
        if capacity is None:
            raise ValueError('MixedRateCapacityBatch serves capacity routes only: pass capacity=N (MixedRateFeatureBatch.run takes exact shapes)')
        check_capacity_wave(waves, capacity)
        arena = self._arena(self._n_utt(sample_offsets), capacity, waves)
        arena.write(sample_offsets, rates, jitter)
        inp, len0, endpoints = self._outputs(arena.B, waves.device)
        self.enqueue(waves, arena, inp, len0, endpoints, jitter is not None, torch.cuda.current_stream(waves.device))
        return inp, len0, endpoints, arena.status

    def capture(self, waves, sample_offsets, rates, jitter=None, capacity=None):
        """A HIP graph of ``run``'s launches over ``waves`` (contiguous [N] device tensor) and the batch it holds now:
        ``g = mc.capture(waves, so, rates, jitter, capacity=N)``.  Before a ``g.replay()`` write the next batch's clips into
        ``waves``, its offsets into ``g.sample_offsets`` (int64 [B + 1]), its rates into ``g.rates`` (int32 [B]) and, if the
        graph was recorded with jitter, its rows into ``g.jitter`` (int64 [B, 2]); ANY B clips at the table's rates whose
        lengths are >= 1 and sum to at most N are served, in any order of rates.  ``replay()`` -> (inp, len0, endpoints) on
        the device; ``g.status`` as ``run``'s."""
        import torch
        from .pipeline import check_capacity_wave
        if capacity is None:
            raise ValueError('MixedRateCapacityBatch serves capacity routes only: pass capacity=N')
        box = []

        def prepare():
            check_capacity_wave(waves, capacity)
            arena = self.prepare(self._n_utt(sample_offsets), capacity, waves)       # the graph's own
            arena.write(sample_offsets, rates, jitter)
            box.append(arena)
            out = self._outputs(arena.B, waves.device)

            def queue():
                self.enqueue(waves, arena, *out, jitter is not None, torch.cuda.current_stream(waves.device))
                return out
            return queue, [arena]
        g = _capture(waves, prepare)
        arena = box[0]
        g.sample_offsets, g.rates, g.status = arena.sample_offsets, arena.rates, arena.status
        g.jitter = arena.jitter if jitter is not None else None
        return g


_DEFAULT_MIXED = None


def get_batch_full(feat, augment=False, rng=None, use_pitch=False, use_timefeat=False):
    """RNNModel.get_batch_full (model.py:114-135) with the reference's signature: ``feat`` is the list of (sig, rate) pairs
    reader.mini_batch_iterator yields (``sig`` any 1-D numeric array, the strided ``sig[:, 0]`` of reader.py:80 included;
    the rates may differ from clip to clip).  -> (inp [200, B, 39 (+2) (+2)] torch tensor on the library's device, len0
    NumPy [B]) in batch order, as model.py:135.  ``augment=True`` (model.py:144) draws the endpoint jitter from ``rng``, a
    ``random.Random`` -- by default the module-level generator the reference uses -- in the reference's order."""
    global _DEFAULT_MIXED
    import random
    if _DEFAULT_MIXED is None:
        _DEFAULT_MIXED = MixedRateFeatureBatch()
    sigs = [np.asarray(sig) for sig, _ in feat]
    rates = [rate for _, rate in feat]
    jitter = MixedRateFeatureBatch.draw_jitter(rates, rng if rng is not None else random) if augment else None
    inp, len0, _ = _DEFAULT_MIXED.run(sigs, None, rates, jitter=jitter, use_pitch=use_pitch, use_timefeat=use_timefeat)
    return inp, len0
