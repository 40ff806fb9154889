"""Device tensors as callers really pass them: strided views (one channel of an interleaved [N, 2] buffer, a column
slice of a wider feature tensor, a transposed batch), inputs produced on a side stream, and buffers the library has to
keep alive itself.  Every other GPU module feeds the Python layer a fresh, contiguous, default-stream tensor that the test
holds; the ``.contiguous()`` and ``stream=`` branches of features/batch.py, pipeline.py, model_glue.py, classifier.py and
ensemble.py are reached only from here.

The rule of every test: the result on the view equals the result of the same call on ``view.contiguous()`` -- bit for
bit where the entry point is deterministic (the suite asserts that between two calls elsewhere), within a stated bar
where the unit-variance shift of c0 comes from fp64 atomics whose order is free -- and one case per entry point is held
to the fp64 oracle at the project's 1e-4 normwise bar (``strided_input_vs_oracle``).

``stereo`` puts the clips into column 0 of an [n, 2] buffer and a decoy into column 1 (the same samples reversed and
negated): a read at the wrong stride gives other numbers, and the decoy must be untouched afterwards.

Bars that are not bit equality:
  * 5e-5 normwise between a strided and a contiguous call of ModelFeatureBatch.run, the bar
    test_model_feature_batch_reads_the_clips_in_place applies between two routes to the same [200, B, 39];
  * 1e-6 normwise between two calls of the SAME route of ModelFeatureBatch (graph replay / eager, side stream / default
    stream, thread / alone): the only difference is the last bit of the fp64 variance sums, which moves -ln(var) of c0 by
    at most one fp32 ulp (1e-6 at |ln var| < 16), a constant per utterance that the mean removal and the z-score take out
    again up to the rounding of values no larger than a few hundred (ulp 3e-5) divided by spreads of order ten and by the
    tensor's maximum of order ten: a few 1e-7."""
import functools
import random
import threading

import numpy as np
import pytest

from conftest import normwise, record
from oracle import dsp_oracle

pytestmark = pytest.mark.gpu

CFG = dict(samplerate=16000, winlen=0.025, winstep=0.01, numcep=13, nfilt=40, nfft=512, lowfreq=0,
           highfreq=None, preemph=0.97, ceplifter=22, appendEnergy=True)
PIPE_KW = {k: v for k, v in CFG.items() if k != 'samplerate'}
TOL = 1e-4               # the project's normwise bar against the oracle
ROUTE_TOL = 5e-5         # strided call vs contiguous call of ModelFeatureBatch.run (see the module docstring)
SAME_ROUTE_TOL = 1e-6    # two calls of one route of ModelFeatureBatch.run
MFCC_LENS = (4000, 9001, 20000, 6503)      # ragged: odd lengths, a clip shorter than the others' groups
DENSE_B, DENSE_N = 3, 8000
SLEEP = int(2e8)         # ~0.1 s of device time (the idiom of test_pipeline_launch_does_not_wait_for_the_device)


def _dev():
    import torch
    return torch.device('cuda', 0)


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


def stereo(clips, tdtype):
    """-> (view, ref): ``view`` = column 0 of an [n, 2] device buffer (stride 2, not contiguous) holding the concatenated
    clips beside the decoy column; ``ref`` = view.contiguous().  The buffer itself is ``view._base``."""
    import torch
    flat = np.concatenate([np.asarray(c) for c in clips]).astype(tdtype)
    buf = torch.from_numpy(np.ascontiguousarray(np.stack([flat, -flat[::-1]], axis=1))).to(_dev())
    view = buf[:, 0]
    assert not view.is_contiguous() and view._base is buf
    return view, view.contiguous()


def dense_of(view, B, N):
    """The [B, N] strided form of a stereo view of B clips of N samples."""
    return view._base.view(B, N, 2)[:, :, 0]


def decoy_untouched(view, ref):
    import torch
    torch.cuda.synchronize()
    buf = view._base
    assert torch.equal(buf[:, 0], ref), 'the input column was written'
    assert torch.equal(buf[:, 1], -ref.flip(0)), 'the decoy column was written'


@functools.lru_cache(maxsize=None)
def mfcc_clips():
    from golden_cases import make_signal
    return tuple(make_signal(('vad', 700 + i, n)) for i, n in enumerate(MFCC_LENS))


@functools.lru_cache(maxsize=None)
def dense_clips():
    from golden_cases import make_signal
    return tuple(make_signal(('vad', 710 + i, DENSE_N)) for i in range(DENSE_B))


@functools.lru_cache(maxsize=None)
def mfcc_oracle(delta_n):
    """Per clip of mfcc_clips(): the fp64 rows (int16 and float32 inputs hold the same values).  Computed once, never modified."""
    return tuple(dsp_oracle.mfcc_delta(c.astype(np.float64), delta_n=delta_n, winfunc=np.hamming, **CFG) for c in mfcc_clips())


@functools.lru_cache(maxsize=None)
def feature_plan():
    from features.batch import FeaturePlan
    return FeaturePlan(winfunc=np.hamming, **CFG)


# ---- 1: strided equals contiguous, entry point by entry point ----
@pytest.mark.parametrize('delta_n', [0, 2])
@pytest.mark.parametrize('tdtype', ['int16', 'float32'])
def test_mfcc_batch_on_strided_views(tdtype, delta_n):
    import torch
    plan = feature_plan()
    clips, so = mfcc_clips(), _offsets(mfcc_clips())
    view, ref = stereo(clips, tdtype)
    got, fo = plan.mfcc_batch(view, sample_offsets=so, delta_n=delta_n)
    want, fo_w = plan.mfcc_batch(ref, sample_offsets=so, delta_n=delta_n)
    assert got.shape == (fo[-1], 39 if delta_n else 13) and np.array_equal(fo, fo_w)
    assert torch.equal(got, want)
    decoy_untouched(view, ref)
    dview, dref = stereo(dense_clips(), tdtype)
    got_d, fo_d = plan.mfcc_batch(dense_of(dview, DENSE_B, DENSE_N), delta_n=delta_n)
    want_d, _ = plan.mfcc_batch(dref.view(DENSE_B, DENSE_N), delta_n=delta_n)
    assert got_d.shape[0] == fo_d[-1] and torch.equal(got_d, want_d)
    decoy_untouched(dview, dref)
    if tdtype == 'int16' and delta_n == 2:
        rows = got.cpu().numpy()
        for b, r in enumerate(mfcc_oracle(2)):
            err = record('strided_input_vs_oracle', normwise(rows[fo[b]:fo[b + 1]], r))
            print('mfcc_batch, strided int16, clip', b, 'normwise vs oracle', err)
            assert err <= TOL, (b, err)


@pytest.mark.parametrize('robust', [False, True], ids=['basic', 'robust'])
@pytest.mark.parametrize('tdtype', ['int16', 'float32'])
def test_detect_batch_on_strided_views(tdtype, robust):
    from features.batch import EndpointPlan
    ep = EndpointPlan(16000, 0.03, 0.01, robust=robust)
    clips, so = mfcc_clips(), _offsets(mfcc_clips())
    view, ref = stereo(clips, tdtype)
    got = ep.detect_batch(view, sample_offsets=so, return_feature=True)
    want = ep.detect_batch(ref, sample_offsets=so, return_feature=True)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    decoy_untouched(view, ref)
    dview, dref = stereo(dense_clips(), tdtype)
    got_d = ep.detect_batch(dense_of(dview, DENSE_B, DENSE_N), return_feature=True)
    want_d = ep.detect_batch(dref.view(DENSE_B, DENSE_N), return_feature=True)
    for g, w in zip(got_d, want_d):
        assert np.array_equal(g, w)
    decoy_untouched(dview, dref)
    if tdtype == 'int16' and not robust:
        ends, amp, zcr, fo = got
        for b, c in enumerate(clips):
            assert tuple(ends[b]) == dsp_oracle.basic_endpoint_detection(c, 16000)
            frames = dsp_oracle.to_frames(c.astype(np.float64), 16000, t=0.03, step=0.01)
            assert fo[b + 1] - fo[b] == frames.shape[0]
            assert list(zcr[fo[b]:fo[b + 1]]) == list(dsp_oracle.get_zcr(frames))
            err = record('strided_input_vs_oracle', normwise(amp[fo[b]:fo[b + 1]], dsp_oracle.get_amplitude(frames)))
            print('detect_batch, strided int16, clip', b, 'amplitude normwise vs oracle', err)
            assert err <= TOL, (b, err)


@pytest.mark.parametrize('tdtype', ['int16', 'float32'])
def test_vad_mfcc_pipeline_on_strided_views(tdtype):
    """download=True, and download=False with a prepared layout whose result is read back only after further torch
    allocations of the input copy's size class have been made and filled on the same stream.  The second half is a
    guard: the kernels that read the copy are queued on that stream in front of the fills, so the allocator's
    stream-ordered reuse already protects them; the result now also holds the copy (``d_out.wave``), which is asserted."""
    import torch
    from features.pipeline import VadMfccPipeline
    clips, so = mfcc_clips(), _offsets(mfcc_clips())
    B = len(clips)
    pipe = VadMfccPipeline(rate=16000, unit_variance=True, winfunc=np.hamming, **PIPE_KW)
    view, ref = stereo(clips, tdtype)
    out, fo, ends = pipe.run(view, so, delta_n=2)
    out_c, fo_c, ends_c = pipe.run(ref, so, delta_n=2)
    assert np.array_equal(fo, fo_c) and np.array_equal(ends, ends_c) and np.array_equal(out, out_c)
    lay, lay_c = pipe.prepare(so, delta_n=2), pipe.prepare(so, delta_n=2)
    (d_out, lay_r), none_a, none_b = pipe.run(view, layout=lay, download=False)
    assert lay_r is lay and none_a is None and none_b is None
    assert d_out.wave.owner.is_contiguous() and d_out.wave.ptr == d_out.wave.owner.data_ptr() and d_out.wave.owner is not view
    junk = [torch.full((view.numel(),), 12345, dtype=view.dtype, device=view.device) for _ in range(4)]
    fo_d = lay.d_frame_off.download((B + 1,), np.int64)
    assert np.array_equal(fo_d, fo) and np.array_equal(lay.d_seg.download((B, 2), np.int64), ends)
    assert np.array_equal(d_out.download((int(fo_d[-1]), 39), np.float32), out)
    (d_ref, _), _, _ = pipe.run(ref, layout=lay_c, download=False)
    assert np.array_equal(d_ref.download((int(fo_d[-1]), 39), np.float32), out)
    assert all(int(j[0]) == 12345 and int(j[-1]) == 12345 for j in junk)
    decoy_untouched(view, ref)
    if tdtype == 'int16':
        for b, c in enumerate(clips):
            lo, hi = dsp_oracle.basic_endpoint_detection(c, 16000)
            assert (lo, min(hi, len(c))) == tuple(ends[b])
            want = dsp_oracle.mfcc_delta(dsp_oracle.model_endpoint_scale(c, lo, hi).reshape(-1), delta_n=2, winfunc=np.hamming, **CFG)
            err = record('strided_input_vs_oracle', normwise(out[fo[b]:fo[b + 1]], want))
            print('VadMfccPipeline.run, strided int16, clip', b, 'normwise vs oracle', err)
            assert err <= TOL, (b, err)


# ---- 2: ModelFeatureBatch.run on a strided view, with the optional streams ----
@functools.lru_cache(maxsize=None)
def model_clips(rate, seed0=120):
    """The clips of test_model_feature_batch_optional_streams (known to meet its >= 98 % pitch-frame condition)."""
    from golden_cases import make_signal
    return tuple(make_signal(('vad', seed0 + i, int((20000 + 3000 * i) * rate / 16000), rate, 0.6)) for i in range(3))


@functools.lru_cache(maxsize=None)
def model_oracle(rate):
    """Per clip: the optional streams of the oracle on its own trimmed, scaled clip.  Computed once, never modified."""
    out = []
    for c in model_clips(rate):
        lo, hi = dsp_oracle.basic_endpoint_detection(c, rate)
        sound = dsp_oracle.model_endpoint_scale(c, lo, hi)
        out.append(dict(amp=dsp_oracle.model_feature_extract_timespace(sound, rate),
                        pitch=dsp_oracle.model_feature_extract_pitch(sound, rate)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def model_default(rate, tdtype):
    """(inp [200, B, 39], len0, endpoints) of the default call on the contiguous clips, as host arrays."""
    import torch
    from features.model_glue import ModelFeatureBatch
    clips = model_clips(rate)
    flat = torch.from_numpy(np.concatenate(clips).astype(tdtype)).to(_dev())
    inp, len0, ends = ModelFeatureBatch(rate=rate).run(flat, _offsets(clips))
    return inp.cpu().numpy(), np.asarray(len0), np.asarray(ends)


def block_state(ptr):
    """The state torch's caching allocator gives the block that contains ``ptr``."""
    import torch
    for seg in torch.cuda.memory_snapshot():
        a = seg['address']
        if not a <= ptr < a + seg['total_size']:
            continue
        for blk in seg['blocks']:
            if a <= ptr < a + blk['size']:
                return blk['state']
            a += blk['size']
    return 'not in a block of the caching allocator'


def optional_stream_problems(got, rate, use_pitch, use_timefeat):
    """The checks of test_model_feature_batch_optional_streams on columns 39.. of ``got`` [200, B, 39 + 2 (+ 2)]."""
    problems = []
    col_p, col_a = 39, 39 + (2 if use_pitch else 0)
    for b, ref in enumerate(model_oracle(rate)):
        if use_timefeat:
            a0, a1 = ref['amp']
            n0, n1 = min(len(a0), 200), min(len(a1), 200)
            e0 = record('model_batch_timefeat', normwise(got[:n0, b, col_a], a0[:n0, 0]))
            e1 = normwise(got[:n1, b, col_a + 1], a1[:n1, 0])
            print('clip', b, 'amplitude stream normwise vs oracle', e0, e1)
            if e0 > TOL or e1 > TOL:
                problems.append(f'clip {b}: amplitude columns off by {e0:.3g} / {e1:.3g} (bar {TOL})')
            if got[n0:, b, col_a].any() or got[n1:, b, col_a + 1].any():
                problems.append(f'clip {b}: amplitude columns are not zero behind their frame counts')
        if use_pitch:
            p0, p1 = ref['pitch']
            m0, m1 = min(len(p0), 200), min(len(p1), 200)
            same = float(np.isclose(got[:m0, b, col_p], p0[:m0, 0], rtol=1e-5, atol=1e-6).mean())
            print('clip', b, 'pitch frames equal to the oracle', same)
            if same < 0.98:
                problems.append(f'clip {b}: only {same:.3f} of the pitch frames equal the oracle (>= 0.98)')
            if got[m0:, b, col_p].any() or got[m1:, b, col_p + 1].any():
                problems.append(f'clip {b}: pitch columns are not zero behind their frame counts')
            if not np.allclose(got[:m1, b, col_p + 1], got[1:m1 + 1, b, col_p] - got[:m1, b, col_p], rtol=0, atol=2e-6):
                problems.append(f'clip {b}: the difference column is not the difference of the pitch column')
    return problems


@pytest.mark.parametrize('streams', ['timefeat', 'pitch', 'both'])
@pytest.mark.parametrize('tdtype', ['int16', 'float32'])
@pytest.mark.parametrize('rate', [16000, 44100])
def test_model_feature_batch_on_a_strided_view_with_optional_streams(monkeypatch, rate, tdtype, streams):
    """The optional streams trim the wave buffer a second time, after ModelFeatureBatch.run has allocated its outputs: the
    contiguous copy made of a strided view has to live until then.  Two checks, so that nothing hangs on what the
    allocator happens to do: (a) at the moment dsp_trim_scale_batch is called, the block holding its wave pointer is
    ``active_allocated`` in torch's allocator; (b) the values.  The copy (3 clips, >= 69 000 samples: 138 KB as int16) is
    larger than inp (200 x 3 x 39 x 4 B = 94 KB), so a freed copy is what ``torch.empty`` most likely hands out for inp."""
    import torch
    from features import _native as nat
    from features.model_glue import ModelFeatureBatch
    use_pitch, use_timefeat = streams in ('pitch', 'both'), streams in ('timefeat', 'both')
    clips, so = model_clips(rate), _offsets(model_clips(rate))
    want_inp, want_len, want_ends = model_default(rate, tdtype)
    model_oracle(rate)
    view, ref = stereo(clips, tdtype)
    mfb = ModelFeatureBatch(rate=rate)
    lib = nat.load()
    forward, states = lib.dsp_trim_scale_batch, []

    def checked_trim(d_wave, *rest):
        states.append(block_state(int(d_wave)))
        return forward(d_wave, *rest)

    torch.cuda.synchronize()
    torch.cuda.empty_cache()                     # (before the call under test only: nothing stale exists yet)
    monkeypatch.setattr(lib, 'dsp_trim_scale_batch', checked_trim)
    inp, len0, ends = mfb.run(view, so, use_pitch=use_pitch, use_timefeat=use_timefeat)
    monkeypatch.undo()
    got = inp.cpu().numpy()
    assert got.shape == (200, 3, 39 + 2 * use_pitch + 2 * use_timefeat)
    problems = []
    if states != ['active_allocated']:
        problems.append(f'(a) the wave buffer of the second trim was {states} in the allocator, not one live block')
    if not (np.array_equal(len0, want_len) and np.array_equal(ends, want_ends)):
        problems.append('(b) len0 / endpoints differ from the contiguous call')
    err = normwise(got[:, :, :39], want_inp)
    print('columns :39, strided vs contiguous call, normwise', err)
    if err > ROUTE_TOL:
        problems.append(f'(b) columns :39 differ from the contiguous call by {err:.3g} (bar {ROUTE_TOL})')
    problems += ['(b) ' + p for p in optional_stream_problems(got, rate, use_pitch, use_timefeat)]
    assert not problems, '\n'.join(problems)
    decoy_untouched(view, ref)


# ---- 3: capture refuses what it cannot serve ----
def test_capture_refuses_a_strided_view_and_serves_an_offset_one():
    import torch
    from features.model_glue import ModelFeatureBatch
    rate = 16000
    clips_a, clips_b = model_clips(rate), model_clips(rate, 220)
    so = _offsets(clips_a)
    n = int(so[-1])
    mfb = ModelFeatureBatch(rate=rate)
    lay = mfb.pipe.prepare(so, delta_n=0)
    view, ref = stereo(clips_a, 'int16')
    with pytest.raises(ValueError, match='contiguous'):
        mfb.capture(view, lay)
    decoy_untouched(view, ref)
    big = torch.zeros(n + 64, dtype=torch.int16, device=_dev())
    window = big[32:32 + n]                       # contiguous, storage offset 32 samples
    assert window.is_contiguous() and window.storage_offset() == 32
    window.copy_(ref)
    g = mfb.capture(window, lay)
    for clips in (clips_a, clips_b):
        flat = torch.from_numpy(np.concatenate(clips)).to(_dev())
        window.copy_(flat)
        inp, len0 = g.replay()
        torch.cuda.synchronize()
        eager, elen, _ = ModelFeatureBatch(rate=rate).run(flat, so)
        assert np.array_equal(len0.cpu().numpy(), elen)
        err = normwise(inp.cpu().numpy(), eager.cpu().numpy())
        assert err <= SAME_ROUTE_TOL, err
    assert not big[:32].any() and not big[32 + n:].any()


# ---- 4: an explicit stream orders the copy ----
def _fresh_clips(seed0):
    from golden_cases import make_signal
    ragged = tuple(make_signal(('vad', seed0 + i, n)) for i, n in enumerate(MFCC_LENS))
    dense = tuple(make_signal(('vad', seed0 + 10 + i, DENSE_N)) for i in range(DENSE_B))
    return ragged, dense


def test_explicit_stream_orders_the_copy_of_a_strided_view():
    """mfcc_batch(view, stream=side) while the current stream is busy: the contiguous copy is made on ``side`` too, so the
    kernel reads it complete, and neither call waits for the current stream: each returns while the sleep queued in front
    of it is still running.  That is asked of the host calls, in front of side.synchronize(): whether the device runs the
    side stream beside the sleep depends on which hardware queue the runtime gives it, and two streams may share one.
    Only contiguous tensors warm the kernels up, so no earlier copy of the same samples lies in the allocator's free lists."""
    import torch
    plan = feature_plan()
    dev = _dev()
    ragged, dense = _fresh_clips(730)
    so = _offsets(ragged)
    view, ref = stereo(ragged, 'int16')
    dview, dref = stereo(dense, 'int16')
    lay = plan.layout(ref, so)                    # prepared: building one uploads its offsets and synchronises
    lay_d = plan.layout(dref.view(DENSE_B, DENSE_N))
    want, _ = plan.mfcc_batch(ref, delta_n=2, layout=lay)
    want_d, _ = plan.mfcc_batch(dref.view(DENSE_B, DENSE_N), delta_n=2, layout=lay_d)
    side = torch.cuda.Stream(dev)
    busy = torch.cuda.Event()
    torch.cuda.synchronize()
    torch.cuda._sleep(SLEEP)                      # the current stream is busy for ~0.1 s
    busy.record(torch.cuda.current_stream(dev))
    got, _ = plan.mfcc_batch(view, delta_n=2, stream=side, layout=lay)
    waited = [busy.query()]                       # the call has returned: is the sleep in front of it still running?
    got_d, _ = plan.mfcc_batch(dense_of(dview, DENSE_B, DENSE_N), delta_n=2, stream=side.cuda_stream, layout=lay_d)   # a raw handle
    waited.append(busy.query())
    side.synchronize()
    same, same_d = torch.equal(got, want), torch.equal(got_d, want_d)
    assert same and same_d, 'the kernel on the side stream read a copy that was not ordered in front of it'
    assert waited == [False, False], f'the sleep on the current stream had ended when the ragged / dense call returned: {waited}'
    decoy_untouched(view, ref)
    decoy_untouched(dview, dref)


def test_explicit_stream_sees_what_its_producer_wrote():
    """The producer of the strided buffer runs on the side stream, behind a sleep: with stream=side the copy and the
    kernel queue behind it."""
    import torch
    plan = feature_plan()
    dev = _dev()
    ragged_old, _ = _fresh_clips(750)
    ragged_new, _ = _fresh_clips(770)
    so = _offsets(ragged_new)
    view, _ = stereo(ragged_old, 'int16')
    new_view, new_ref = stereo(ragged_new, 'int16')
    lay = plan.layout(new_ref, so)
    want, _ = plan.mfcc_batch(new_ref, delta_n=2, layout=lay)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP)
        view._base.copy_(new_view._base)
    got, _ = plan.mfcc_batch(view, delta_n=2, stream=side, layout=lay)
    side.synchronize()
    assert torch.equal(got, want)
    decoy_untouched(view, new_ref)


# ---- 5: the pipelines under torch.cuda.stream(side) ----
@pytest.mark.parametrize('layout', ['offset_contiguous', 'strided'])
def test_pipelines_on_a_side_stream(layout):
    """ModelFeatureBatch.run and VadMfccPipeline.run under ``with torch.cuda.stream(side)``, the input written on ``side``
    behind a sleep, jitter given: the default-stream results."""
    import torch
    from features.model_glue import ModelFeatureBatch
    from features.pipeline import VadMfccPipeline
    dev, rate = _dev(), 16000
    clips, so = model_clips(rate), _offsets(model_clips(rate))
    n = int(so[-1])
    mfb = ModelFeatureBatch(rate=rate)
    pipe = VadMfccPipeline(rate=rate, unit_variance=True, winfunc=np.hamming, **PIPE_KW)
    jit = mfb.draw_jitter(len(clips), random.Random(5))
    src_view, ref = stereo(clips, 'int16')
    want_m = mfb.run(ref, so, jitter=jit, use_timefeat=True)
    want_p = pipe.run(ref, so, delta_n=2, jitter=jit)
    if layout == 'strided':
        dst, source = torch.zeros_like(src_view._base), src_view._base
        arg = dst[:, 0]
    else:
        big = torch.zeros(n + 64, dtype=torch.int16, device=dev)
        dst = arg = big[32:32 + n]                 # contiguous, storage offset 32 samples
        source = ref
    assert arg.is_contiguous() == (layout != 'strided')
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP)
        dst.copy_(source)                          # produced on the side stream, behind the sleep
        got_m = mfb.run(arg, so, jitter=jit, use_timefeat=True)
        dst.zero_()
        torch.cuda._sleep(SLEEP)
        dst.copy_(source)
        got_p = pipe.run(arg, so, delta_n=2, jitter=jit)
    side.synchronize()
    assert np.array_equal(got_m[1], want_m[1]) and np.array_equal(got_m[2], want_m[2])
    a, b = got_m[0].cpu().numpy(), want_m[0].cpu().numpy()
    assert a.shape == b.shape == (200, len(clips), 41)
    assert normwise(a[:, :, :39], b[:, :, :39]) <= SAME_ROUTE_TOL and normwise(a[:, :, 39:], b[:, :, 39:]) <= SAME_ROUTE_TOL
    for g, w in zip(got_p, want_p):
        assert np.array_equal(g, w)
    if layout == 'strided':
        torch.cuda.synchronize()
        assert torch.equal(dst[:, 1], src_view._base[:, 1])


# ---- 6: two threads, one ModelFeatureBatch ----
def test_two_threads_share_one_model_feature_batch():
    """Each thread runs its own device batch (same sample offsets, other content: a crossed pointer stays inside a buffer)
    through ONE ModelFeatureBatch with use_timefeat=True and gets its own single-threaded result.  A guard, not a proof:
    what removes the shared state is that the wave buffer travels with the result of VadMfccPipeline.run."""
    import torch
    from features.model_glue import ModelFeatureBatch
    rate = 16000
    batches = [model_clips(rate), model_clips(rate, 220)]
    so = _offsets(batches[0])
    assert np.array_equal(so, _offsets(batches[1]))
    flats = [torch.from_numpy(np.concatenate(c)).to(_dev()) for c in batches]
    mfb = ModelFeatureBatch(rate=rate)
    alone = []
    for f in flats:
        inp, len0, ends = mfb.run(f, so, use_timefeat=True)
        alone.append((inp.cpu().numpy(), len0, ends))
    assert normwise(alone[0][0][:, :, 39:], alone[1][0][:, :, 39:]) > 1e-2       # the batches do differ
    errs = []

    def work(i):
        try:
            for k in range(20):
                inp, len0, ends = mfb.run(flats[i], so, use_timefeat=True)
                got = inp.cpu().numpy()
                e = normwise(got[:, :, 39:], alone[i][0][:, :, 39:])
                if e > 1e-6 or not np.array_equal(len0, alone[i][1]) or not np.array_equal(ends, alone[i][2]):
                    errs.append((i, k, e))
                    return
                e39 = normwise(got[:, :, :39], alone[i][0][:, :, :39])
                if e39 > SAME_ROUTE_TOL:
                    errs.append((i, k, 'columns :39', e39))
                    return
        except Exception as e:      # noqa: BLE001 - reported to the main thread
            errs.append((i, repr(e)))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


# ---- 7: recurrent entry points on views ----
RNN_B, RNN_T = 5, 6
RNN_LENS = (1, 6, 3, 6, 2)         # ragged, with 1 and T


def _views(I, pad):
    """x [T, B, I] as a column slice of a [T, B, I + pad] tensor and as the transpose of a [B, T, I] one (same values)."""
    import torch
    g = torch.Generator(device='cpu').manual_seed(17)
    x = torch.randn(RNN_T, RNN_B, I, generator=g)
    wide = torch.cat([x, torch.full((RNN_T, RNN_B, pad), 1e3)], dim=2).to(_dev())
    bt = x.transpose(0, 1).contiguous().to(_dev())
    views = {'column_slice': wide[:, :, :I], 'transposed': bt.transpose(0, 1)}
    for v in views.values():
        assert not v.is_contiguous() and torch.equal(v, x.to(_dev()))
    return views


def _grads(run, outputs_of, module, x, loss_kind, weights):
    """Gradients of x and every parameter for one loss; ``x`` keeps its layout (a view stays a view)."""
    import torch
    x = x.detach().requires_grad_(True) if x.is_contiguous() else x
    res = outputs_of(run(x))
    if loss_kind == 'weighted_transpose':          # the upstream gradient of the sequence output arrives non-contiguous
        loss = (res[0].transpose(0, 1) * weights).sum()
    else:                                          # expanded, stride-0 gradients for every output
        loss = sum(o.sum() for o in res)
    params = [p for p in module.parameters()]
    return torch.autograd.grad(loss, [x] + params, allow_unused=True)


def _check_recurrent(module, run, outputs_of, seq_of, I, pad):
    import torch
    views = _views(I, pad)
    for name, view in views.items():
        dense = view.contiguous()
        module.eval()
        with torch.no_grad():
            got, want = outputs_of(run(view)), outputs_of(run(dense))
        for k, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), (name, 'forward', k)
        module.train()
        for loss_kind in ('weighted_transpose', 'sums'):
            seq = seq_of(want)
            weights = torch.randn(seq.transpose(0, 1).shape, generator=torch.Generator(device='cpu').manual_seed(3)).to(_dev())
            base = view._base.detach().requires_grad_(True)          # the view of a leaf: autograd sees the strides
            leaf_view = base[:, :, :I] if name == 'column_slice' else base.transpose(0, 1)
            assert leaf_view.stride() == view.stride()
            g_view = _grads(run, outputs_of, module, leaf_view, loss_kind, weights)
            g_dense = _grads(run, outputs_of, module, dense, loss_kind, weights)
            assert len(g_view) == len(g_dense) >= 2
            for k, (g, w) in enumerate(zip(g_view, g_dense)):
                assert (g is None) == (w is None), (name, loss_kind, k)
                if g is not None:
                    assert g.shape == w.shape and torch.equal(g, w), (name, loss_kind, k)
            assert g_view[0] is not None and g_view[0].abs().max().item() > 0


def test_bigru_encoder_on_views():
    """_DynEnc.run(native=True), 39 -> 20 x 2, B 5, T 6: x = wide[:, :, :39] of a 43-wide tensor and x = bt.transpose(0, 1)."""
    import torch
    from features.classifier import _DynEnc, fill_parameters
    torch.manual_seed(0)
    enc = _DynEnc(39, 20, 2)
    fill_parameters(enc, 41)
    enc = enc.to(_dev())
    lens = np.array(RNN_LENS)
    _check_recurrent(enc, lambda x: enc.run(x, lens, native=True), lambda r: tuple(r), lambda outs: outs[0], 39, 4)


def test_hmlstm_on_views():
    """HMLSTM.run(native=True) at the smallest shape of the HM-LSTM fixtures (24 -> 20, 28), the same two views."""
    import torch
    from features.classifier import HMLSTM, fill_parameters
    torch.manual_seed(0)
    m = HMLSTM(1.0, 24, [20, 28])
    fill_parameters(m, 43)
    m = m.to(_dev())
    lens = np.array(RNN_LENS)

    def outputs_of(r):
        outs = (r.h_2, r.h_1, r.last_h2)              # h_2 [B, T, H2] first: weighted as [T, B, H2], its gradient arrives transposed
        if not torch.is_grad_enabled():
            outs += (r.z_1, r.z_2, r.z_hat) + tuple(r.hidden)
        return outs

    _check_recurrent(m, lambda x: m.run(x, None, lens=lens, native=True), outputs_of, lambda outs: outs[0], 24, 4)


# ---- 8: the ensemble on views ----
def test_ensemble_entry_points_on_views():
    import torch
    from ensemble_cases import design_logits, make_clips
    from features.ensemble import EnsembleBatch, PitchSVM, ensemble_decide
    from test_gpu_ensemble import random_model
    dev = _dev()
    pairs, thresholds = ((0, 1), (6, 7)), (0.8, 0.7)
    models = [random_model(60 + r, (37, 129)[r], 5, classes=pairs[r]) for r in range(2)]
    svms = [PitchSVM.from_arrays(m['support_vectors'], m['dual_coef'], m['intercept'], m['gamma'], m['classes'],
                                 scale=m['scale'], center=m['center']) for m in models]
    rules = list(zip(pairs, thresholds, svms))
    rng = np.random.default_rng(9)
    n = 37
    X = torch.from_numpy(rng.standard_normal((5, n))).to(dev)                    # stored [F, n]
    assert X.t().stride(1) != 1
    for svm in svms:
        got, want = svm.decision_function(X.t()), svm.decision_function(X.t().contiguous())
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        assert torch.equal(svm.predict(X.t()), svm.predict(X.t().contiguous()))
    # the gate: logits stored [C, B], features stored [F, B]
    B = 14
    logits_cb = torch.from_numpy(np.ascontiguousarray(design_logits().T)).to(dev)
    feat_fb = torch.from_numpy(rng.standard_normal((5, B))).to(dev)
    got = ensemble_decide(logits_cb.t(), rules, feat_fb.t())
    want = ensemble_decide(logits_cb.t().contiguous(), rules, feat_fb.t().contiguous())
    assert (want[2].cpu().numpy() > 0).any()                                   # some rule did fire
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), k
    side = torch.cuda.Stream(dev)                                              # ... and with the copies made on an explicit stream
    side.wait_stream(torch.cuda.current_stream(dev))
    on_side = ensemble_decide(logits_cb.t(), rules, feat_fb.t(), stream=side)
    side.synchronize()
    for k, (g, w) in enumerate(zip(on_side, want)):
        assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), ('side', k)
    # the whole path on one channel of a stereo buffer, a stub head
    clips, rate = make_clips()
    clips = clips[:4]
    so = _offsets(clips)
    fixed = torch.from_numpy(design_logits()[:4].copy()).to(dev)
    eb = EnsembleBatch(rate, lambda inp, len0: (fixed, None), rules)
    view, ref = stereo(clips, 'int16')
    a, b = eb.run(view, so), eb.run(ref, so)
    for name in ('pred', 'prob', 'used', 'decision', 'logits', 'feat', 'valid', 'len0'):
        ga, gb = getattr(a, name), getattr(b, name)
        ga, gb = (v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v) for v in (ga, gb))
        assert ga.tobytes() == gb.tobytes(), name
    assert np.array_equal(a.endpoints, b.endpoints) and a.valid.cpu().numpy().all()
    assert normwise(a.inp.cpu().numpy(), b.inp.cpu().numpy()) <= SAME_ROUTE_TOL
    decoy_untouched(view, ref)
