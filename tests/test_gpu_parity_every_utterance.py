"""MFCC parity on EVERY utterance, and on frames whose narrow mel filters are cancelled on purpose.

The front end's contract is the reference's MFCC | delta | delta-delta rows within 1e-4 normwise per utterance.  The
other parity tests sample utterances of large batches; an fp32 spectrum loses a frame whose one-bin filter is nearly
cancelled by pre-emphasis and window (about one frame in 1e5 of a noise batch, tests/cancel_cases.py), and a sample does
not meet it.  Here (1) such frames are built, 13-frame clips, and sent through every route -- dense with the MFCC and
the delta kernel, dense through the fused kernel, ragged and misaligned, the generic kernel, cepstra only, single calls
-- and (2) all 1 024 utterances of the headline batches are compared with the oracle.  The kernels pass because they
recompute a filter that falls below 7e-10 of its frame's energy in fp64 (csrc/kernels_repair.h).

Which kernel a plan reaches: 40 and 26 filters run the NFFT = 512 kernel's standard instantiations, 44 filters its
catch-all instantiation (six filter iterations); the 64-filter cases run the GENERIC kernel on every route (the
NFFT = 512 kernel takes at most 48 filters), so they test that kernel only.  The VadMfccPipeline route reads the trimmed
clip in place (an offset into the clip and a shorter length per utterance): its engineered frame 0 is the frame whose
first sample the pre-emphasis leaves alone.

Measured values go through conftest.record into the session's file of measured parity.  Only the default (vector-pipe) kernels
run here; the opt-in matrix-pipe kernels are not covered."""
import numpy as np
import pytest

import cancel_cases as cc
from conftest import normwise, record
from oracle import dsp_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-4
CANARY = 1234.5

_PLANS, _REFS = {}, {}


def _plan(case):
    from features.batch import FeaturePlan
    key = (case['plan'], case['winfunc'], case['preemph'])
    if key not in _PLANS:
        kw, wf = cc.plan_kwargs(case)
        _PLANS[key] = FeaturePlan(winfunc=wf, **kw)
    return _PLANS[key]


def _ref(case, delta_n=2):
    """Oracle rows of a case, computed once and shared."""
    key = (case['name'], delta_n)
    if key not in _REFS:
        kw, wf = cc.plan_kwargs(case)
        x = cc.make_input(case).astype(np.float64)
        r = dsp_oracle.mfcc_delta(x, delta_n=delta_n, winfunc=wf, **kw) if delta_n else dsp_oracle.mfcc(x, winfunc=wf, **kw)
        r.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _groups():
    """Cases that can share a plan and a dtype."""
    g = {}
    for c in cc.CASES:
        g.setdefault((c['plan'], c['winfunc'], c['preemph'], c['dtype']), []).append(c)
    return g


GROUPS = _groups()
GROUP_IDS = ['-'.join(str(v) for v in k) for k in GROUPS]


def _run_guarded(plan, waves, so, delta_n):
    """plan.run_raw into a NaN-filled buffer with a canary row behind it -> rows [sum T, D], frame offsets."""
    import torch
    from features import _native as nat
    dev = torch.device('cuda', 0)
    lay = plan.layout(waves, so)
    D = plan.width(delta_n)
    rows = int(lay.total_frames)
    buf = torch.full((rows + 1, D), float('nan'), device=dev)
    buf[rows] = CANARY
    d_wave = torch.from_numpy(np.ascontiguousarray(waves).reshape(-1)).to(dev)
    wd = nat.WAVE_I16 if waves.dtype == np.int16 else nat.WAVE_F32
    plan.run_raw(d_wave.data_ptr(), wd, lay, buf.data_ptr(), delta_n, None)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[rows] == CANARY), 'the row behind the output was written'
    assert np.isfinite(got[:rows]).all()
    return got[:rows], np.asarray(lay.frame_offsets)


def _assert_cases(tag, cases, out, fo, delta_n=2, first=0):
    errs = {}
    for i, c in enumerate(cases):
        ref = _ref(c, delta_n)
        rows = out[fo[first + i]:fo[first + i + 1]]
        assert rows.shape == ref.shape, (c['name'], rows.shape, ref.shape)
        errs[c['name']] = record(f"cancel_{tag}_{c['name']}", normwise(rows, ref))
        print(f"{tag:10s} {c['name']:22s} ratio {c['ratio']:.0e}  normwise {errs[c['name']]:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad


def _ragged(cases, dtype, lead=4001):
    """The cases' clips behind one odd-length ordinary clip, so that nothing is aligned."""
    head = cc.base_clip(77, lead, dtype)
    head = head.astype(np.float32) if np.dtype(dtype) == np.float32 else np.round(head).astype(np.int16)
    clips = [head] + [cc.make_input(c) for c in cases]
    so = np.concatenate([[0], np.cumsum([len(x) for x in clips])]).astype(np.int64)
    return np.concatenate(clips), so


def _dense_sets(cases):
    """Cases of equal length can form a dense batch."""
    by_n = {}
    for c in cases:
        by_n.setdefault(c['n'], []).append(c)
    return by_n


@pytest.mark.parametrize('key', list(GROUPS), ids=GROUP_IDS)
def test_engineered_dense_mfcc_then_delta(key):
    """Dense batches of a few utterances: the MFCC kernel, then the delta kernel."""
    for n, cases in _dense_sets(GROUPS[key]).items():
        waves = np.stack([cc.make_input(c) for c in cases])
        out, fo = _run_guarded(_plan(cases[0]), waves, None, 2)
        _assert_cases('dense', cases, out, fo)


@pytest.mark.parametrize('key', list(GROUPS), ids=GROUP_IDS)
def test_engineered_ragged_misaligned(key):
    cases = GROUPS[key]
    flat, so = _ragged(cases, key[3])
    out, fo = _run_guarded(_plan(cases[0]), flat, so, 2)
    _assert_cases('ragged', cases, out, fo, first=1)


@pytest.mark.parametrize('key', list(GROUPS), ids=GROUP_IDS)
def test_engineered_generic_kernel(key):
    from features import _native as nat
    lib = nat.load()
    cases = GROUPS[key]
    flat, so = _ragged(cases, key[3])
    try:
        nat.check(lib.dsp_debug_force_generic(1))
        out, fo = _run_guarded(_plan(cases[0]), flat, so, 2)
    finally:
        nat.check(lib.dsp_debug_force_generic(0))
    _assert_cases('generic', cases, out, fo, first=1)


@pytest.mark.parametrize('key', list(GROUPS), ids=GROUP_IDS)
def test_engineered_cepstra_only_and_single_calls(key):
    """delta_n = 0, ragged and dense, and features.mfcc clip by clip: all within the bar, and the single call gives the
    bits of the dense batch (as tests/test_gpu_batch.py::test_batch_equals_single_calls asserts on ordinary clips)."""
    import features
    cases = GROUPS[key]
    flat, so = _ragged(cases, key[3])
    out, fo = _run_guarded(_plan(cases[0]), flat, so, 0)
    _assert_cases('cepstra', cases, out, fo, delta_n=0, first=1)
    for n, same in _dense_sets(cases).items():
        dense, fo = _run_guarded(_plan(same[0]), np.stack([cc.make_input(c) for c in same]), None, 0)
        for i, c in enumerate(same):
            kw, wf = cc.plan_kwargs(c)
            single = features.mfcc(cc.make_input(c), winfunc=wf, **kw).astype(np.float32)
            assert record(f"cancel_single_{c['name']}", normwise(single, _ref(c, 0))) <= TOL, c['name']
            assert np.array_equal(single, dense[fo[i]:fo[i + 1]]), c['name']


# ---- the fused MFCC + delta kernel: engineered utterances among ordinary ones -------------------------------------------
FUSED_B, FUSED_N, FUSED_T = 512, 9360, 57          # the smallest batch the fused form takes (tests/test_gpu_fused_delta_runs.py)
FUSED = [  # (utterance, frames, bins, ratio)
    (0, (0,), (1,), 1e-6), (1, (7, 8), (1,), 1e-5), (100, tuple(range(8, 16)), (1,), 1e-5), (255, (30, 31), (2, 3), 1e-6),
    (256, (56,), (1, 2, 3), 1e-6), (300, (55,), (1,), 1e-8), (511, (56,), (1,), 1e-6), (510, (20,), (2,), 1e-6),
]


@pytest.fixture(scope='module')
def fused_batch():
    out = {}
    for dtype in ('float32', 'int16'):
        rng = np.random.default_rng(900)
        g = rng.standard_normal((FUSED_B, FUSED_N))
        waves = (0.25 * g).astype(np.float32) if dtype == 'float32' else np.round(3000 * g).astype(np.int16)
        for b, frames, bins, ratio in FUSED:
            if dtype == 'int16':          # what +-1 moves on integers can reach
                ratio, frames = max(ratio, 1e-5), frames[:2]
            waves[b] = cc.engineer(waves[b].astype(np.float64), cc.L, cc.S, cc.NFFT, 0.97, np.hamming, frames, bins, ratio, dtype)
            # the clip bites: fp32 within 2 % of the asked ratio, int16 (the greedy search may stop early) at or below it
            got = cc.achieved(waves[b], cc.L, cc.S, cc.NFFT, 0.97, np.hamming(cc.L), frames, bins) / ratio
            assert (got.max() <= 1.0) if dtype == 'int16' else np.all(np.abs(got - 1.0) <= 0.02), (dtype, b, got)
        out[dtype] = waves
    return out


@pytest.mark.parametrize('dtype', ['float32', 'int16'])
def test_engineered_fused_kernel(fused_batch, dtype):
    """Through the fused launch: within the bar on every engineered utterance and, as the suite asserts on ordinary
    batches, the same bits as the MFCC kernel followed by the delta kernel."""
    import torch
    from features import _native as nat
    lib = nat.load()
    waves = fused_batch[dtype]
    plan = _plan(cc.BY_NAME['b123_r1e-5'])
    fused, fo = _run_guarded(plan, waves, None, 2)
    assert fo[-1] == FUSED_B * FUSED_T
    dev = torch.device('cuda', 0)
    C, rows = plan.C, FUSED_B * FUSED_T
    d_wave = torch.from_numpy(waves).to(dev)
    wd = nat.WAVE_I16 if waves.dtype == np.int16 else nat.WAVE_F32
    two = torch.full((rows, 3 * C), float('nan'), device=dev)
    nat.check(lib.dsp_features_batch(plan.plan.handle, d_wave.data_ptr(), wd, None, None, FUSED_B, rows, FUSED_N, nat.OUT_MFCC,
                                     two.data_ptr(), 3 * C, None, None))
    nat.check(lib.dsp_delta_batch(two.data_ptr(), 3 * C, None, FUSED_B, rows, FUSED_T, C, 2, two.data_ptr() + C * 4, 3 * C,
                                  two.data_ptr() + 2 * C * 4, 3 * C, None))
    torch.cuda.synchronize()
    assert np.array_equal(fused, two.cpu().numpy())
    bad = {}
    for b, frames, bins, ratio in FUSED:
        ref = dsp_oracle.mfcc_delta(waves[b].astype(np.float64), delta_n=2, winfunc=np.hamming, **cc.PLAN40)
        e = record(f'cancel_fused_{dtype}_utt{b}', normwise(fused[fo[b]:fo[b + 1]], ref))
        print(f'fused {dtype} utterance {b} frames {frames} bins {bins} ratio {ratio:.0e}: normwise {e:.3e}')
        if not e <= TOL:
            bad[b] = e
    assert not bad, bad


def test_engineered_fused_step_in_a_graph(fused_batch):
    """The dense step allocates nothing: captured into a graph, it replays to the bits of the plain launch."""
    import torch
    from features import _native as nat
    waves = fused_batch['float32']
    plan = _plan(cc.BY_NAME['b123_r1e-5'])
    want, _ = _run_guarded(plan, waves, None, 2)
    dev = torch.device('cuda', 0)
    lay = plan.layout(waves, None)
    d_wave = torch.from_numpy(waves).to(dev)
    out = torch.zeros((FUSED_B * FUSED_T, 39), device=dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.run_raw(d_wave.data_ptr(), nat.WAVE_F32, lay, out.data_ptr(), 2, torch.cuda.current_stream(dev))
    for _ in range(2):
        out.fill_(float('nan'))
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert np.array_equal(out.cpu().numpy(), want)


def test_a_nan_clip_next_to_an_engineered_one():
    cases = [cc.BY_NAME['sweep_b1_r1e-06'], cc.BY_NAME['frames7_8_b1'], cc.BY_NAME['b123_r1e-6']]
    plan = _plan(cases[0])
    waves = np.stack([cc.make_input(c) for c in cases])
    clean, fo = _run_guarded(plan, waves, None, 2)
    bad = np.insert(waves, 1, np.full(cc.N13, np.nan, dtype=np.float32), axis=0)
    lay = plan.layout(bad, None)
    got, fo2 = plan.mfcc_batch(bad, delta_n=2)
    T = int(fo[1])
    assert np.array_equal(got[:T], clean[:T]) and np.array_equal(got[2 * T:], clean[T:])
    assert int(lay.total_frames) == 4 * T


# ---- VAD -> trim -> MFCC: the trimmed clip read in place, engineered relative to the oracle's left endpoint ----------------
@pytest.mark.parametrize('copy_trimmed', [False, True], ids=['in_place', 'trimmed_copy'])
@pytest.mark.parametrize('unit_variance', [False, True], ids=['plain', 'unit_variance'])
def test_engineered_vad_pipeline(unit_variance, copy_trimmed):
    """VadMfccPipeline.run on a burst-in-noise clip whose TRIMMED form has frames 0 and 20 cancelled (cc.make_vad_case:
    the endpoints did not move), between two ordinary clips of other lengths."""
    from features.pipeline import VadMfccPipeline
    case = cc.make_vad_case()
    assert case is not None, 'no seed of cancel_cases.VAD_SEEDS keeps the endpoints'
    seed, clip, left, right = case
    clips = [cc.burst_clip(41)[:17001], clip, cc.burst_clip(42)]
    so = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    pipe = VadMfccPipeline(rate=16000, unit_variance=unit_variance, winfunc=np.hamming,
                           **{k: v for k, v in cc.PLAN40.items() if k != 'samplerate'})
    pipe.copy_trimmed = copy_trimmed
    out, fo, ends = pipe.run(np.concatenate(clips), so, delta_n=2)
    assert (int(ends[1, 0]), int(ends[1, 1])) == (left, right)
    for b, c in enumerate(clips):
        lo, hi = dsp_oracle.basic_endpoint_detection(c, 16000)
        assert (lo, min(hi, len(c))) == (int(ends[b, 0]), int(ends[b, 1])), b
        seg = dsp_oracle.model_endpoint_scale(c, lo, hi).reshape(-1) if unit_variance else np.asarray(c[lo:hi], dtype=np.float64)
        ref = dsp_oracle.mfcc_delta(seg, delta_n=2, winfunc=np.hamming, **cc.PLAN40)
        got = out[fo[b]:fo[b + 1]]
        assert got.shape == ref.shape, (b, got.shape, ref.shape)
        err = record(f"cancel_vad_{'uv' if unit_variance else 'plain'}_{'copy' if copy_trimmed else 'inplace'}_{b}", normwise(got, ref))
        print(f'vad pipeline unit_variance {unit_variance} copy {copy_trimmed} clip {b}: normwise {err:.3e}')
        assert err <= TOL, (b, err)


# ---- every utterance of the headline batches ----------------------------------------------------------------------------
def _every_utterance(tag, waves):
    from features.batch import FeaturePlan
    plan = FeaturePlan(winfunc=np.hamming, **cc.PLAN40)
    out, fo = plan.mfcc_batch(waves, delta_n=2)
    B = len(waves)
    assert out.shape == (B * 99, 39) and np.isfinite(out).all()
    err = np.array([normwise(out[fo[b]:fo[b + 1]],
                             dsp_oracle.mfcc_delta(waves[b].astype(np.float64), delta_n=2, winfunc=np.hamming, **cc.PLAN40))
                    for b in range(B)])
    record(f'every_utterance_{tag}_worst', err.max())
    record(f'every_utterance_{tag}_q999', np.quantile(err, 0.999))
    record(f'every_utterance_{tag}_median', np.median(err))
    print(f'{tag}: worst {err.max():.3e} (utterance {int(err.argmax())})  99.9 % {np.quantile(err, 0.999):.3e}  median {np.median(err):.3e}')
    assert err.max() <= TOL, (int(err.argmax()), err.max())


def test_every_utterance_of_the_seed1_batch():
    """configs[1], B = 1 024, drawn exactly as tools/parity_full.py draws it: utterance 322, frame 80 is a frame whose bin 1
    is cancelled by the data alone (2.63e-4 without the repair)."""
    rng = np.random.default_rng(1)
    _every_utterance('seed1_f32', (0.25 * rng.standard_normal((1024, 16000))).astype(np.float32))


@pytest.mark.parametrize('dtype', [np.float32, np.int16], ids=['f32', 'i16'])
def test_every_utterance_of_the_config2_batch(dtype):
    """The batch of test_gpu_batch.test_config2_batch_1024_vs_oracle."""
    rng = np.random.default_rng(11)
    g = rng.standard_normal((1024, 16000))
    waves = np.clip(np.round(3000 * g), -32768, 32767).astype(np.int16) if dtype == np.int16 else (0.25 * g).astype(np.float32)
    _every_utterance('config2_' + np.dtype(dtype).name, waves)


def test_fast_paths_stay():
    """The repair routes a 1536 plan with a filter of one or two taps to the generic kernel; neither model plan has one."""
    from features import _native as nat
    from features.batch import FeaturePlan
    lib = nat.load()
    assert lib.dsp_plan_has_fast_path(FeaturePlan(winfunc=np.hamming, **cc.PLAN40).plan.handle) == 1
    for rate in (44100, 48000):
        p = FeaturePlan(samplerate=rate, winlen=0.03, winstep=0.01, numcep=13, nfilt=26, nfft=1536, winfunc=np.hamming)
        assert lib.dsp_plan_has_fast_path(p.plan.handle) == 1
