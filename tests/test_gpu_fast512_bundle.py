"""The NFFT = 512 kernel after its spectrum stores were paired (kernels_fast512.h: f512_lds_store2, lane 0's odd bins
stored from inside its rows-0/16 branch): every instantiation that shares the code, at the smallest shapes that can go
wrong, each compared three ways --

  * against the oracle at the project's bar (normwise <= 1e-4 per utterance),
  * dsp_mfcc_delta_batch against the MFCC kernel followed by dsp_delta_batch, bit for bit, on NaN-filled outputs,
  * against the generic kernel (dsp_debug_force_generic) at the existing tolerance of two fp32 pipelines (5e-5 normwise,
    tests/test_gpu_batch.py).

Dense batches of 512 utterances: the fused kernel takes a batch of >= 2 x CUs utterances with T >= 57 frames (512 on the
256 CUs of an MI355X; the count of the device at hand is printed).  The three short shapes (T = 6, 8, 9) are served by the
MFCC-only instantiation plus the delta kernel inside dsp_mfcc_delta_batch itself: T = 6 is less than one 8-frame group,
T = 8 one full group per utterance, T = 9 flat grouping with a seam in every group.  One batch per dtype is generated
once and shared; the plans differ in their filter bank only."""
import numpy as np
import pytest

import cancel_cases as cc
from conftest import normwise
from oracle import dsp_oracle

pytestmark = pytest.mark.gpu

CFG = dict(samplerate=16000, winlen=0.025, winstep=0.01, numcep=13, nfilt=40, nfft=512, lowfreq=0,
           highfreq=None, preemph=0.97, ceplifter=22, appendEnergy=True)
TOL = 1e-4            # the project's bar against the oracle
TOL_GENERIC = 5e-5    # two fp32 pipelines, each ~1e-5 from fp64 (tests/test_gpu_batch.py)
B = 512

_PLANS, _BATCHES = {}, {}


def _plan(nfilt=40):
    from features.batch import FeaturePlan
    if nfilt not in _PLANS:
        _PLANS[nfilt] = (FeaturePlan(winfunc=np.hamming, **dict(CFG, nfilt=nfilt)), dict(CFG, nfilt=nfilt))
    return _PLANS[nfilt]


def _batch(N, dtype):
    key = (N, np.dtype(dtype).name)
    if key not in _BATCHES:
        rng = np.random.default_rng(9100 + N)
        if np.dtype(dtype) == np.int16:
            w = np.clip(np.round(3000 * rng.standard_normal((B, N))), -32768, 32767).astype(np.int16)
        else:
            w = (0.25 * rng.standard_normal((B, N), dtype=np.float32)).astype(np.float32)
        w.setflags(write=False)
        _BATCHES[key] = w
    return _BATCHES[key]


def _rows(plan, waves, delta_n=2):
    """-> (dsp_mfcc_delta_batch rows, MFCC kernel + dsp_delta_batch rows, generic-kernel rows, T), NaN-filled outputs."""
    import torch
    from features import _native as nat
    lib = nat.load()
    n_utt, N = waves.shape
    C = plan.C
    lay = plan.layout(waves)
    T = lay.total_frames // n_utt
    dev = torch.device('cuda', 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f'{n_utt} utterances x {T} frames on {cus} CUs: the fused kernel takes this batch: {n_utt >= 2 * cus and T >= 57}')
    d_wave = torch.from_numpy(np.array(waves)).to(dev)      # (a copy: the shared batches are read-only)
    wd = nat.WAVE_I16 if waves.dtype == np.int16 else nat.WAVE_F32
    one = torch.full((n_utt * T, 3 * C), float('nan'), device=dev)
    plan.run_raw(d_wave.data_ptr(), wd, lay, one.data_ptr(), delta_n, None)
    two = torch.full((n_utt * T, 3 * C), float('nan'), device=dev)
    nat.check(lib.dsp_features_batch(plan.plan.handle, d_wave.data_ptr(), wd, None, None, n_utt, n_utt * T, N, nat.OUT_MFCC,
                                     two.data_ptr(), 3 * C, None, None))
    nat.check(lib.dsp_delta_batch(two.data_ptr(), 3 * C, None, n_utt, n_utt * T, T, C, delta_n, two.data_ptr() + C * 4, 3 * C,
                                  two.data_ptr() + 2 * C * 4, 3 * C, None))
    gen = torch.full((n_utt * T, 3 * C), float('nan'), device=dev)
    try:
        nat.check(lib.dsp_debug_force_generic(1))
        plan.run_raw(d_wave.data_ptr(), wd, lay, gen.data_ptr(), delta_n, None)
    finally:
        nat.check(lib.dsp_debug_force_generic(0))
    torch.cuda.synchronize()
    return one.cpu().numpy(), two.cpu().numpy(), gen.cpu().numpy(), T


def _three_ways(plan, cfg, waves, T_expected, sampled, delta_n=2):
    one, two, gen, T = _rows(plan, waves, delta_n)
    assert T == T_expected, T
    assert np.isfinite(one).all() and np.isfinite(gen).all()
    assert np.array_equal(one.view(np.int32), two.view(np.int32)), np.argwhere(one != two)[:8]
    eg = normwise(one, gen)
    print(f'against the generic kernel, whole batch: normwise {eg:.3e}')
    worst = 0.0
    for b in sampled:
        ref = dsp_oracle.mfcc_delta(waves[b].astype(np.float64), delta_n=delta_n, winfunc=np.hamming, **cfg)
        err = normwise(one[b * T:(b + 1) * T], ref)
        print(f'utterance {b}: normwise error against the oracle {err:.3e}')
        worst = max(worst, err)
    assert eg <= TOL_GENERIC, eg
    assert worst <= TOL, worst
    return one


_SHAPE3 = {}


@pytest.mark.parametrize('N,T', [(1200, 6), (1520, 8), (1680, 9)], ids=['T6', 'T8', 'T9'])
def test_short_utterances(N, T):
    """Cases 1-3: less than one group; T % 8 = 0; flat grouping with a seam in every group."""
    plan, cfg = _plan()
    one = _three_ways(plan, cfg, _batch(N, np.float32), T, (0, 255, 511))
    if T == 9:
        _SHAPE3['rows'] = one


def test_flagship_shape_fp32():
    """Case 4: 512 x 1 s, the tag-1 fused instantiation."""
    plan, cfg = _plan()
    _three_ways(plan, cfg, _batch(16000, np.float32), 99, (0, 511))


def test_flagship_shape_int16():
    """Case 5: the same shape from int16 samples."""
    plan, cfg = _plan()
    _three_ways(plan, cfg, _batch(16000, np.int16), 99, (1, 510))


@pytest.mark.parametrize('nfilt', [26, 39, 44], ids=['tag2_26_filters', 'tag0_39_filters', 'catch_all_44_filters'])
def test_flagship_shape_other_plans(nfilt):
    """Cases 6-8: the second tagged layout; a plan on the run-time layout (39 filters fit the 40-filter block table); the
    catch-all instantiation (six filter iterations, 32 pass-1 rows)."""
    plan, cfg = _plan(nfilt)
    _three_ways(plan, cfg, _batch(16000, np.float32), 99, (2, 509))


def test_mfcc_only_at_shape_3():
    """DSP_OUT_MFCC alone at T = 9: the oracle's cepstra, the generic kernel's, and -- bit for bit -- the first 13 columns of
    the rows dsp_mfcc_delta_batch wrote for the same batch."""
    import torch
    from features import _native as nat
    lib = nat.load()
    plan, cfg = _plan()
    waves = _batch(1680, np.float32)
    T, C = 9, plan.C
    dev = torch.device('cuda', 0)
    d_wave = torch.from_numpy(np.array(waves)).to(dev)      # (a copy: the shared batches are read-only)
    outs = []
    for force in (0, 1):
        o = torch.full((B * T, C), float('nan'), device=dev)
        try:
            nat.check(lib.dsp_debug_force_generic(force))
            nat.check(lib.dsp_features_batch(plan.plan.handle, d_wave.data_ptr(), nat.WAVE_F32, None, None, B, B * T, 1680,
                                             nat.OUT_MFCC, o.data_ptr(), C, None, None))
        finally:
            nat.check(lib.dsp_debug_force_generic(0))
        torch.cuda.synchronize()
        outs.append(o.cpu().numpy())
    fast, gen = outs
    assert np.isfinite(fast).all()
    eg = normwise(fast, gen)
    print(f'against the generic kernel: normwise {eg:.3e}')
    assert eg <= TOL_GENERIC, eg
    for b in (0, 300, 511):
        ref = dsp_oracle.mfcc(waves[b].astype(np.float64), winfunc=np.hamming, **cfg)
        err = normwise(fast[b * T:(b + 1) * T], ref)
        print(f'utterance {b}: normwise error against the oracle {err:.3e}')
        assert err <= TOL, (b, err)
    rows = _SHAPE3.get('rows')
    if rows is None:      # run on its own: the rows of case 3 are computed here
        rows = _three_ways(plan, cfg, waves, T, (0,))
    assert np.array_equal(fast.view(np.int32), np.ascontiguousarray(rows[:, :C]).view(np.int32))


def test_cancelled_filter_is_still_named():
    """An engineered clip (tests/cancel_cases.py: filter 16 of the 40-filter bank, a slot of the middle filter iteration,
    cancelled to 1e-5 of its frame's median in frame 5) as utterance 300 of a dense batch of 13-frame clips: a single-precision
    spectrum loses that frame, so the rows meet the oracle only if the fp64 repair recomputes the right filter."""
    case = cc.BY_NAME['p40_f16_r1e-5']
    assert case['whole'] and case['plan'] == '40' and case['dtype'] == 'float32'
    plan, cfg = _plan()
    waves = np.array(_batch(cc.N13, np.float32))
    waves[300] = cc.make_input(case)
    one = _three_ways(plan, cfg, waves, cc.n_frames(cc.N13), (300, 0))
    ref = dsp_oracle.mfcc_delta(waves[300].astype(np.float64), delta_n=2, winfunc=np.hamming, **cfg)
    T = cc.n_frames(cc.N13)
    t = case['frames'][0]
    err = float(np.max(np.abs(one[300 * T + t, :13] - ref[t, :13])) / np.max(np.abs(ref)))
    print(f'the cancelled frame alone: {err:.3e}')
    assert err <= TOL, err
