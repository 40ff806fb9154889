"""The engineered cancelled-filter clips (tests/cancel_cases.py), the part that needs no GPU: the generator reaches the
ratio it is asked for, the oracle is stable at those frames and equals the reference there, and the cases bite -- a
single-precision pipeline with numpy's FFT misses the 1e-4 bar on them."""
import os

import numpy as np
import pytest

import cancel_cases as cc
from oracle import dsp_oracle

IDS = [c['name'] for c in cc.CASES]


@pytest.fixture(scope='module')
def cancel_golden():
    return np.load(os.path.join(os.path.dirname(__file__), 'golden', 'cancel_golden.npz'))


@pytest.mark.parametrize('case', cc.CASES, ids=IDS)
def test_generator_reaches_the_ratio(case, cancel_golden):
    x = cc.make_input(case)
    assert x.dtype == np.dtype(case['dtype']) and len(x) == case['n']
    assert np.array_equal(x, cancel_golden[f"{case['name']}/x"]), 'the stored clip is not what the generator makes'
    kw, wf = cc.plan_kwargs(case)
    win = np.asarray(wf(cc.L), dtype=np.float64)
    got = cc.achieved(x, cc.L, cc.S, cc.NFFT, kw['preemph'], win, case['frames'], case['bins']) / case['ratio']
    if case['dtype'] == 'int16':
        assert got.max() <= 1.0, got
    else:
        assert np.all(np.abs(got - 1.0) <= 0.02), got


@pytest.mark.parametrize('case', cc.CASES, ids=IDS)
def test_oracle_is_stable_at_the_tiny_bin(case):
    """The oracle's own spectrum (numpy's fp64 FFT of its frames) against a direct longdouble DFT sum of the samples."""
    x = cc.make_input(case)
    kw, wf = cc.plan_kwargs(case)
    win = np.asarray(wf(cc.L), dtype=np.float64)
    frames = dsp_oracle.framesig(dsp_oracle.preemphasis(x.astype(np.float64), kw['preemph']), cc.L, cc.S, wf)
    spec = np.fft.rfft(frames, cc.NFFT)
    xl = x.astype(np.longdouble)
    for t in case['frames']:
        for k in case['bins']:
            direct = complex(np.sum(cc.bin_functional(len(x), cc.L, cc.S, cc.NFFT, kw['preemph'], win, t, k) * xl))
            assert abs(spec[t, k] - direct) <= 1e-6 * abs(direct), (t, k, spec[t, k], direct)


@pytest.mark.parametrize('case', cc.CASES, ids=IDS)
def test_oracle_matches_reference_on_cancelled_frames(case, cancel_golden):
    kw, wf = cc.plan_kwargs(case)
    ref = cancel_golden[f"{case['name']}/mfcc"]
    got = dsp_oracle.mfcc(cancel_golden[f"{case['name']}/x"].astype(np.float64), winfunc=wf, **kw)
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, float(np.max(np.abs(ref))))


@pytest.mark.parametrize('case', [c for c in cc.CASES if c['whole'] and c['ratio'] <= 1e-5],
                         ids=[c['name'] for c in cc.CASES if c['whole'] and c['ratio'] <= 1e-5])
def test_case_breaks_a_single_precision_pipeline(case):
    x = cc.make_input(case)
    kw, wf = cc.plan_kwargs(case)
    ref = dsp_oracle.mfcc(x.astype(np.float64), winfunc=wf, **kw)
    assert cc.normwise(cc.emulate_fp32(x, kw, wf), ref) > 1e-4


def test_vad_case_keeps_its_endpoints_and_bites():
    """The burst-in-noise clip of the pipeline route: engineered relative to the oracle's left endpoint, endpoints unmoved."""
    case = cc.make_vad_case()
    assert case is not None, 'no seed of VAD_SEEDS keeps the endpoints'
    seed, clip, left, right = case
    lo, hi = dsp_oracle.basic_endpoint_detection(clip, 16000)
    assert (lo, min(hi, len(clip))) == (left, right)
    lo0, hi0 = dsp_oracle.basic_endpoint_detection(cc.burst_clip(seed), 16000)
    assert (lo0, min(hi0, len(clip))) == (left, right)
    seg = clip[left:right]
    got = cc.achieved(seg, cc.L, cc.S, cc.NFFT, 0.97, np.hamming(cc.L), cc.VAD_FRAMES, cc.VAD_BINS) / cc.VAD_RATIO
    assert np.all(np.abs(got - 1.0) <= 0.02), got
    ref = dsp_oracle.mfcc(seg.astype(np.float64), winfunc=np.hamming, **cc.PLAN40)
    assert cc.normwise(cc.emulate_fp32(seg, cc.PLAN40, np.hamming), ref) > 1e-4


def test_every_axis_value_appears():
    assert {c['ratio'] for c in cc.CASES} >= set(cc.RATIOS)
    assert {c['dtype'] for c in cc.CASES} == {'float32', 'int16'}
    assert {c['winfunc'] for c in cc.CASES} == {'hamming', 'hanning'} and any(c['preemph'] == 0.0 for c in cc.CASES)
    b40 = {c['bins'] for c in cc.CASES if c['plan'] == '40'}
    assert b40 >= {(1,), (2, 3), (1, 2, 3), (2,)}
    assert {c['bins'] for c in cc.CASES if c['plan'] == '64'} >= {(0,), (3,), (5,), (6, 7), (0, 1, 2, 3, 4, 5)}
    assert any(c['plan'] == '26' and c['bins'] == (1, 2, 3) for c in cc.CASES)
    fr = {c['frames'] for c in cc.CASES}
    assert fr >= {(0,), (7, 8), tuple(range(8)), (cc.LAST,), (cc.LASTPAD,)} and any(c['n'] < cc.L for c in cc.CASES)


def test_narrow_filters_are_where_the_cases_say():
    def narrow(nfilt, rate=16000):
        fb = dsp_oracle.get_filterbanks(nfilt, 512, rate, 0, None)
        return {j: tuple(np.nonzero(fb[j])[0]) for j in range(nfilt) if np.count_nonzero(fb[j]) <= 2}
    assert narrow(40) == {0: (1,), 1: (2, 3)}
    n64 = narrow(64)       # seventeen of them; the cases use the first eight
    assert {j: n64[j] for j in range(8)} == {0: (0,), 1: (1,), 2: (2,), 3: (3,), 4: (4,), 5: (5,), 6: (6, 7), 7: (7, 8)}
    assert narrow(26) == {} and narrow(20) == {} and narrow(40, 8000) == {}
    for rate in (44100, 48000):
        fb = dsp_oracle.get_filterbanks(26, 1536, rate, 0, None)
        assert min(np.count_nonzero(fb[j]) for j in range(26)) >= 3
