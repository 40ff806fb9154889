"""Every NFFT from 16 to 4096 (dsp_plan_create_ex with DSP_PLAN_ANY_NFFT), the part that needs no GPU.

  * oracle/dsp_oracle.py equals the real reference at sizes that are neither 2^k nor 3 2^k (tests/golden/anyfft_golden.npz).
  * Every integer 16 .. 4096 makes a plan (tables in host memory, dsp_debug_host_dry_run) and takes the route it should;
    the 17 old sizes keep their pass list; what lies outside the range, or is not an old size without the flag, is refused.
  * tools/anyfft_emul.py -- both new transforms restated in NumPy on the LIBRARY's tables, read back through
    dsp_debug_plan_transform_tables -- equals numpy.fft.rfft: a wrong chirp, a spectrum stored in another order than the
    passes leave theirs, a wrong pass list all show here.
  * The inputs of tests/test_gpu_anyfft.py are feasible by the rule of tests/test_generic_cases_host.py: the single-precision
    pipeline of generic_cases.emulate_fp32 with ITS transform replaced by the emulation of the route the size takes, the
    flagged filters from fp64, stays at or below 5e-5 normwise on every clip.  A condition on the inputs, never on a kernel.
  * The near-threshold frames lie where they claim.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import anyfft_cases as ac
import generic_cases as gc
from oracle import dsp_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import anyfft_emul as emul  # noqa: E402

FEASIBLE = 5e-5
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'anyfft_golden.npz'))


def _host_plan(nfft, L=None, any_nfft=True):
    return emul.host_plan(nfft, L, any_nfft)


@pytest.mark.parametrize('cfg', ac.GOLDEN, ids=[str(c[0]) for c in ac.GOLDEN])
def test_oracle_equals_the_reference(cfg):
    nfft = cfg[0]
    kw = ac.golden_kw(*cfg)
    x = ac.golden_clip(*cfg).astype(np.float64)
    fr = ac.golden_frames(x, *cfg)
    feat, energy = dsp_oracle.fbank(x, kw['samplerate'], kw['winlen'], kw['winstep'], kw['nfilt'], nfft, kw['lowfreq'],
                                    kw['highfreq'], kw['preemph'], np.hamming)
    got = dict(mfcc=dsp_oracle.mfcc(x, winfunc=np.hamming, **kw), fbank=feat, energy=energy, powspec=dsp_oracle.powspec(fr, nfft),
               magspec=dsp_oracle.magspec(fr, nfft), logpowspec=dsp_oracle.logpowspec(fr, nfft))
    for k, v in got.items():
        ref = GOLD[f'{nfft}/{k}']
        assert v.shape == ref.shape and ref.shape[0] >= 4, (k, v.shape, ref.shape)
        assert gc.normwise(v, ref) <= 1e-12, (nfft, k, gc.normwise(v, ref))


def test_every_size_makes_a_plan_and_takes_its_route():
    from features import _native as nat
    lib = nat.load()
    assert hasattr(lib, 'dsp_plan_create_ex') and hasattr(lib, 'dsp_plan_transform')
    counts = [0, 0, 0]
    for nfft in range(16, 4097):
        L = nfft if nfft % 3 else max(1, (25 * nfft) // 32)            # both L = NFFT and L < NFFT occur
        plan = _host_plan(nfft, L)
        route, conv = plan.transform()
        assert route == ac.expected_route(nfft), (nfft, route)
        counts[route] += 1
        if route == 2:
            K, lfft = nfft // 2 + 1, min(L, nfft)
            assert conv >= lfft + K - 1 and conv == ac.expected_conv_len(nfft, L), (nfft, L, conv)
            assert conv <= 6144
        else:
            assert conv == 0, (nfft, conv)
    assert counts == [17, 87, 3977], counts       # 104 numbers 2^a 3^b 5^c in [8, 2048], 17 of them 2^k or 3 2^k
    assert _host_plan(4095, 4095).transform() == (2, 6144) and _host_plan(4093, 5000).transform() == (2, 6144)


def test_the_old_sizes_keep_their_pass_list():
    for nfft in gc.NFFTS:
        want = []
        n2 = nfft // 2
        if n2 % 3 == 0:
            want.append(3)
            n2 //= 3
        while n2 % 4 == 0:
            want.append(4)
            n2 //= 4
        if n2 % 2 == 0:
            want.append(2)
            n2 //= 2
        assert n2 == 1
        for flag in (False, True):
            plan = _host_plan(nfft, any_nfft=flag)
            assert plan.transform() == (0, 0), nfft
            assert plan.transform_tables() == (want, None, None), (nfft, flag, plan.transform_tables()[0])


def test_mixed_radix_pass_lists():
    for nfft in ac.SMOOTH:
        radix = _host_plan(nfft).transform_tables()[0]
        assert int(np.prod(radix)) == nfft // 2 and set(radix) <= {2, 3, 4, 5} and len(radix) <= 12, (nfft, radix)
    assert _host_plan(3750).transform_tables()[0] == [3, 5, 5, 5, 5]
    assert _host_plan(4050).transform_tables()[0].count(3) == 4


def test_what_is_refused():
    from features import _native as nat
    for nfft in (15, 4097, 0):
        with pytest.raises(nat.DspError, match='16 <= nfft <= 4096'):
            _host_plan(nfft, L=20)
    with pytest.raises(nat.DspError, match=r'2\^k or 3\*2\^k'):
        _host_plan(500, any_nfft=False)
    # unknown flag bits
    p = _host_plan(400)
    lib, h = nat.load(), C.c_void_p(0)
    assert lib.dsp_plan_create_ex(None, 1, C.byref(h)) == nat.EINVAL
    r, c = C.c_int32(0), C.c_int32(0)
    assert lib.dsp_plan_transform(None, C.byref(r), C.byref(c)) == nat.EINVAL
    assert lib.dsp_plan_transform(p.handle, None, C.byref(c)) == nat.EINVAL


def test_chirp_tables_are_what_the_header_says():
    for nfft in (17, 25, 1103, 4093):
        plan = _host_plan(nfft)
        _, w, spec = plan.transform_tables()
        n = np.arange(nfft, dtype=np.int64)
        want = np.exp(-1j * np.pi * ((n * n) % (2 * nfft)) / nfft)
        assert w.dtype == np.complex64 and np.max(np.abs(w - want)) <= 1e-7
        conv = plan.transform()[1]
        assert spec.shape == (conv,)
        # the stored spectrum is a permutation of fft(conj chirp laid out circularly) / conv_len
        h = np.zeros(conv, dtype=np.complex128)
        K = nfft // 2 + 1
        h[:K] = np.conj(want[:K])
        h[conv - np.arange(1, nfft)] = np.conj(want[1:nfft])
        H = np.fft.fft(h) / conv
        assert np.allclose(np.sort(np.abs(spec)), np.sort(np.abs(H)), atol=1e-6 * np.abs(H).max())


@pytest.mark.parametrize('nfft', ac.SIZES)
def test_emulation_on_the_librarys_tables_equals_rfft(nfft):
    rng = np.random.default_rng(nfft)
    worst = 0.0
    for kind in gc.LKINDS:
        L = gc.frame_len(nfft, kind)
        plan = _host_plan(nfft, L)
        fr = rng.standard_normal((3, L))
        ref = np.fft.rfft(fr[:, :min(L, nfft)], nfft)
        got = emul.rfft(plan, fr, np.float64)
        assert got.shape == ref.shape == (3, nfft // 2 + 1)
        e = float(np.max(np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)))
        worst = max(worst, e)
        assert e <= 1e-6, (nfft, kind, e)
    print(f'nfft {nfft}: fp64 emulation on the fp32-rounded tables, worst {worst:.2e} of the row maximum')


class _EmulatedRfft:
    """numpy.fft.rfft for single-precision input replaced by the emulation of the plan's route (generic_cases.emulate_fp32
    calls numpy.fft.rfft(frames[:, :lfft], nfft) on float32 frames; every other caller passes fp64 and is left alone)."""

    def __init__(self, plan):
        self.plan, self.orig, self.calls = plan, np.fft.rfft, 0

    def __call__(self, a, n=None, *args, **kw):
        a = np.asarray(a)
        if a.dtype == np.float32 and n == self.plan.nfft:
            self.calls += 1
            return emul.rfft(self.plan, a, np.float32)
        return self.orig(a, n, *args, **kw)


def _emul_vs_oracle(x, p, plan, monkeypatch):
    wf = gc.winfunc_of(p)
    ref = dsp_oracle.mfcc(np.asarray(x, dtype=np.float64), winfunc=wf, **p['kw'])
    fake = _EmulatedRfft(plan)
    with monkeypatch.context() as m:
        m.setattr(np.fft, 'rfft', fake)
        got, _ = gc.emulate_fp32(x, p['kw'], wf, flagged_from_fp64=True)
    assert fake.calls == 1 and got.shape == ref.shape
    return gc.normwise(got, ref)


@pytest.mark.parametrize('nfft', ac.SIZES)
def test_inputs_are_feasible(nfft, monkeypatch):
    worst = 0.0
    for kind in gc.LKINDS:
        p = ac.PLAN_BY_NAME[f'{nfft}-{kind}']
        plan = _host_plan(nfft, p['L'])
        assert plan.transform()[0] == (1 if nfft in ac.SMOOTH else 2)
        for dtype in (np.float32, np.int16):
            for x in gc.clips(p, dtype) + list(gc.dense_clips(p, dtype)):
                e = _emul_vs_oracle(x, p, plan, monkeypatch)
                worst = max(worst, e)
                assert e <= FEASIBLE, (p['name'], np.dtype(dtype).name, len(x), e)
    print(f'nfft {nfft}: fp32 emulation of its route with flagged filters from fp64, worst normwise {worst:.2e}')


NEAR = ac.near_cases()


@pytest.mark.parametrize('case', NEAR, ids=[c['name'] for c in NEAR])
def test_near_threshold_frames_lie_where_they_claim(case, monkeypatch):
    p = case['plan']
    x = gc.natural_clip(case['nfft'], case['seed'], case['frame'], case['dtype'])
    assert x.dtype == np.dtype(case['dtype']) and gc.cc.n_frames(len(x), p['L'], p['S']) == 13
    r = gc.filter_ratios64(x, p['kw'], gc.winfunc_of(p))[6]
    rmin = r[r > 0].min()
    lo, hi = ac.near_window(case['nfft'], case['side'])
    assert lo <= rmin < hi, (rmin, lo, hi)
    assert _emul_vs_oracle(x, p, _host_plan(case['nfft'], p['L']), monkeypatch) <= FEASIBLE


ENG = ac.engineered_cases()


@pytest.mark.parametrize('case', ENG, ids=[c['name'] for c in ENG])
def test_engineered_frames_lie_where_they_claim(case, monkeypatch):
    p = case['plan']
    x = ac.engineered_clip(case)
    assert x.dtype == np.dtype(case['dtype']) and gc.cc.n_frames(len(x), p['L'], p['S']) == 13
    j, bins = gc.narrowest_filter(p['kw'])
    r = gc.filter_ratios64(x, p['kw'], gc.winfunc_of(p))[case['frame']]
    thr = float(gc.repair_threshold(p['nfft'] // 2 + 1))
    assert r[j] == r[r > 0].min()                   # the engineered filter is the frame's smallest
    assert (r[j] >= thr) == (case['side'] == 'above'), (r[j], thr)
    e = _emul_vs_oracle(x, p, _host_plan(p['nfft'], p['L']), monkeypatch)
    print(f"{case['name']}: filter {j} bins {bins} at {r[j]:.2e} of the energy (threshold {thr:.2e}): emulation {e:.2e}")
    assert e <= FEASIBLE, e


def test_near_cases_cover_both_sides():
    cases = NEAR + ENG
    for nfft in ac.NEAR_SIZES:
        for side in ('below', 'above'):
            mine = [c for c in cases if c['nfft' if 'nfft' in c else 'key'] == nfft or c['plan']['nfft'] == nfft]
            assert sum(c['side'] == side and c['dtype'] == 'float32' for c in mine) >= 1, (nfft, side)
        assert any(c['dtype'] == 'int16' for c in mine), nfft
