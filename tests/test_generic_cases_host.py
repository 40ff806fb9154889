"""The cases of tests/generic_cases.py, the part that needs no GPU.

  * The host table builders (features/_plan.py: mel triangles, their CSR form, DCT x lifter, frame sizes) against the
    oracle on the 51 plans of every accepted NFFT and 300 random ones -- both device routes read these tables, so a
    comparison of one route with the other cannot see a wrong one.
  * The inputs are feasible: a single-precision pipeline with numpy's FFT, the filters the kernels' rule flags taken from
    fp64, stays at or below 5e-5 normwise (half the device bar) on every clip the GPU tests use.  The cap is a condition on
    the INPUTS, checked against the emulation, never against a kernel.
  * The near-threshold clips do what they claim.
"""
import numpy as np
import pytest

import generic_cases as gc
from oracle import dsp_oracle

FEASIBLE = 5e-5
RANDOM300 = gc.random_plans(77, 300)
RANDOM60 = gc.random_plans(gc.RANDOM_SEED, gc.N_RANDOM)


def _emul_vs_oracle(x, plan_kw, wf, substitute=True):
    ref = dsp_oracle.mfcc(np.asarray(x, dtype=np.float64), winfunc=wf, **plan_kw)
    got, _ = gc.emulate_fp32(x, plan_kw, wf, flagged_from_fp64=substitute)
    assert got.shape == ref.shape
    return gc.normwise(got, ref)


def test_the_plans_are_what_the_issue_lists():
    assert len(gc.NFFTS) == 17 and len(gc.PLANS) == 51
    assert set(gc.NFFTS) == {n for n in range(16, 4097) if any(n == b << k for b in (1, 3) for k in range(13))}
    p = gc.PLAN_BY_NAME['4096-gt']
    assert max(gc.clip_lengths(p['L'], p['S'])) == 30726
    assert gc.PLAN_BY_NAME['16-eq']['M'] == 4 and gc.PLAN_BY_NAME['16-eq']['C'] == 4
    assert len({p['nfft'] for p in RANDOM60}) >= 12


@pytest.mark.parametrize('plans', [gc.PLANS, RANDOM300, RANDOM60], ids=['every_nfft', 'random300', 'random60'])
def test_sizes_round_trip_and_equal_the_oracles(plans):
    from features import _plan
    for p in plans:
        kw = p['kw']
        assert gc.sizes(kw) == (p['L'], p['S']), p['name']
        assert _plan.frame_sizes(kw['winlen'] * kw['samplerate'], kw['winstep'] * kw['samplerate']) == (p['L'], p['S']), p['name']
        for n in (1, p['L'] - 1, p['L'], p['L'] + 1, p['L'] + p['S'], 6 * p['L'] + 1):
            assert gc.cc.n_frames(n, p['L'], p['S']) == dsp_oracle.frame_geometry(n, p['L'], p['S'])[2]


def test_table_builders_equal_the_oracle_on_every_plan():
    from features import _plan
    n_zero_rows = n_repeated = 0
    for p in gc.PLANS + RANDOM300 + RANDOM60:
        kw = p['kw']
        args = (kw['nfilt'], kw['nfft'], kw['samplerate'], kw['lowfreq'], kw['highfreq'])
        ref = dsp_oracle.get_filterbanks(*args)
        fb = _plan.filterbank_matrix(*args)
        assert np.array_equal(fb, ref), p['name']
        assert np.array_equal(_plan.mel_edges(*args), dsp_oracle.mel_bin_edges(*args)), p['name']
        start, count, w = _plan.mel_csr(fb)
        assert w.dtype == np.float32 and int(count.sum()) == w.size
        dense = np.zeros_like(fb)
        off = 0
        for j in range(fb.shape[0]):
            assert 0 <= start[j] and start[j] + count[j] <= fb.shape[1], (p['name'], j)
            dense[j, start[j]:start[j] + count[j]] = w[off:off + count[j]]
            off += count[j]
            if not ref[j].any():
                assert count[j] == 0, (p['name'], j)
                n_zero_rows += 1
        assert np.all(np.abs(dense - ref) <= 2.0 ** -24 * np.abs(ref)), p['name']      # fp32 rounding of each weight, zeros exact
        n_repeated += int(np.any(np.diff(dsp_oracle.mel_bin_edges(*args)) == 0))
        C = min(kw['numcep'], kw['nfilt'])
        want = dsp_oracle.lifter_vector(C, kw['ceplifter'])[:, None] * dsp_oracle.dct2_ortho_matrix(kw['nfilt'], C)
        got = _plan.dct_lifter_matrix(kw['nfilt'], kw['numcep'], kw['ceplifter'])
        assert got.shape == want.shape and np.max(np.abs(got - want)) <= 1e-12, p['name']
    assert n_zero_rows > 50 and n_repeated > 20, (n_zero_rows, n_repeated)     # all-zero rows and repeated edges occur


def test_repair_rule_mirror():
    """The mirror of dsp_repair_threshold: today's constant at 257 bins and above, never below it, monotone in K."""
    assert gc.repair_threshold(257) == np.float32(7e-10) and gc.repair_threshold(769) == np.float32(7e-10)
    assert gc.repair_threshold(2049) == np.float32(7e-10)
    prev = np.inf
    for nfft in gc.NFFTS:
        t = gc.repair_threshold(nfft // 2 + 1)
        assert t.dtype == np.float32 and np.float32(7e-10) <= t <= prev
        prev = t
    assert abs(float(gc.repair_threshold(9)) / (7e-10 * (257 / 9) ** 3) - 1) < 1e-6


@pytest.mark.parametrize('nfft', gc.NFFTS)
def test_every_nfft_inputs_are_feasible(nfft):
    worst = 0.0
    for kind in gc.LKINDS:
        p = gc.PLAN_BY_NAME[f'{nfft}-{kind}']
        wf = gc.winfunc_of(p)
        for dtype in (np.float32, np.int16):
            for x in gc.clips(p, dtype) + list(gc.dense_clips(p, dtype)):
                e = _emul_vs_oracle(x, p['kw'], wf)
                worst = max(worst, e)
                assert e <= FEASIBLE, (p['name'], np.dtype(dtype).name, len(x), e)
    print(f'nfft {nfft}: emulation with flagged filters from fp64, worst normwise {worst:.2e}')


def test_random_plan_inputs_are_feasible():
    worst = 0.0
    for i, p in enumerate(RANDOM60):
        wf = gc.winfunc_of(p)
        for x in gc.random_clips(p, i):
            e = _emul_vs_oracle(x, p['kw'], wf)
            worst = max(worst, e)
            assert e <= FEASIBLE, (p['name'], p['kw'], p['winfunc'], len(x), e)
    assert len({p['nfft'] for p in RANDOM60}) >= 12
    print(f'60 random plans: worst normwise {worst:.2e}')


def _host_has_fast_path(cfg, winfunc):
    """dsp_plan_has_fast_path of the plan built with its tables in host memory (no device is touched)."""
    from features import _native as nat
    from features import _plan
    L, S = _plan.frame_sizes(cfg['winlen'] * cfg['samplerate'], cfg['winstep'] * cfg['samplerate'])
    fb = _plan.filterbank_matrix(cfg['nfilt'], cfg['nfft'], cfg['samplerate'], cfg['lowfreq'], cfg['highfreq'])
    dct = _plan.dct_lifter_matrix(cfg['nfilt'], cfg['numcep'], cfg['ceplifter'])
    plan = _plan.Plan(L, S, cfg['nfft'], np.asarray(winfunc(L), dtype=np.float64), preemph=cfg['preemph'], fb=fb, dct=dct,
                      append_energy=cfg['appendEnergy'], host_dry_run=True)
    return bool(nat.load().dsp_plan_has_fast_path(plan.handle))


@pytest.mark.parametrize('nfft', [512, 1536])
def test_fuzz_inputs_are_feasible(nfft):
    """The batches of tests/test_gpu_fuzz.py::test_random_configs_fast_vs_generic, utterance by utterance."""
    n, worst = 0, 0.0
    for trial, cfg, wf, L, S, flat, so, dense in gc.fuzz_trials(nfft, _host_has_fast_path):
        n += 1
        assert gc.sizes(cfg) == (L, S)
        for b in range(len(so) - 1):
            e = _emul_vs_oracle(flat[so[b]:so[b + 1]], cfg, wf)
            worst = max(worst, e)
            assert e <= FEASIBLE, (trial, cfg, b, e)
    assert n >= 15, n
    print(f'nfft {nfft}: {n} fuzz configurations, worst normwise {worst:.2e}')


NAT = gc.natural_cases()
ENG = gc.engineered_cases()


@pytest.mark.parametrize('case', NAT, ids=[c['name'] for c in NAT])
def test_natural_frames_lie_just_above_the_constant(case):
    p = case['plan']
    x = gc.natural_clip(case['nfft'], case['seed'], case['frame'], case['dtype'])
    assert x.dtype == np.dtype(case['dtype']) and gc.cc.n_frames(len(x), p['L'], p['S']) == 13
    r = gc.filter_ratios64(x, p['kw'], gc.winfunc_of(p))[6]
    rmin = r[r > 0].min()
    assert gc.REPAIR_RATIO <= rmin < 100 * gc.REPAIR_RATIO, rmin
    assert _emul_vs_oracle(x, p['kw'], gc.winfunc_of(p)) <= FEASIBLE


def test_natural_cases_cover_the_sizes():
    for nfft in (16, 24, 64, 192):
        assert len(gc.NATURAL[nfft]['float32']) == 8 and len(gc.NATURAL[nfft]['int16']) == 2
    # what a single-precision pipeline WITHOUT the fp64 values makes of them (a figure, not a claim: how far a frame in
    # this window is off depends on its phase)
    for nfft in (16, 24, 64, 192):
        p = gc.PLAN_BY_NAME[f'{nfft}-eq']
        worst = max(_emul_vs_oracle(gc.natural_clip(nfft, s, t, 'float32'), p['kw'], gc.winfunc_of(p), substitute=False)
                    for s, t in gc.NATURAL[nfft]['float32'])
        print(f'nfft {nfft}: natural near-threshold clips without substitution, worst normwise {worst:.2e}')


@pytest.mark.parametrize('case', ENG, ids=[c['name'] for c in ENG])
def test_engineered_frames_do_what_they_claim(case):
    p = case['plan']
    wf = gc.winfunc_of(p)
    x = gc.engineered_clip(case)
    assert x.dtype == np.dtype(case['dtype'])
    T = gc.cc.n_frames(len(x), p['L'], p['S'])
    assert T == 13 and case['frame'] < T
    if case['pad']:
        assert case['frame'] == T - 1 and len(x) < (T - 1) * p['S'] + p['L']       # the zero-padded last frame
    j, bins = gc.narrowest_filter(p['kw'])
    assert len(bins) <= 3, bins
    got = gc.cc.achieved(x, p['L'], p['S'], p['nfft'], p['kw']['preemph'], np.asarray(wf(p['L']), dtype=np.float64),
                         (case['frame'],), bins) / case['ratio']
    assert got.max() <= 1.05, got
    plain = _emul_vs_oracle(x, p['kw'], wf, substitute=False)
    fixed = _emul_vs_oracle(x, p['kw'], wf, substitute=True)
    print(f"{case['name']}: filter {j} bins {bins}: plain {plain:.2e}, flagged from fp64 {fixed:.2e}")
    if case['breaks']:
        assert plain > 1e-4, plain
    assert fixed <= FEASIBLE, fixed


def test_forced_cases_have_a_specialised_kernel():
    for case in ENG:
        if case['force']:
            assert _host_has_fast_path(case['plan']['kw'], gc.winfunc_of(case['plan']))
    assert {c['plan']['nfft'] for c in ENG} == {64, 256, 1024, 1536, 2048} and any(c['force'] for c in ENG)
    assert any(c['plan']['L'] > c['plan']['nfft'] for c in ENG) and any(c['pad'] for c in ENG)
