"""Every NFFT from 16 to 4096 on the device: the mixed-radix and the chirp-z route of the generic kernel
(csrc/kernels_generic.h, dsp_plan_create_ex with DSP_PLAN_ANY_NFFT) against oracle/dsp_oracle.py at the 24 sizes of
tests/anyfft_cases.py, three frame lengths each, for every output kind, ragged and dense, fp32 and int16; the public
functions against the real reference's numbers (tests/golden/anyfft_golden.npz); frames on both sides of the fp64 repair's
threshold; the endpoint -> trim -> MFCC pipeline at 48 kHz / NFFT 1200 and the model's feature batch at NFFT = its frame
length; the old sizes bit for bit.

The harness is the one of tests/test_gpu_generic_configs.py: raw dsp_features_batch calls into canary-guarded buffers prefilled
with a NaN pattern (every element of every row written, pad columns and guards untouched), the project's bar of 1e-4
normwise per utterance and nothing looser.  tests/test_anyfft_host.py shows the inputs feasible.
"""
import os

import numpy as np
import pytest

import anyfft_cases as ac
import generic_cases as gc
from conftest import record
from test_gpu_canaries import _guarded
from test_gpu_generic_configs import KINDS, TOL, _Batch, _close, _oracle, _plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [(n, k, d) for n in ac.SIZES for k in gc.LKINDS for d in ('float32', 'int16')]


def _route(fplan):
    return fplan.plan.transform()


@pytest.mark.parametrize('nfft,kind,dtype', IDS, ids=[f'{n}-{k}-{d}' for n, k, d in IDS])
def test_every_plan_all_outputs(nfft, kind, dtype):
    from features import _native as nat
    from oracle import dsp_oracle as o
    p = ac.PLAN_BY_NAME[f'{nfft}-{kind}']
    fplan = _plan(p)
    assert (fplan.L, fplan.S, fplan.plan.M, fplan.C, fplan.plan.K) == (p['L'], p['S'], p['M'], p['C'], nfft // 2 + 1)
    route, conv = _route(fplan)
    assert route == ac.expected_route(nfft) == (1 if nfft in ac.SMOOTH else 2)
    assert conv == (ac.expected_conv_len(nfft, p['L']) if route == 2 else 0)
    assert not nat.load().dsp_plan_has_fast_path(fplan.plan.handle)
    worst = dict.fromkeys(KINDS + ('energy', 'mfcc_delta'), 0.0)
    for form, clips in (('ragged', gc.clips(p, dtype)), ('dense', gc.dense_clips(p, dtype))):
        b = _Batch(fplan, clips)
        refs = [_oracle(p, x) for x in b.clips]
        assert list(np.diff(b.fo)) == [len(r['mfcc']) for r in refs]
        assert (b.lay.uniform_samples > 0) == (form == 'dense')
        what = f'{p["name"]} {dtype} {form}'
        got = {k: b.run(k, what=what) for k in ('frames', 'magspec', 'powspec', 'mfcc')}
        got['fbank'], got['energy'] = b.run('fbank', what=what)
        wide = b.run('mfcc', ld=p['C'] + 3, what=what)
        again = b.run('mfcc', what=what)
        rows, _ = fplan.mfcc_batch(b.flat if form == 'ragged' else clips, sample_offsets=b.so, delta_n=2)
        assert np.array_equal(wide, got['mfcc']), f'{what}: ld_out = width + 3 changes the rows'
        assert np.array_equal(again.view(np.int32), got['mfcc'].view(np.int32)), f'{what}: two runs, different bits'
        assert rows.shape == (b.fo[-1], 3 * p['C'])
        for u, r in enumerate(refs):
            sl = slice(b.fo[u], b.fo[u + 1])
            for k in KINDS + ('energy',):
                worst[k] = max(worst[k], _close(got[k][sl], r[k], (what, k, u)))
            ref_d = o.mfcc_delta(np.asarray(b.clips[u], dtype=np.float64), delta_n=2, winfunc=gc.winfunc_of(p), **p['kw'])
            worst['mfcc_delta'] = max(worst['mfcc_delta'], _close(rows[sl], ref_d, (what, 'mfcc_delta', u)))
    for k, v in worst.items():
        record(f'anyfft_{k}_vs_oracle_route{route}', v)
        record(f'anyfft_{k}_vs_oracle_nfft{nfft}', v)
    print(f'{p["name"]} {dtype} route {route}: ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))


@pytest.mark.parametrize('cfg', ac.GOLDEN, ids=[str(c[0]) for c in ac.GOLDEN])
def test_public_functions_against_the_reference(cfg):
    import features
    from features import sigproc
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'anyfft_golden.npz'))
    nfft = cfg[0]
    kw = ac.golden_kw(*cfg)
    x = ac.golden_clip(*cfg)
    fr = ac.golden_frames(x.astype(np.float64), *cfg)
    fb_kw = {k: kw[k] for k in ('samplerate', 'winlen', 'winstep', 'nfilt', 'nfft', 'lowfreq', 'highfreq', 'preemph')}
    feat, energy = features.fbank(x, winfunc=np.hamming, **fb_kw)
    got = dict(mfcc=features.mfcc(x, winfunc=np.hamming, **kw), fbank=feat, energy=energy, powspec=sigproc.powspec(fr, nfft),
               magspec=sigproc.magspec(fr, nfft), logpowspec=sigproc.logpowspec(fr, nfft))
    for k, v in got.items():
        e = record(f'anyfft_public_{k}_vs_reference', _close(v, gold[f'{nfft}/{k}'], (nfft, k)))
        print(f'nfft {nfft} {k}: {e:.2e}')


def test_plan_transform_reports_the_route():
    from features import _plan
    for nfft in ac.SIZES + (512, 1024, 1536, 16, 4096):
        pl = _plan.frame_plan(nfft, max(1, nfft // 3), np.ones(nfft), nfft=nfft, any_nfft=True)
        route, conv = pl.transform()
        assert route == ac.expected_route(nfft), (nfft, route)
        assert conv == (ac.expected_conv_len(nfft, nfft) if route == 2 else 0), (nfft, conv)


@pytest.mark.parametrize('nfft', [512, 1024, 1536])
def test_old_sizes_through_the_new_entry_are_the_same_bits(nfft):
    """A plan of an old size made with DSP_PLAN_ANY_NFFT is the plan dsp_plan_create makes: same route, same rows, on the
    default route (the specialised kernels at 512 and 1536) and on the generic kernel."""
    from features import _native as nat
    from features import _plan
    from features.batch import FeaturePlan
    p = gc.PLAN_BY_NAME[f'{nfft}-lt']
    kw, wf = p['kw'], gc.winfunc_of(p)
    new = FeaturePlan(winfunc=wf, **kw)
    old = FeaturePlan(winfunc=wf, **kw)
    old.plan = _plan.mfcc_plan(kw['samplerate'], kw['winlen'], kw['winstep'], kw['numcep'], kw['nfilt'], nfft, kw['lowfreq'],
                               kw['highfreq'], kw['preemph'], kw['ceplifter'], kw['appendEnergy'], wf, any_nfft=False)
    assert old.plan is not new.plan and old.plan.handle != new.plan.handle
    assert new.plan.transform() == old.plan.transform() == (0, 0)
    assert new.plan.transform_tables() == old.plan.transform_tables()
    lib = nat.load()
    assert lib.dsp_plan_has_fast_path(new.plan.handle) == lib.dsp_plan_has_fast_path(old.plan.handle)
    for clips in (gc.clips(p, 'float32'), gc.dense_clips(p, 'int16')):
        bn, bo = _Batch(new, clips), _Batch(old, clips)
        for force in (0, 1):
            nat.check(lib.dsp_debug_force_generic(force))
            try:
                for kind in ('mfcc', 'powspec'):
                    a, b = bn.run(kind, what=f'{nfft} new'), bo.run(kind, what=f'{nfft} old')
                    assert np.array_equal(a.view(np.int32), b.view(np.int32)), (nfft, kind, force)
            finally:
                nat.check(lib.dsp_debug_force_generic(0))


def _near_batches():
    """(name, plan, [clips of one dtype])"""
    out = []
    for nfft, sides in ac.NEAR.items():
        p = gc.PLAN_BY_NAME[f'{nfft}-eq']
        for side, by in sides.items():
            for dt, lst in by.items():
                out.append((nfft, f'natural {nfft} {side} {dt}', p, [gc.natural_clip(nfft, s, t, dt) for s, t in lst]))
    cases = ac.engineered_cases()
    for key in ac.ENG_PLANS:
        for dt in ('float32', 'int16'):
            mine = [c for c in cases if c['key'] == key and c['dtype'] == dt]
            out.append((mine[0]['plan']['nfft'], f'engineered {key} {dt}', mine[0]['plan'], [ac.engineered_clip(c) for c in mine]))
    return out


def test_frames_on_both_sides_of_the_repair_threshold():
    from oracle import dsp_oracle as o
    worst = {}
    for nfft, name, p, clips in _near_batches():
        fplan = _plan(p)
        assert _route(fplan)[0] == ac.expected_route(nfft) != 0
        b = _Batch(fplan, np.stack(clips) if len({len(c) for c in clips}) == 1 and len(clips) > 1 else clips)
        got = b.run('mfcc', what=name)
        for u, x in enumerate(b.clips):
            ref = o.mfcc(np.asarray(x, dtype=np.float64), winfunc=gc.winfunc_of(p), **p['kw'])
            e = gc.normwise(got[b.fo[u]:b.fo[u + 1]], ref)
            worst[nfft] = max(worst.get(nfft, 0.0), e)
            print(f'{name} clip {u}: {e:.2e}')
            record(f'anyfft_near_threshold_vs_oracle_nfft{nfft}', e)
    assert set(worst) == set(ac.NEAR_SIZES)
    bad = {k: v for k, v in worst.items() if v > TOL}
    assert not bad, bad


def test_vad_pipeline_at_48k_nfft_1200():
    """VadMfccPipeline with a 25 ms window at 48 kHz (L = 1200 = NFFT, route 1): endpoints, trim, MFCC + delta + delta2
    against the oracle, utterance by utterance (the trimmed-copy path: these plans have no specialised kernel)."""
    from features.pipeline import VadMfccPipeline
    from golden_cases import make_signal
    from oracle import dsp_oracle as o
    rate = 48000
    cfg = dict(samplerate=rate, winlen=0.025, winstep=0.01, numcep=13, nfilt=26, nfft=1200, lowfreq=0, highfreq=None,
               preemph=0.97, ceplifter=22, appendEnergy=True)
    clips = [make_signal(('vad', 400 + i, 60000 + 5100 * i, rate)) for i in range(4)]
    so = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    pipe = VadMfccPipeline(rate=rate, unit_variance=False, winfunc=np.hamming, **{k: v for k, v in cfg.items() if k != 'samplerate'})
    assert pipe.features.plan.transform() == (1, 0)
    out, fo, ends = pipe.run(np.concatenate(clips), so, delta_n=2)
    assert fo[-1] == out.shape[0] and out.shape[1] == 39
    for b, c in enumerate(clips):
        lo, hi = o.basic_endpoint_detection(c, rate)
        assert (lo, min(hi, len(c))) == (int(ends[b, 0]), int(ends[b, 1])) or (lo, hi) == (int(ends[b, 0]), int(ends[b, 1]))
        ref = o.mfcc_delta(np.asarray(c[lo:hi], dtype=np.float64), delta_n=2, winfunc=np.hamming, **cfg)
        got = out[fo[b]:fo[b + 1]]
        assert got.shape == ref.shape, (b, got.shape, ref.shape)
        record('anyfft_vad_pipeline_nfft1200', _close(got, ref, ('pipeline', b)))


@pytest.mark.parametrize('nfft', [25, 1103, 4095])
def test_mfcc_delta_rows_stay_inside_their_buffer(nfft):
    """dsp_features_batch's outputs are guarded in every test above; this is dsp_mfcc_delta_batch (scratch and delta pass
    behind the generic kernel) between sentinels, ragged and dense, and the same bits on a second run."""
    import torch
    from features import _native as nat
    dev = torch.device('cuda', 0)
    for kind in gc.LKINDS:
        p = ac.PLAN_BY_NAME[f'{nfft}-{kind}']
        fplan = _plan(p)
        for clips in (gc.clips(p, 'int16'), gc.dense_clips(p, 'float32')):
            b = _Batch(fplan, clips)
            runs = []
            for _ in range(2):
                buf, ptr, check = _guarded(b.lay.total_frames * fplan.width(2) * 4, dev)
                fplan.run_raw(b.wave.data_ptr(), b.wd, b.lay, ptr, 2, torch.cuda.current_stream(dev))
                runs.append(check(f'{p["name"]} mfcc + delta').view(np.int32).copy())
            assert np.isfinite(runs[0].view(np.float32)).all()
            assert np.array_equal(runs[0], runs[1]), f'{p["name"]}: two runs, different bits'


@pytest.mark.parametrize('rate,nfft,route', [(48000, 1440, 1), (44100, 1323, 2)], ids=['48k-1440', '44k-1323'])
def test_model_feature_batch_at_the_frame_length(rate, nfft, route):
    """ModelFeatureBatch (model.py:52-88) with NFFT = its 30 ms frame instead of 1536 -- the size that stops the reference's
    truncation warning -- against the oracle's model path with the same nfft, clip by clip."""
    from features.model_glue import ModelFeatureBatch
    from golden_cases import make_signal
    from oracle import dsp_oracle as o
    clips = [make_signal(('vad', 420 + i, 50000 + 7000 * i, rate, 0.5 + 0.1 * i)) for i in range(3)]
    so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
    mfb = ModelFeatureBatch(rate=rate, nfft=nfft)
    inp, len0, ends = mfb.run(np.concatenate(clips), so)
    got = inp.cpu().numpy()
    assert got.shape == (200, 3, 39)
    for b, c in enumerate(clips):
        lo, hi = o.basic_endpoint_detection(c, rate)
        (m0, m1, m2), n = o.model_feature_extract_mfcc(o.model_endpoint_scale(np.asarray(c), lo, hi), rate, nfft=nfft)
        assert len0[b] == n
        ref = np.concatenate([m0, m1, m2], axis=1)[:n]
        record(f'anyfft_model_batch_route{route}', _close(got[:n, b, :13], ref[:, :13], ('m0', b)))
        record(f'anyfft_model_batch_route{route}', _close(got[:n, b, 13:], ref[:, 13:], ('m1, m2', b)))
        assert not got[n:, b].any()
