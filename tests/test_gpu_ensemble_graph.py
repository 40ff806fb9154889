"""Raw clips to labels as ONE HIP graph (features/ensemble.py: ``EnsembleBatch.capture``, ``MixedRateEnsembleBatch.capture``,
``run(sync_free=True)``): front end, head with the lengths on the device, pre-emphasised trim, pitch features and gate.

``replay()`` is compared with the eager ``run()`` -- the route with the host synchronisation in the middle -- on the same
content: integers (pred, used, valid, len0, endpoints) equal, the pitch features and the SVM decisions equal bytes, logits
within 2e-5 max(1, |ref|) (the front end's fp64 statistics are accumulated in an order that may differ from run to run).
Buffer ownership is shown without freeing anything: ``nat.SCRATCH.get`` raises while ``capture()`` runs, so no library scratch
pointer can have been recorded, and a replay after a larger eager pitch call -- which replaces every scratch slot of the
pitch chain -- still gives the first replay's bytes."""
import numpy as np
import pytest

from conftest import record
from ensemble_cases import PAIRS, THRESHOLDS, make_clips
from golden_cases import make_signal

pytestmark = pytest.mark.gpu

BAR = 2e-5
B = 5


def _np(t):
    return t.detach().cpu().numpy()


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


@pytest.fixture(scope='module')
def env():
    import os
    import types
    import torch
    from features import _native as nat
    from features import ensemble
    from features.classifier import HMRNNHead, fill_parameters
    from conftest import ROOT
    nat.require_device()
    dev = torch.device('cuda', 0)
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ensemble_golden.npz')) as z:
        models = [{k: z[f'svm{p[0]}{p[1]}/{k}'] for k in ('scale', 'support_vectors', 'dual_coef', 'intercept', 'gamma', 'classes')}
                  for p in PAIRS]
    rules = [(p, t, ensemble.PitchSVM.from_arrays(m['support_vectors'], m['dual_coef'], m['intercept'], m['gamma'], m['classes'],
                                                  scale=m['scale']))
             for p, t, m in zip(PAIRS, THRESHOLDS, models)]                     # the fixture's rules
    # two more, so that more of the 20 labels are gated (a seeded head is far from confident)
    rng = np.random.default_rng(7)
    for pair in ((2, 3), (12, 13)):
        rules.append((pair, 0.9, ensemble.PitchSVM.from_arrays(rng.standard_normal((40, 5)), rng.uniform(-1, 1, 40), rng.uniform(-0.2, 0.2),
                                                               0.1, pair, scale=rng.uniform(0.5, 2.0, 5), center=rng.standard_normal(5))))
    head = HMRNNHead().to(dev).eval()
    fill_parameters(head, 3)
    clips, rate = make_clips()
    return types.SimpleNamespace(nat=nat, ens=ensemble, torch=torch, dev=dev, rules=rules, head=head, clips=clips[:B], rate=rate)


def _compare(tag, got, want, n):
    """``got``: a replayed (or sync-free) namespace, every field on the device; ``want``: the eager run()'s."""
    assert str(got.len0.dtype) == 'torch.int32' and got.len0.is_cuda
    assert str(got.endpoints.dtype) == 'torch.int64' and tuple(got.endpoints.shape) == (n, 2) and got.endpoints.is_cuda
    for name in ('pred', 'used', 'valid'):
        assert np.array_equal(_np(getattr(got, name)), _np(getattr(want, name))), (tag, name)
    assert np.array_equal(_np(got.len0), np.asarray(want.len0)) and np.array_equal(_np(got.endpoints), np.asarray(want.endpoints)), tag
    assert _np(got.feat).tobytes() == _np(want.feat).tobytes(), (tag, 'feat')
    assert _np(got.decision).tobytes() == _np(want.decision).tobytes(), (tag, 'decision')
    e = record(f'ensemble_graph_logits_{tag}', _err(_np(got.logits), _np(want.logits)))
    print(f'{tag}: logits err {e:.3g}')
    assert e <= BAR
    assert int(_np(got.n_clamped)[0]) == 0
    print(f'{tag}: rules fired on {int((_np(want.used) != 0).sum())} of {n} clips')


def _snapshot(ns):
    return {k: _np(getattr(ns, k)).tobytes() for k in ('pred', 'used', 'valid', 'len0', 'endpoints', 'feat', 'decision', 'logits', 'prob')}


def test_capture_replays_the_whole_chain(env, monkeypatch):
    torch, nat = env.torch, env.nat
    from features.pitch import pitch_feature_batch
    so = _offsets(env.clips)
    flat = np.concatenate(env.clips)
    buf = torch.from_numpy(flat).to(env.dev)
    eb = env.ens.EnsembleBatch(env.rate, env.head, env.rules)

    def boom(*a, **k):
        raise AssertionError('library scratch was asked for while the graph was being built')
    with monkeypatch.context() as m:                       # no library scratch pointer can be recorded
        m.setattr(nat.SCRATCH, 'get', boom)
        g = eb.capture(buf, so, dropout=False)
    with torch.no_grad():
        out = g.replay()
        torch.cuda.synchronize(env.dev)
        _compare('same', out, eb.run(flat, so, dropout=False), B)
        first = _snapshot(out)
        # a sync-free eager run gives the same namespace
        free = eb.run(buf, so, sync_free=True, dropout=False)
        torch.cuda.synchronize(env.dev)
        _compare('sync_free', free, eb.run(flat, so, dropout=False), B)
        # other samples in the captured buffer: the same clips negated and halved
        other = (-(flat.astype(np.int32)) // 2).astype(np.int16)
        buf.copy_(torch.from_numpy(other))
        out = g.replay()
        torch.cuda.synchronize(env.dev)
        _compare('other', out, eb.run(other, so, dropout=False), B)
        # a larger eager pitch call replaces the library's scratch slots; the graph's buffers are its own
        big = [make_signal(('vad', 900 + i, 3 * 16000 + 11 * i, 16000, 0.6)) for i in range(2 * B)]
        pitch_feature_batch(np.concatenate(big), _offsets(big), 16000)
        buf.copy_(torch.from_numpy(flat))
        out = g.replay()
        torch.cuda.synchronize(env.dev)
        again = _snapshot(out)
        for k in ('pred', 'used', 'valid', 'len0', 'endpoints', 'feat', 'decision'):
            assert again[k] == first[k], k
        assert _err(np.frombuffer(again['logits'], np.float32), np.frombuffer(first['logits'], np.float32)) <= BAR
    with pytest.raises(ValueError, match='contiguous'):
        eb.capture(torch.from_numpy(np.stack([flat, flat], axis=1)).to(env.dev)[:, 0], so, dropout=False)
    with pytest.raises(TypeError, match='device tensor'):
        eb.capture(flat, so, dropout=False)


def test_mixed_rate_capture(env, monkeypatch):
    torch, nat = env.torch, env.nat
    rates = [44100, 48000, 44100, 48000]                   # two rates interleaved: the gather route
    lens = [int((0.9 + 0.1 * i) * r) + 5 for i, r in enumerate(rates)]
    clips_a = [make_signal(('vad', 750 + i, n, r, 0.6)) for i, (n, r) in enumerate(zip(lens, rates))]
    clips_b = [make_signal(('vad', 760 + i, n, r, 0.45)) for i, (n, r) in enumerate(zip(lens, rates))]
    so = _offsets(clips_a)
    buf = torch.from_numpy(np.concatenate(clips_a)).to(env.dev)
    mb = env.ens.MixedRateEnsembleBatch(env.head, env.rules)

    def boom(*a, **k):
        raise AssertionError('library scratch was asked for while the graph was being built')
    with monkeypatch.context() as m:
        m.setattr(nat.SCRATCH, 'get', boom)
        g = mb.capture(buf, so, rates, dropout=False)
    with torch.no_grad():
        for tag, clips in (('mixed_a', clips_a), ('mixed_b', clips_b)):
            flat = np.concatenate(clips)
            buf.copy_(torch.from_numpy(flat))
            out = g.replay()
            torch.cuda.synchronize(env.dev)
            _compare(tag, out, mb.run(flat, so, rates, dropout=False), 4)
        free = mb.run(buf, so, rates, sync_free=True, dropout=False)
        torch.cuda.synchronize(env.dev)
        _compare('mixed_sync_free', free, mb.run(np.concatenate(clips_b), so, rates, dropout=False), 4)
    with pytest.raises(ValueError, match='contiguous'):
        mb.capture(torch.from_numpy(np.stack([np.concatenate(clips_a)] * 2, axis=1)).to(env.dev)[:, 0], so, rates, dropout=False)
    with pytest.raises(TypeError, match='device tensor'):
        mb.capture(np.concatenate(clips_a), so, rates, dropout=False)
