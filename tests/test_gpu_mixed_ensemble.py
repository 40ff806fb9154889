"""The ensemble over mixed-rate capacity batches on the device (include/dsp_frontend.h: dsp_scatter_group_rows_batch;
features.ensemble.MixedRateCapacityEnsembleBatch; features.fit.Trainer over the mixed-rate pair):

  a  the scatter kernel against the NumPy restatement of tests/mixed_ensemble_cases.py under ``==``: B = 1 / 5 / 64 / 1500, G = 1 /
     2 / 4, rows of 4 / 36 / 40 / 256 bytes, tables of the partition's restatement (a group of pads alone, all clips in the last
     group), a column >= n_utt and a column far outside planted by hand, a sentinel-filled output with canary words behind it, a
     second run with the same bytes;
  b  the pad slots through the pitch tail (DESIGN 7.22 reads every kernel of it at n = 1): a one-rate batch, canaries behind every
     group's trim buffer and rows, ``valid`` 0 on every pad slot, every row of the batch-order results written;
  c  ONE graph replayed on five batches that differ in lengths and rate assignments against the exact-shape eager
     ``MixedRateEnsembleBatch.run(sync_free=True)``, at the bars of tests/test_gpu_capacity_layout.py's single-rate ensemble test;
     the census; the scratch monkeypatch; the metrics against tools/metrics_emul.py;
  d  the two golden clips of the real reference in one mixed capacity ensemble call;
  e  ``Trainer`` over the mixed-rate pair against the loop written out (the pattern of tests/test_gpu_fit.py), and with
     ``native_sums=True`` (the partial batch through a second graph);
  f  the refusals that need the device."""
import copy
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import capacity_cases as cc
import mixed_ensemble_cases as mec
from conftest import ROOT, normwise, record
from golden_cases import case_by_name, make_signal

sys.path.insert(0, os.path.join(ROOT, 'tools'))

import metrics_emul as me  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
BAR = 2e-5                                # logits and prob: tests/test_gpu_capacity_layout.py
INTS = ('seen', 'scored', 'correct', 'ignored', 'bad_label', 'wrong_total', 'calls')
TABLE = (44100, 48000)


@pytest.fixture(scope='module')
def env():
    import types

    import torch
    from features import _native as nat
    from features import ensemble
    nat.require_device()
    return types.SimpleNamespace(nat=nat, lib=nat.load(), torch=torch, dev=torch.device('cuda', 0), ens=ensemble)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(env, a):
    return env.torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


# ---- a: the scatter kernel alone --------------------------------------------------------------------------------------------------

def _scatter_on_device(env, rows, cols, B, row_bytes):
    """-> the uint8 [B, row_bytes] output of two runs on a sentinel-filled buffer; asserts the canary words behind it."""
    torch = env.torch
    d_rows = [_dev(env, r.reshape(-1)) for r in rows]
    d_cols = [_dev(env, c) for c in cols]
    n = B * row_bytes
    runs = []
    for _ in range(2):
        out = torch.full((n + GUARD,), mec.SENT_BYTE, dtype=torch.uint8, device=env.dev)
        env.nat.check(env.lib.dsp_scatter_group_rows_batch(_ptrs(d_rows), _ptrs(d_cols), B, len(rows), row_bytes, out.data_ptr(),
                                                           torch.cuda.current_stream(env.dev).cuda_stream))
        torch.cuda.synchronize(env.dev)
        host = _np(out)
        assert np.all(host[n:] == mec.SENT_BYTE), 'a word behind the output was written'
        runs.append(host[:n].reshape(B, row_bytes).copy())
    assert runs[0].tobytes() == runs[1].tobytes()
    return runs[0]


@pytest.mark.parametrize('B', [1, 5, 64, 1500])
def test_a_scatter_kernel(env, B):
    for G in (1, 2, 4):
        for row_bytes in (4, 36, 40, 256):
            for kind in ('seeded', 'pads_alone', 'last_group'):
                seed = 100 * B + 10 * G + row_bytes
                rates, table, cols = mec.tables(B, G, seed, kind)
                rows = mec.group_rows(B, G, row_bytes, seed)
                planted = []
                if kind == 'seeded':                     # two real slots lose their way home: a column >= n_utt, one far outside
                    real = [(g, k) for g in range(G) for k in range(B) if cols[g][k] >= 0]
                    for (g, k), col in zip(real[::max(1, len(real) // 2)][:2], (B, 2 ** 31 - 1)):
                        planted.append(int(cols[g][k]))
                        cols[g][k] = col
                want = mec.scatter_rows(rows, cols, B, row_bytes, np.full((B, row_bytes), mec.SENT_BYTE, dtype=np.uint8))
                got = _scatter_on_device(env, rows, cols, B, row_bytes)
                assert np.array_equal(got, want), (B, G, row_bytes, kind)
                for b in planted:                        # the skipped slots' rows keep the sentinel
                    assert np.all(got[b] == mec.SENT_BYTE), (B, G, row_bytes, b)
                written = np.any(got != mec.SENT_BYTE, axis=1)
                assert int(written.sum()) == B - len(planted), (B, G, row_bytes, kind)       # the groups partition the batch


# ---- the clips, the head and the rules --------------------------------------------------------------------------------------------

SEVEN_RATES = [44100, 48000, 44100, 48000, 48000, 44100, 44100]


def _seven(extra=0, seed=700):
    """DESIGN 7.17's seven clips (tests/test_gpu_mixed_capacity.py): six of 0.9 - 1.4 s interleaved 44.1 / 48 kHz and one of 0.3 s;
    ``extra`` samples are spread over the six long clips."""
    secs = [0.9, 1.0, 1.1, 1.2, 1.3, 1.4]
    add = [extra // 6 + (extra % 6 if i == 5 else 0) for i in range(6)]
    clips = [make_signal(('vad', seed + i, int(s * r) + 37 * i + 1 + add[i], r, 0.6)) for i, (s, r) in enumerate(zip(secs, SEVEN_RATES))]
    clips.append(make_signal(('vad', seed + 6, int(0.3 * 44100) + 5, 44100, 0.6)))
    return clips


def _load(env, buf, clips, tail=12345):
    flat = np.concatenate(clips)
    host = np.full(buf.numel(), tail, dtype=flat.dtype)
    host[:len(flat)] = flat
    buf.copy_(env.torch.from_numpy(host))
    return flat, cc.offsets_of([len(c) for c in clips])


def _toy_svm(env, seed, classes, n_sv=40):
    rng = np.random.default_rng(seed)
    return env.ens.PitchSVM.from_arrays(rng.standard_normal((n_sv, 5)), rng.uniform(-1, 1, n_sv), rng.uniform(-0.2, 0.2), 0.1, classes,
                                        scale=rng.uniform(0.5, 2.0, 5), center=rng.standard_normal(5))


@pytest.fixture(scope='module')
def model(env):
    """The head and the rules of tests/test_gpu_mixed_rate.py::test_ensemble_on_a_mixed_batch."""
    import types
    from features.classifier import HMRNNHead, fill_parameters
    head = HMRNNHead().to(env.dev).eval()
    fill_parameters(head, 3)
    rules = [(pair, thr, _toy_svm(env, 20 + k, pair)) for k, (pair, thr) in enumerate(env.ens.REFERENCE_RULES)]
    rules += [((2, 3), 0.9, _toy_svm(env, 30, (2, 3))), ((12, 13), 0.9, _toy_svm(env, 31, (12, 13)))]
    return types.SimpleNamespace(head=head, rules=rules)


# ---- b: the pad slots through the pitch tail ----------------------------------------------------------------------------------

def test_b_pad_slots_through_the_pitch_tail(env, model):
    torch = env.torch
    from features.pitch import N_AUX
    B = 7
    clips = _seven(seed=740)
    rates = [48000] * B                                    # the 44.1 kHz group: B pad clips of one sample
    cap = sum(len(c) for c in clips) + 77
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    flat, so = _load(env, buf, clips)
    eb = env.ens.MixedRateCapacityEnsembleBatch(TABLE, model.head, model.rules)
    arena = env.ens._MixedEnsembleArena(eb.features.prepare(B, cap, buf))
    n_trim = cap + B                                       # N + B * PAD_SAMPLES
    guarded = []
    for g in range(2):                                     # the same buffers with canary words behind them
        assert arena.trim[g].numel() == n_trim
        trim = torch.full((n_trim + GUARD,), -7.5e33, dtype=torch.float32, device=env.dev)
        feat = torch.full((B * 5 + GUARD,), -7.5e300, dtype=torch.float64, device=env.dev)
        aux = torch.full((B * N_AUX + GUARD,), 0x7fc0beef, dtype=torch.int32, device=env.dev)
        arena.trim[g], arena.feat[g], arena.aux[g] = trim[:n_trim], feat[:B * 5].view(B, 5), aux[:B * N_AUX].view(B, N_AUX)
        guarded.append((trim, feat, aux))
    arena.p_feat, arena.p_aux = _ptrs(arena.feat), _ptrs(arena.aux)
    eb._arenas[(buf.device.index, B, cap, str(buf.dtype))] = arena
    with torch.no_grad():
        res = eb.run(buf, so, rates, capacity=cap, dropout=False)
    torch.cuda.synchronize(env.dev)
    assert eb._arenas[(buf.device.index, B, cap, str(buf.dtype))] is arena
    assert int(res.status.cpu()[0]) == 0
    for g, (trim, feat, aux) in enumerate(guarded):
        assert np.all(_np(trim)[n_trim:] == np.float32(-7.5e33)), f'group {g}: a word behind the trim buffer was written'
        assert np.all(_np(feat)[B * 5:] == -7.5e300), f'group {g}: a word behind feat_g was written'
        assert np.all(_np(aux)[B * N_AUX:] == 0x7fc0beef), f'group {g}: a word behind aux_g was written'
    pads, real = _np(arena.aux[0]), _np(arena.aux[1])
    assert np.array_equal(_np(arena.mixed.dst_col[0]), np.full(B, -1)) and np.array_equal(_np(arena.mixed.dst_col[1]), np.arange(B))
    assert not pads[:, N_AUX - 1].any()                    # valid = 0 on every pad slot
    assert np.all(pads != 0x7fc0beef) and np.all(real != 0x7fc0beef)            # ... whose rows were written all the same
    assert np.isnan(_np(arena.feat[0])).all()              # a pad slot's row is NaN: it stays in its own feat_g
    # every row of the batch-order results is written: the two scatter launches again, on sentinel-filled outputs
    st = torch.cuda.current_stream(env.dev).cuda_stream
    out_feat = torch.full((B, 5), -7.5e300, dtype=torch.float64, device=env.dev)
    out_aux = torch.full((B, N_AUX), 0x7fc0beef, dtype=torch.int32, device=env.dev)
    env.nat.check(env.lib.dsp_scatter_group_rows_batch(arena.p_feat, arena.mixed.p_dst_col, B, 2, 40, out_feat.data_ptr(), st))
    env.nat.check(env.lib.dsp_scatter_group_rows_batch(arena.p_aux, arena.mixed.p_dst_col, B, 2, 4 * N_AUX, out_aux.data_ptr(), st))
    torch.cuda.synchronize(env.dev)
    assert not np.any(_np(out_feat) == -7.5e300) and not np.any(_np(out_aux) == 0x7fc0beef)
    assert _np(out_feat).tobytes() == _np(res.feat).tobytes() == _np(arena.feat[1]).tobytes()
    assert np.array_equal(_np(out_aux)[:, N_AUX - 1], _np(res.valid)) and np.array_equal(_np(res.valid), real[:, N_AUX - 1])
    assert np.isfinite(_np(res.logits)).all() and np.isfinite(_np(res.inp)).all()


# ---- c: any lengths and rates through one graph -----------------------------------------------------------------------------------

def _compare(tag, got, want, n):
    assert str(got.len0.dtype) == 'torch.int32' and got.len0.is_cuda
    assert str(got.endpoints.dtype) == 'torch.int64' and tuple(got.endpoints.shape) == (n, 2) and got.endpoints.is_cuda
    for name in ('pred', 'used', 'valid', 'len0', 'endpoints'):
        assert np.array_equal(_np(getattr(got, name)), _np(getattr(want, name))), (tag, name)
    feat_same = _np(got.feat).tobytes() == _np(want.feat).tobytes()
    if not feat_same:
        ok = _np(want.valid) != 0
        print(f'{tag}: feat differs, max abs distance on valid rows {np.max(np.abs(_np(got.feat)[ok] - _np(want.feat)[ok])):.3g}')
    assert feat_same, (tag, 'feat')
    assert _np(got.decision).tobytes() == _np(want.decision).tobytes(), (tag, 'decision')
    worst = 0.0
    for b in range(n):
        worst = max(worst, record('mixed_capacity_ensemble_inp', normwise(_np(got.inp)[:, b], _np(want.inp)[:, b])))
    e_logits = record('mixed_capacity_ensemble_logits', _err(_np(got.logits), _np(want.logits)))
    e_prob = record('mixed_capacity_ensemble_prob', _err(_np(got.prob), _np(want.prob)))
    print(f'{tag}: inp normwise {worst:.3g}, logits err {e_logits:.3g}, prob err {e_prob:.3g}, rules fired on '
          f'{int((_np(want.used) != 0).sum())} of {n} clips')
    assert worst <= 5e-5 and e_logits <= BAR and e_prob <= BAR, tag
    assert int(_np(got.n_clamped)[0]) == 0


def _snapshot(ns):
    return {k: _np(getattr(ns, k)).tobytes() for k in ('pred', 'used', 'valid', 'len0', 'endpoints', 'feat', 'decision', 'logits', 'prob', 'inp')}


def test_c_one_graph_serves_any_lengths_and_rates(env, model, monkeypatch):
    torch, nat = env.torch, env.nat
    from features.metrics import Metrics
    B = 7
    first = _seven()
    cap = (5 * sum(len(c) for c in first)) // 4            # 1.25 x the first batch
    order = [3, 0, 6, 2, 5, 1, 4]                          # DESIGN 7.17's permutation: positions 0, 1, 3, 4, 5, 6 change their rate
    filling = _seven(extra=cap - sum(len(c) for c in first), seed=720)
    vectors = [('first', first, SEVEN_RATES),
               ('permuted', [first[i] for i in order], [SEVEN_RATES[i] for i in order]),
               ('one_rate', _seven(extra=900, seed=740), [48000] * B),
               ('filling', filling, SEVEN_RATES[::-1]),
               ('first_again', first, SEVEN_RATES)]
    # (a permutation of the same clips changes an even number of positions: this one changes six, the five asked for and one more)
    assert [a != b for a, b in zip(vectors[0][2], vectors[1][2])].count(True) >= 5
    assert sum(len(c) for c in filling) == cap
    eb = env.ens.MixedRateCapacityEnsembleBatch(TABLE, model.head, model.rules)
    ref = env.ens.MixedRateEnsembleBatch(model.head, model.rules)
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    flat, so = _load(env, buf, first)
    labels = np.array([3, 0, -100, 7, 1, 12, 6], dtype=np.int64)
    lab = torch.from_numpy(labels).to(env.dev)
    m = Metrics(20, 64, env.dev)

    def boom(*a, **k):
        raise AssertionError('library scratch was asked for while the graph was being built')
    with monkeypatch.context() as mp:                      # no library scratch pointer can be recorded
        mp.setattr(nat.SCRATCH, 'get', boom)
        g = eb.capture(buf, so, SEVEN_RATES, capacity=cap, labels=lab, metrics=m, census=True, dropout=False)
    torch.cuda.synchronize(env.dev)
    assert not m.state.cpu().numpy().any()                 # capture left the block as it found it
    c = g.census
    print(f'census: {c.nodes} nodes = {c.kernels} kernels + {c.memsets} memsets + {c.memcpys} memcpys + {c.others} others, '
          f'roots {c.roots}, max fan-out {c.max_fanout}')
    assert c.is_chain and c.memsets == 0, c
    assert len(c.kernels_named('scatter_group_rows')) == 2 and not c.kernels_named('index_copy') and not c.kernels_named('index_put'), c
    assert g.sample_offsets.dtype == torch.int64 and tuple(g.sample_offsets.shape) == (B + 1,) and g.sample_offsets.is_cuda
    assert g.rates.dtype == torch.int32 and tuple(g.rates.shape) == (B,) and g.rates.is_cuda
    snaps, calls = [], []
    with torch.no_grad():
        for k, (tag, clips, rates) in enumerate(vectors):
            flat, so = _load(env, buf, clips, tail=12345 + k)
            g.sample_offsets.copy_(torch.from_numpy(so))
            g.rates.copy_(torch.from_numpy(np.asarray(rates, dtype=np.int32)))
            lab_k = np.roll(labels, k)
            lab.copy_(torch.from_numpy(lab_k))
            out = g.replay()
            torch.cuda.synchronize(env.dev)
            assert int(g.status.cpu()[0]) == 0, tag
            snaps.append(_snapshot(out))
            calls.append((_np(out.logits).copy(), _np(out.pred).copy(), lab_k))
            want = ref.run(torch.from_numpy(flat).to(env.dev), so, rates, sync_free=True, dropout=False)
            torch.cuda.synchronize(env.dev)
            _compare(tag, out, want, B)
            # the eager form: the same launch sequence, the replay's namespace
            free = eb.run(buf, so, rates, capacity=cap, dropout=False)
            torch.cuda.synchronize(env.dev)
            assert int(free.status.cpu()[0]) == 0
            again = _snapshot(free)
            for name in ('pred', 'used', 'valid', 'len0', 'endpoints', 'feat', 'decision', 'inp'):
                assert again[name] == snaps[k][name], (tag, name)
            for name in ('logits', 'prob'):
                assert _err(np.frombuffer(again[name], np.float32), np.frombuffer(snaps[k][name], np.float32)) <= BAR, (tag, name)
    for name in ('pred', 'used', 'valid', 'len0', 'endpoints', 'feat', 'decision', 'inp'):
        assert snaps[4][name] == snaps[0][name], name        # back on the first vector: the first replay's bytes
    for name in ('logits', 'prob'):
        assert _err(np.frombuffer(snaps[4][name], np.float32), np.frombuffer(snaps[0][name], np.float32)) <= BAR, name
    # the metrics block after the five replays: tools/metrics_emul.py on the downloaded logits / pred, in every integer
    st = me.State(20, 64)
    for logits, pred, lab_k in calls:
        st.update(logits.astype(np.float64), lab_k, pred)
    r, want = m.result(), st.result()
    for name in INTS:
        assert getattr(r, name) == getattr(want, name), name
    assert np.array_equal(r.confusion, want.confusion) and np.array_equal(r.wrong, want.wrong)
    assert abs(r.loss - want.loss) <= 1e-6, (r.loss, want.loss)
    assert (r.seen, r.calls) == (5 * B, 5)


# ---- d: the real reference's rows -----------------------------------------------------------------------------------------------

def test_d_two_rates_against_the_reference(env, model, golden):
    torch = env.torch
    from features.model_glue import MixedRateFeatureBatch
    from oracle import dsp_oracle
    names, rates = ['model_feat_48k', 'model_feat_44k'], [48000, 44100]
    clips = [make_signal(case_by_name(n)['sig']) for n in names]
    cap = sum(len(c) for c in clips) + 1000
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    flat, so = _load(env, buf, clips)
    eb = env.ens.MixedRateCapacityEnsembleBatch(TABLE, model.head, model.rules)
    with torch.no_grad():
        res = eb.run(buf, so, rates, capacity=cap, dropout=False)
    torch.cuda.synchronize(env.dev)
    got, len0, ends = _np(res.inp), _np(res.len0), _np(res.endpoints)
    assert int(res.status.cpu()[0]) == 0 and got.shape == (200, 2, 39)
    for b, name in enumerate(names):
        n = int(golden[f'{name}/len'][0])
        assert len0[b] == n
        for key, col in (('m0', 0), ('m1', 13), ('m2', 26)):
            err = record(f'mixed_capacity_ensemble_{name}_{key}', normwise(got[:n, b, col:col + 13], golden[f'{name}/{key}'][:n]))
            assert err <= 1e-4, (name, key, err)
        assert not got[n:, b].any()
        # the endpoints: the restated reference's (oracle/dsp_oracle.py: endpoint.py:34-66), sample for sample
        assert tuple(int(v) for v in ends[b]) == tuple(dsp_oracle.basic_endpoint_detection(clips[b], rates[b])), name
    _, elen, eends = MixedRateFeatureBatch().run(torch.from_numpy(flat).to(env.dev), so, rates)
    assert np.array_equal(len0, elen) and np.array_equal(ends, eends)


# ---- e: Trainer against the loop written out ------------------------------------------------------------------------------------

B_FIT, N_CLASSES, LR0, EPOCHS = 5, 20, 1e-3, 3


def _head(dev):
    import torch
    from features import classifier as C
    torch.manual_seed(0)
    head = C.HMRNNHead().train()
    C.fill_parameters(head, 3)
    for m in head.modules():
        if isinstance(m, C._DynEnc):
            m.gru.dropout = 0.0
    return head.to(dev)


def _data():
    """12 training and 7 validation clips of 0.5 - 0.8 s, rates alternating 44.1 / 48 kHz; the label skew of tests/test_gpu_fit.py."""
    def clip(i, seed):
        rate = TABLE[i % 2]
        return make_signal(('vad', seed + i, int((0.5 + 0.06 * (i % 6)) * rate) + 3 * i, rate, 0.6)), rate
    train, val = [clip(i, 1200) for i in range(12)], [clip(i + 1, 1300) for i in range(7)]
    rng = np.random.default_rng(12)
    tlab, vlab = rng.integers(0, N_CLASSES, 12).astype(np.int64), rng.integers(0, N_CLASSES, 7).astype(np.int64)
    tlab[[0, 1, 2, 4, 5, 7, 8, 10, 11]] = 3
    vlab[[0, 2, 3, 4, 6]] = 3
    return (train, tlab), (val, vlab)


def _same_bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _hand_loop(env, train, val, head, cap, epochs=EPOCHS, **train_kw):
    """model.py:219-240 with 137-150 and 162-187 written out for mixed-rate data: eager ``MixedRateTrainBatch.run(capacity=)`` steps with
    ``DeviceAdam.step()``, the exact-shape eager ``MixedRateEnsembleBatch.run(sync_free=True)``, NumPy metrics."""
    torch = env.torch
    from features.optim import DeviceAdam
    from features.train import MixedRateTrainBatch
    tb, eb = MixedRateTrainBatch(TABLE, head), env.ens.MixedRateEnsembleBatch(head, [])
    opt = DeviceAdam(list(head.parameters()), lr=LR0)
    jitter_rng = random.Random(7)
    (tfeat, tlab), (vfeat, vlab) = train, val
    torder, vorder = list(range(len(tfeat))), list(range(len(vfeat)))
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    prev_acc, lr, early_stop = 0, LR0, 3
    out = []
    for epoch in range(epochs):
        opt.reset()
        opt.set_lr(lr)
        head.train()
        random.Random(0).shuffle(torder)
        st = me.State(N_CLASSES, 64)
        for s in range(0, len(torder), B_FIT):
            idx = torder[s:s + B_FIT]
            clips, rates = [tfeat[i][0] for i in idx], [tfeat[i][1] for i in idx]
            jitter = tb.draw_jitter(rates, jitter_rng)
            for p in opt.params:
                p.grad = None
            _, so = _load(env, buf, clips, tail=0)
            res = tb.run(buf, so, rates, tlab[idx], jitter, capacity=cap, loss='native', dropout=False, **train_kw)
            res.loss.backward()
            opt.step()
            st.update(res.logits.detach().cpu().numpy().astype(np.float64), tlab[idx])
        train_res = st.result()
        head.eval()
        random.Random(0).shuffle(vorder)
        sv = me.State(N_CLASSES, 64)
        with torch.no_grad():
            for s in range(0, len(vorder), B_FIT):
                idx = vorder[s:s + B_FIT]
                clips, rates = [vfeat[i][0] for i in idx], [vfeat[i][1] for i in idx]
                res = eb.run(torch.from_numpy(np.concatenate(clips)).to(env.dev), cc.offsets_of([len(c) for c in clips]), rates,
                             sync_free=True, dropout=False)
                sv.update(res.logits.cpu().numpy().astype(np.float64), vlab[idx], res.pred.cpu().numpy())
        val_res = sv.result()
        acc, lr_now = val_res.accuracy, lr
        improved, stop = acc > prev_acc, False
        if improved:
            prev_acc = acc
            lr *= 0.8
        else:
            early_stop -= 1
            lr *= 0.5
            stop = not early_stop
        torch.cuda.synchronize(env.dev)
        out.append((lr_now, train_res, val_res, improved, [p.detach().clone() for p in head.parameters()]))
        if stop:
            break
        head.adjust_param()
        head.train()
    return out


def _same_result(got, want, tag):
    for name in ('seen', 'scored', 'correct', 'ignored', 'bad_label', 'wrong_total'):
        assert getattr(got, name) == getattr(want, name), (tag, name)
    assert got.accuracy == want.accuracy, tag
    assert np.array_equal(got.confusion, want.confusion) and np.array_equal(got.wrong, want.wrong), tag
    print(f'{tag}: loss {got.loss:.9f} against {want.loss:.9f}')
    assert abs(got.loss - want.loss) <= 1e-6, (tag, got.loss, want.loss)


def test_e_trainer_against_the_loop_written_out(env):
    torch = env.torch
    from features.fit import Trainer
    from features.optim import DeviceAdam
    from features.train import MixedRateTrainBatch
    train, val = _data()
    cap = int(sum(sorted((len(c) for c, _ in train[0] + val[0]), reverse=True)[:B_FIT]))
    head = _head(env.dev)
    twin = copy.deepcopy(head)
    want = _hand_loop(env, train, val, twin, cap)

    tb, eb = MixedRateTrainBatch(TABLE, head), env.ens.MixedRateCapacityEnsembleBatch(TABLE, head, [])
    opt = DeviceAdam(list(head.parameters()), lr=LR0)
    trainer = Trainer(tb, eb, opt, N_CLASSES, wrong_capacity=64, head_kwargs={'dropout': False}, jitter_rng=random.Random(7))
    snaps, improved_at = [], []

    def on_epoch(entry):
        torch.cuda.synchronize(env.dev)
        snaps.append([p.detach().clone() for p in head.parameters()])
    hist = trainer.fit(train, val, LR0, epochs=EPOCHS, batch_size=B_FIT, capacity=cap,
                       on_improve=lambda epoch, acc: improved_at.append(epoch), on_epoch=on_epoch)
    assert len(hist) == len(want) == len(snaps)
    names = [n for n, _ in head.named_parameters()]
    for k, (entry, (lr, train_res, val_res, improved, params)) in enumerate(zip(hist, want)):
        assert float(entry.lr).hex() == float(lr).hex() and entry.improved == improved, k
        _same_result(entry.train, train_res, f'train epoch {k}')
        _same_result(entry.val, val_res, f'val epoch {k}')
        assert (entry.train.seen, entry.train.calls, entry.val.seen, entry.val.calls) == (12, 3, 7, 2)
        bad = [n for n, p, q in zip(names, snaps[k], params) if not _same_bits(p, q)]
        assert not bad, (k, bad)
    assert improved_at == [k for k, w in enumerate(want) if w[3]]
    assert head.training and head.enc2.a == twin.enc2.a
    assert any(not _same_bits(p, q) for p, q in zip(snaps[0], snaps[-1]))
    # a clip at a rate outside the table: refused on the host, before any launch
    with pytest.raises(ValueError, match='22050 Hz'):
        trainer.fit(([(train[0][0][0], 22050)], train[1][:1]), val, LR0, epochs=1, batch_size=B_FIT)


def test_e_trainer_with_native_sums_records_the_partial_batch_too(env):
    """``fit(native_sums=True)`` on mixed data: the full batches through one training graph and the partial batch of 2 through a second
    one (both recorded anew after ``adjust_param``); every parameter after each of two epochs equals the loop written out."""
    torch = env.torch
    from features.fit import Trainer
    from features.optim import DeviceAdam
    from features.train import MixedRateTrainBatch
    train, val = _data()
    cap = int(sum(sorted((len(c) for c, _ in train[0] + val[0]), reverse=True)[:B_FIT]))
    head = _head(env.dev)
    twin = copy.deepcopy(head)
    want = _hand_loop(env, train, val, twin, cap, epochs=2, native_sums=True)
    tb, eb = MixedRateTrainBatch(TABLE, head), env.ens.MixedRateCapacityEnsembleBatch(TABLE, head, [])
    trainer = Trainer(tb, eb, DeviceAdam(list(head.parameters()), lr=LR0), N_CLASSES, wrong_capacity=64, head_kwargs={'dropout': False},
                      jitter_rng=random.Random(7))
    snaps = []

    def on_epoch(entry):
        torch.cuda.synchronize(env.dev)
        snaps.append([p.detach().clone() for p in head.parameters()])
    hist = trainer.fit(train, val, LR0, epochs=2, batch_size=B_FIT, capacity=cap, on_epoch=on_epoch, native_sums=True)
    assert len(hist) == len(want) == len(snaps) == 2
    names = [n for n, _ in head.named_parameters()]
    for k, (entry, (lr, train_res, val_res, improved, params)) in enumerate(zip(hist, want)):
        assert float(entry.lr).hex() == float(lr).hex() and entry.improved == improved, k
        _same_result(entry.train, train_res, f'native_sums train epoch {k}')
        _same_result(entry.val, val_res, f'native_sums val epoch {k}')
        assert (entry.train.seen, entry.train.calls, entry.val.seen, entry.val.calls) == (12, 3, 7, 2)
        bad = [n for n, p, q in zip(names, snaps[k], params) if not _same_bits(p, q)]
        assert not bad, (k, bad)
    assert [e.train_graphs for e in hist] == [2, 4]            # two training graphs per epoch: sizes 5 and 2


# ---- f: the refusals that need the device -----------------------------------------------------------------------------------------

def test_f_refusals(env, model):
    torch = env.torch
    clips = _seven()[:3]
    rates = SEVEN_RATES[:3]
    cap = sum(len(c) for c in clips) + 10
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    _, so = _load(env, buf, clips)
    eb = env.ens.MixedRateCapacityEnsembleBatch(TABLE, model.head, model.rules)
    for call in (eb.run, eb.capture):
        with pytest.raises(ValueError, match='exactly that many'):
            call(buf, so, rates, capacity=cap + 1, dropout=False)            # waves of the wrong length
        with pytest.raises(ValueError, match='contiguous'):
            call(torch.zeros(2 * cap, dtype=torch.int16, device=env.dev)[::2], so, rates, capacity=cap, dropout=False)
        with pytest.raises(ValueError, match=r'rates must be \[3\]'):
            call(buf, so, rates[:2], capacity=cap, dropout=False)
    with pytest.raises(TypeError, match='device tensor'):
        eb.run(np.zeros(cap, dtype=np.int16), so, rates, capacity=cap, dropout=False)
    with pytest.raises(TypeError):
        eb.run(buf.to(torch.float64), so, rates, capacity=cap, dropout=False)
    plain = env.ens.MixedRateCapacityEnsembleBatch(TABLE, lambda inp, len0: torch.zeros(3, 20, device=env.dev), [])
    with pytest.raises(TypeError, match='device_len'):
        plain.run(buf, so, rates, capacity=cap)                               # a head without device_len
    # a rate outside the table is the device's to report: bit 4, and every result stays defined
    with torch.no_grad():
        res = eb.run(buf, so, [44100, 22050, 44100], capacity=cap, dropout=False)
    torch.cuda.synchronize(env.dev)
    assert int(res.status.cpu()[0]) == 16 and np.isfinite(_np(res.logits)).all() and np.isfinite(_np(res.inp)).all()
