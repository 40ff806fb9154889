"""Recorded training steps at batch sizes OUTSIDE ``CAPTURE_VERIFIED`` (features/train.py): with ``native_sums=True`` among the
head's keywords and ``loss='native'`` the step launches no reduction of torch's, ``capture`` serves any size and checks the
recorded graph's census instead of a table.

The recipe of tests/test_gpu_adv.py / tests/test_gpu_metrics.py: three replays -- new clips, labels and jitter each, ``set_lr``
before the third -- equal three eager ``run`` steps in every bit of every loss, parameter and Adam moment, with the ``DeviceAdam``
step recorded, ``loss='native'``, the metrics block and the dropouts drawn by a ``DeviceRng``:

  * the five heads at B in {3, 17, 64, 100} and ``AdvHRNNHead`` at {3, 17}: none of these sizes is in the tables (asserted);
  * ``TransformerHead`` at B = 17 through a capacity graph with a new length vector per step;
  * ``HMRNNHead`` at B = 17 through ``MixedRateTrainBatch`` with new lengths and rate assignments per step;
  * the census of every recorded step: a chain (1 root, fan-out 1), no memset node of more than 4 bytes, no ``reduce_kernel`` of
    torch's (``at::native::reduce_kernel``; the library's own ``rows_wgrad_reduce_kernel`` and the like are fixed-order sums);
  * without ``native_sums`` (or with the torch loss) the same call still raises the ``CAPTURE_VERIFIED`` error;
  * ``Trainer.fit(batch_size=6, native_sums=True)`` over 15 short clips -- two full batches and a partial one of 3 per epoch, each
    size through a capacity graph of its own -- equals the loop written out with eager steps in every parameter after each of
    two epochs, and reports the two graphs each epoch recorded."""
import copy
import random

import numpy as np
import pytest

import capacity_cases as cc
import mixed_capacity_cases as mc
from ensemble_cases import make_clips
from golden_cases import make_signal

pytestmark = pytest.mark.gpu

SEED = 20240607
SIZES = (3, 17, 64, 100)
HEADS = ('RNNHead', 'HRNNHead', 'HRNNAttHead', 'TransformerHead', 'HMRNNHead')
LRS = (1e-3, 1e-3, 3e-4)


def _head(kind, dev):
    """In training mode, every dropout as the class builds it."""
    import torch
    from features import classifier as C
    torch.manual_seed(0)
    head = getattr(C, kind)().train()
    C.fill_parameters(head, 3)
    return head.to(dev)


def _kw(kind, rng):
    kw = {'rng': rng, 'native_sums': True}
    if kind != 'RNNHead':
        kw['dropout'] = True
    return kw


def _bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


def _cut(stored, B, k):
    """Batch k of B clips: prefixes of the stored clips in an order and at lengths that change with k."""
    out = []
    for i in range(B):
        c = stored[(i + 3 * k) % len(stored)]
        frac = (0.60 + 0.05 * ((3 * i) % 5)) if k == 0 else (0.55 + 0.05 * ((7 * i + 3 * k) % 5))
        out.append(c[:int(frac * len(c)) + 7 * i + k])
    return out


def _assert_clean(census, what):
    print(f'{what}: {census.kernels} kernels, {census.memsets} memsets (widest {census.widest_memset_bytes} B), {census.memcpys} memcpys, '
          f'{census.others} others, {census.roots} root(s), fan-out {census.max_fanout}')
    assert census is not None and census.is_chain and (census.roots, census.max_fanout) == (1, 1), (what, census)
    assert census.wide_memsets == 0 and census.widest_memset_bytes <= 4, (what, census)
    assert census.torch_reductions() == () and census.kernels > 0 and len(census.kernel_names) == census.kernels, (what, census)


def _assert_same_state(head_a, opt_a, head_b, opt_b):
    names = [n for n, _ in head_a.named_parameters()]
    bad = [n for n, p, q in zip(names, head_a.parameters(), head_b.parameters()) if not _bits(p, q)]
    bad += [n + '.exp_avg' for n, p, q in zip(names, opt_a.exp_avg, opt_b.exp_avg) if not _bits(p, q)]
    bad += [n + '.exp_avg_sq' for n, p, q in zip(names, opt_a.exp_avg_sq, opt_b.exp_avg_sq) if not _bits(p, q)]
    assert not bad, bad
    assert opt_a.device_state() == opt_b.device_state() and opt_a.device_state()[0] == 3


def test_sizes_are_outside_the_tables():
    from features.train import ADV_CAPTURE_VERIFIED, CAPTURE_VERIFIED
    assert all(B not in CAPTURE_VERIFIED[kind] for kind in HEADS for B in SIZES + (6,))
    assert all(B not in ADV_CAPTURE_VERIFIED['AdvHRNNHead'] for B in (3, 17))
    assert CAPTURE_VERIFIED == {'RNNHead': (32, 512), 'HRNNHead': (32, 512), 'HRNNAttHead': (32, 512), 'TransformerHead': (32, 512),
                                'HMRNNHead': (5, 32, 512)} and ADV_CAPTURE_VERIFIED == {'AdvHRNNHead': (32, 512)}


def _content(tb, B, stored, capacity):
    """Three batches.  Exact shape: the same clip lengths, other samples; capacity: other clips and lengths each."""
    labels = np.random.default_rng(B).integers(0, 20, B).astype(np.int64)
    if capacity:
        batches = [_cut(stored, B, k) for k in range(3)]
        return [(np.concatenate(c), _offsets(c), (labels + 7 * k) % 20, tb.draw_jitter(B, random.Random(B + k))) for k, c in enumerate(batches)]
    clips = [stored[i % len(stored)] for i in range(B)]
    flat = np.concatenate(clips).astype(np.int32)
    waves = [flat, -flat // 2, (3 * flat) // 4]
    return [(waves[k].astype(np.int16), _offsets(clips), (labels + 7 * k) % 20, tb.draw_jitter(B, random.Random(B + k))) for k in range(3)]


def _three_steps(kind, B, capacity=False):
    import torch
    from features.dropout import DeviceRng
    from features.metrics import Metrics
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    head = _head(kind, dev)
    twin = copy.deepcopy(head)
    tb, tb_twin = TrainBatch(rate, head), TrainBatch(rate, twin)
    content = _content(tb, B, stored, capacity)
    cap = (5 * max(len(c[0]) for c in content)) // 4 if capacity else None
    rng, rng_twin = DeviceRng(SEED, dev), DeviceRng(SEED, dev)
    m, m_twin = Metrics(20, 8), Metrics(20, 8)
    opt = DeviceAdam(list(head.parameters()), lr=LRS[0])
    flat, so0, l0, j0 = content[0]
    buf = torch.zeros(cap if capacity else len(flat), dtype=torch.int16, device=dev)
    buf[:len(flat)].copy_(torch.from_numpy(flat))
    lab, jit = torch.from_numpy(l0).to(dev), torch.from_numpy(j0).to(dev)
    extra = dict(capacity=cap) if capacity else {}
    with pytest.raises(NotImplementedError, match='CAPTURE_VERIFIED'):                # without the switch: the refusal as it was
        tb.capture(buf, so0, lab, jit, optimizer=opt, loss='native', metrics=m, **extra, **{k: v for k, v in _kw(kind, rng).items() if k != 'native_sums'})
    with pytest.raises(NotImplementedError, match='CAPTURE_VERIFIED'):                # ... and with torch's loss, which reduces
        tb.capture(buf, so0, lab, jit, optimizer=opt, **extra, **_kw(kind, rng))
    g = tb.capture(buf, so0, lab, jit, optimizer=opt, loss='native', metrics=m, **extra, **_kw(kind, rng))
    torch.cuda.synchronize(dev)
    assert rng.state_dict() == {'seed': SEED, 'step': 0} and opt.device_state()[0] == 0 and not m.state.cpu().numpy().any()
    _assert_clean(g.census, f'{kind} B={B}{" capacity" if capacity else ""}')
    losses = []
    for k, (flat, so, l, j) in enumerate(content):
        if LRS[k] != opt.lr:
            opt.set_lr(LRS[k])
        if capacity:
            buf.fill_(12345)
            g.sample_offsets.copy_(torch.from_numpy(so))
        buf[:len(flat)].copy_(torch.from_numpy(flat))
        lab.copy_(torch.from_numpy(l))
        jit.copy_(torch.from_numpy(j))
        losses.append(g.replay().loss.clone())
    torch.cuda.synchronize(dev)
    opt_twin = DeviceAdam(list(twin.parameters()), lr=LRS[0])
    want = []
    for k, (flat, so, l, j) in enumerate(content):
        if LRS[k] != opt_twin.lr:
            opt_twin.set_lr(LRS[k])
        for p in opt_twin.params:
            p.grad = None
        out = tb_twin.run(torch.from_numpy(flat).to(dev), so, torch.from_numpy(l).to(dev), torch.from_numpy(j).to(dev), loss='native',
                          metrics=m_twin, **_kw(kind, rng_twin))
        out.loss.backward()
        opt_twin.step()
        want.append(out.loss.detach().clone())
    torch.cuda.synchronize(dev)
    differing = [k for k in range(3) if not _bits(losses[k], want[k])]
    print(f'{kind} B={B}: losses {[float(x) for x in losses]}, differing from the eager steps in bits: {differing}')
    assert not differing
    assert not _bits(losses[0], losses[1])                                            # the replays saw the new content
    _assert_same_state(head, opt, twin, opt_twin)
    assert rng_twin.state_dict() == rng.state_dict() == {'seed': SEED, 'step': 3}
    assert torch.equal(m.state, m_twin.state) and m.result().seen == 3 * B


@pytest.mark.parametrize('B', SIZES)
@pytest.mark.parametrize('kind', HEADS)
def test_three_replays_equal_three_eager_steps(kind, B):
    _three_steps(kind, B)


def test_capacity_graph_with_new_length_vectors():
    _three_steps('TransformerHead', 17, capacity=True)


@pytest.mark.parametrize('B', [3, 17])
def test_adversarial_head(B):
    import torch
    from features import classifier as C
    from features.dropout import DeviceRng
    from features.metrics import Metrics
    from features.optim import DeviceAdam
    from features.train import AdvTrainBatch
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    head = _head('AdvHRNNHead', dev)
    head.device_gamma()
    twin = copy.deepcopy(head)
    tb, tb_twin = AdvTrainBatch(rate, head), AdvTrainBatch(rate, twin)
    content = _content(tb, B, stored, False)
    speakers = [np.random.default_rng(B + k).integers(0, 35, B).astype(np.int64) for k in range(3)]
    rng, rng_twin = DeviceRng(SEED, dev), DeviceRng(SEED, dev)
    m, ms, m_twin, ms_twin = Metrics(20, 8), Metrics(35, 8), Metrics(20, 8), Metrics(35, 8)
    opt = DeviceAdam(list(head.parameters()), lr=LRS[0])
    flat, so, l0, j0 = content[0]
    buf, lab, jit, spk = (torch.from_numpy(a).to(dev) for a in (flat, l0, j0, speakers[0]))
    kw = dict(loss='native', native_disc=True, dropout=True, native_sums=True)
    with pytest.raises(NotImplementedError, match='CAPTURE_VERIFIED'):
        tb.capture(buf, so, lab, spk, jit, optimizer=opt, loss='native', native_disc=True, dropout=True, rng=rng)
    g = tb.capture(buf, so, lab, spk, jit, optimizer=opt, metrics=m, speaker_metrics=ms, rng=rng, **kw)
    torch.cuda.synchronize(dev)
    _assert_clean(g.census, f'AdvHRNNHead B={B}')
    got = []
    for k, (flat, _, l, j) in enumerate(content):
        if k == 2:
            opt.set_lr(LRS[2])
            head.device_gamma(0.05)
        for t, a in ((buf, flat), (lab, l), (jit, j), (spk, speakers[k])):
            t.copy_(torch.from_numpy(a))
        r = g.replay()
        got.append((r.loss.clone(), r.loss_label.clone(), r.loss_speaker.clone()))
    torch.cuda.synchronize(dev)
    opt_twin = DeviceAdam(list(twin.parameters()), lr=LRS[0])
    want = []
    for k, (flat, _, l, j) in enumerate(content):
        if k == 2:
            opt_twin.set_lr(LRS[2])
            twin.device_gamma(0.05)
        for p in opt_twin.params:
            p.grad = None
        t = lambda a: torch.from_numpy(a).to(dev)
        out = tb_twin.run(t(flat), so, t(l), t(speakers[k]), t(j), metrics=m_twin, speaker_metrics=ms_twin, rng=rng_twin, **kw)
        AdvTrainBatch.backward(out)
        opt_twin.step()
        want.append((out.loss.detach().clone(), out.loss_label.detach().clone(), out.loss_speaker.detach().clone()))
    torch.cuda.synchronize(dev)
    differing = [(k, i) for k in range(3) for i in range(3) if not _bits(got[k][i], want[k][i])]
    print(f'AdvHRNNHead B={B}: losses {[[float(x) for x in row] for row in got]}, differing from the eager steps in bits: {differing}')
    assert not differing
    _assert_same_state(head, opt, twin, opt_twin)
    assert torch.equal(m.state, m_twin.state) and torch.equal(ms.state, ms_twin.state)
    assert isinstance(head, C.AdvHRNNHead)


def test_mixed_rate_batch():
    """``MixedRateTrainBatch`` over ``HMRNNHead`` at B = 17: new clips, lengths, rate assignments, labels, jitter per step."""
    import torch
    from features.dropout import DeviceRng
    from features.metrics import Metrics
    from features.optim import DeviceAdam
    from features.train import MixedRateTrainBatch
    kind, B = 'HMRNNHead', 17
    dev = torch.device('cuda', 0)
    head = _head(kind, dev)
    twin = copy.deepcopy(head)
    tb, tb_twin = MixedRateTrainBatch((44100, 48000), head), MixedRateTrainBatch((44100, 48000), twin)
    content = []
    for k in range(3):
        r = np.random.default_rng(100 * B + k)
        rates = mc.rate_vector(B, (44100, 48000), 7 * B + k)
        clips = [make_signal(('vad', 900 + 40 * k + i, int(r.uniform(0.5, 0.8) * rt) + i, int(rt), 0.6)) for i, rt in enumerate(rates)]
        content.append((clips, rates, r.integers(0, 20, B).astype(np.int64), tb.draw_jitter(rates, random.Random(B + k))))
    cap = (11 * max(sum(len(c) for c in b[0]) for b in content)) // 10

    def load(buf, clips, tail):
        flat = np.concatenate(clips)
        host = np.full(buf.numel(), tail, dtype=flat.dtype)
        host[:len(flat)] = flat
        buf.copy_(torch.from_numpy(host))
        return cc.offsets_of([len(c) for c in clips])
    rng, rng_twin = DeviceRng(SEED, dev), DeviceRng(SEED, dev)
    m, m_twin = Metrics(20, 8), Metrics(20, 8)
    opt = DeviceAdam(list(head.parameters()), lr=LRS[0])
    buf = torch.zeros(cap, dtype=torch.int16, device=dev)
    so0 = load(buf, content[0][0], 12345)
    lab, jit = torch.from_numpy(content[0][2]).to(dev), torch.from_numpy(content[0][3]).to(dev)
    with pytest.raises(NotImplementedError, match='CAPTURE_VERIFIED'):
        tb.capture(buf, so0, content[0][1], lab, jit, optimizer=opt, capacity=cap, loss='native', dropout=True, rng=rng)
    g = tb.capture(buf, so0, content[0][1], lab, jit, optimizer=opt, capacity=cap, loss='native', metrics=m, **_kw(kind, rng))
    torch.cuda.synchronize(dev)
    _assert_clean(g.census, f'MixedRateTrainBatch {kind} B={B}')
    losses, offs = [], []
    for k, (clips, rates, l, j) in enumerate(content):
        offs.append(load(buf, clips, 77 + k))
        g.sample_offsets.copy_(torch.from_numpy(offs[-1]))
        g.rates.copy_(torch.from_numpy(rates))
        lab.copy_(torch.from_numpy(l))
        g.jitter.copy_(torch.from_numpy(j))
        if LRS[k] != opt.lr:
            opt.set_lr(LRS[k])
        losses.append(g.replay().loss.clone())
    torch.cuda.synchronize(dev)
    assert int(g.status.cpu()[0]) == 0
    opt_twin = DeviceAdam(list(twin.parameters()), lr=LRS[0])
    want = []
    for k, (clips, rates, l, j) in enumerate(content):
        if LRS[k] != opt_twin.lr:
            opt_twin.set_lr(LRS[k])
        load(buf, clips, 77 + k)
        for p in opt_twin.params:
            p.grad = None
        out = tb_twin.run(buf, offs[k], rates, torch.from_numpy(l).to(dev), torch.from_numpy(j).to(dev), capacity=cap, loss='native',
                          metrics=m_twin, **_kw(kind, rng_twin))
        out.loss.backward()
        opt_twin.step()
        want.append(out.loss.detach().clone())
    torch.cuda.synchronize(dev)
    differing = [k for k in range(3) if not _bits(losses[k], want[k])]
    print(f'mixed-rate {kind} B={B}: losses {[float(x) for x in losses]}, differing from the eager steps in bits: {differing}')
    assert not differing
    _assert_same_state(head, opt, twin, opt_twin)
    assert torch.equal(m.state, m_twin.state)


def test_trainer_records_at_any_batch_size():
    """``Trainer.fit(batch_size=6, native_sums=True)``: 15 clips are two full batches and a partial one of 3; every parameter after
    each of two epochs equals the loop written out with eager exact-shape steps; two graphs are recorded per epoch (the head's
    ``adjust_param`` makes the second epoch record anew)."""
    import torch
    from features.ensemble import EnsembleBatch
    from features.fit import Trainer
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    B, N, LR0, EPOCHS = 6, 15, 1e-3, 2
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    short = lambda i, f: stored[i % len(stored)][:int(f * len(stored[i % len(stored)])) + 3 * i]
    tclips = [short(i, 0.35 + 0.04 * (i % 5)) for i in range(N)]
    vclips = [short(i + 5, 0.33 + 0.05 * (i % 4)) for i in range(7)]
    r = np.random.default_rng(12)
    tlab, vlab = r.integers(0, 20, N).astype(np.int64), r.integers(0, 20, 7).astype(np.int64)
    tlab[::2] = 3
    vlab[::2] = 3
    head = _head('HMRNNHead', dev)
    for mod in head.modules():
        if hasattr(mod, 'gru'):
            mod.gru.dropout = 0.0
    twin = copy.deepcopy(head)

    # the loop written out: model.py:219-240 with eager steps
    tb2 = TrainBatch(rate, twin)
    opt2 = DeviceAdam(list(twin.parameters()), lr=LR0)
    jr = random.Random(7)
    order, vorder = list(range(N)), list(range(7))
    prev, lr, want = 0, LR0, []
    eb2 = EnsembleBatch(rate, twin, [])
    for epoch in range(EPOCHS):
        opt2.reset()
        opt2.set_lr(lr)
        twin.train()
        random.Random(0).shuffle(order)
        for s in range(0, N, B):
            idx = order[s:s + B]
            clips = [tclips[i] for i in idx]
            jitter = tb2.draw_jitter(len(idx), jr)
            for p in opt2.params:
                p.grad = None
            res = tb2.run(np.concatenate(clips), _offsets(clips), tlab[idx], jitter, loss='native', dropout=False, native_sums=True)
            res.loss.backward()
            opt2.step()
        twin.eval()
        random.Random(0).shuffle(vorder)
        correct = 0
        with torch.no_grad():
            for s in range(0, 7, B):
                idx = vorder[s:s + B]
                clips = [vclips[i] for i in idx]
                out = eb2.run(np.concatenate(clips), _offsets(clips), sync_free=True, dropout=False)
                correct += int((out.pred.cpu().numpy() == vlab[idx]).sum())
        acc = correct / 7
        if acc > prev:
            prev, lr = acc, lr * 0.8
        else:
            lr *= 0.5
        torch.cuda.synchronize(dev)
        want.append([p.detach().clone() for p in twin.parameters()])
        twin.adjust_param()
        twin.train()

    tb, eb = TrainBatch(rate, head), EnsembleBatch(rate, head, [])
    opt = DeviceAdam(list(head.parameters()), lr=LR0)
    trainer = Trainer(tb, eb, opt, 20, wrong_capacity=64, head_kwargs={'dropout': False}, jitter_rng=random.Random(7))
    snaps = []

    def on_epoch(entry):
        torch.cuda.synchronize(dev)
        snaps.append([p.detach().clone() for p in head.parameters()])
    feat = lambda clips: [(c, rate) for c in clips]
    hist = trainer.fit((feat(tclips), tlab), (feat(vclips), vlab), LR0, epochs=EPOCHS, batch_size=B, on_epoch=on_epoch, native_sums=True)
    assert len(hist) == len(snaps) == EPOCHS
    names = [n for n, _ in head.named_parameters()]
    for k in range(EPOCHS):
        bad = [n for n, p, q in zip(names, snaps[k], want[k]) if not _bits(p, q)]
        assert not bad, (k, bad)
        assert (hist[k].train.seen, hist[k].train.calls) == (N, 3)
    assert [e.train_graphs for e in hist] == [2, 4]                                   # two graphs per epoch: sizes 6 and 3
    assert any(not _bits(p, q) for p, q in zip(snaps[0], snaps[1]))
    with torch.no_grad(), pytest.raises(RuntimeError, match='native_sums=True cannot run'):   # validation is forward only
        eb.run(np.concatenate(vclips[:3]), _offsets(vclips[:3]), sync_free=True, dropout=False, native_sums=True)
