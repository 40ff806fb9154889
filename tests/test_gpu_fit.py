"""``features.fit.Trainer`` (model.py:219-240 on the device) and ``DeviceAdam.reset``.

``Trainer``: ``HMRNNHead``, B = 5, 12 clips for training (two batches through the recorded capacity graph and a partial batch of
2 through the eager exact-shape step), 7 for validation (one recorded batch, a partial batch of 2), 2 epochs, dropout off --
against the same loop written out here with the eager ``TrainBatch.run``, ``loss.backward()``, ``DeviceAdam.step()``, the eager
sync-free ``EnsembleBatch.run`` and NumPy metrics (tools/metrics_emul.py) from the downloaded logits.  After each epoch every
parameter is equal in every bit; the learning rates, accuracies, confusion matrices, wrong lists and the epochs ``on_improve`` was
called at are equal.  (The head's ``adjust_param`` moves a value the recorded launches took by value: a stale graph in the second
epoch would show in the parameters.)

``DeviceAdam.reset()`` followed by a step equals a fresh optimiser's first step under ``==``."""
import copy
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT
from ensemble_cases import make_clips

sys.path.insert(0, os.path.join(ROOT, 'tools'))

import metrics_emul as me  # noqa: E402

pytestmark = pytest.mark.gpu

B, N_CLASSES, LR0, EPOCHS = 5, 20, 1e-3, 2


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


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
    stored, rate = make_clips()
    train = [stored[i % len(stored)][:int((0.60 + 0.05 * (i % 5)) * len(stored[i % len(stored)])) + 3 * i] for i in range(12)]
    val = [stored[(i + 5) % len(stored)][:int((0.55 + 0.07 * (i % 4)) * len(stored[(i + 5) % len(stored)])) + 11 * i] for i in range(7)]
    # most clips of both sets carry label 3, so that an epoch of training moves the validation accuracy (an epoch that improves
    # and one that does not are both wanted); the others are seeded
    rng = np.random.default_rng(12)
    tlab, vlab = rng.integers(0, N_CLASSES, 12).astype(np.int64), rng.integers(0, N_CLASSES, 7).astype(np.int64)
    tlab[[0, 1, 2, 4, 5, 7, 8, 10, 11]] = 3
    vlab[[0, 2, 3, 4, 6]] = 3
    return rate, (train, tlab), (val, vlab)


def _same_bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _hand_loop(dev, rate, train, val, head):
    """model.py:219-240 with 137-150 and 162-187 written out: eager steps, NumPy metrics.  -> per epoch (lr, train result, val
    result, improved, parameters)."""
    import torch
    from features.ensemble import EnsembleBatch
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    tb, eb = TrainBatch(rate, head), EnsembleBatch(rate, head, [])
    opt = DeviceAdam(list(head.parameters()), lr=LR0)
    jitter_rng = random.Random(7)
    (tclips, tlab), (vclips, vlab) = train, val
    torder, vorder = list(range(len(tclips))), list(range(len(vclips)))
    prev_acc, lr, early_stop = 0, LR0, 3
    out = []
    for epoch in range(EPOCHS):
        opt.reset()
        opt.set_lr(lr)
        head.train()
        random.Random(0).shuffle(torder)
        st = me.State(N_CLASSES, 64)
        for s in range(0, len(torder), B):
            idx = torder[s:s + B]
            clips = [tclips[i] for i in idx]
            jitter = tb.draw_jitter(len(idx), jitter_rng)
            for p in opt.params:
                p.grad = None
            res = tb.run(np.concatenate(clips), _offsets(clips), tlab[idx], jitter, loss='native', dropout=False)
            res.loss.backward()
            opt.step()
            st.update(res.logits.detach().cpu().numpy().astype(np.float64), tlab[idx])
        train_res = st.result()
        head.eval()
        random.Random(0).shuffle(vorder)
        sv = me.State(N_CLASSES, 64)
        with torch.no_grad():
            for s in range(0, len(vorder), B):
                idx = vorder[s:s + B]
                clips = [vclips[i] for i in idx]
                res = eb.run(np.concatenate(clips), _offsets(clips), sync_free=True, dropout=False)
                sv.update(res.logits.cpu().numpy().astype(np.float64), vlab[idx], res.pred.cpu().numpy())
        val_res = sv.result()
        acc, lr_now = val_res.accuracy, lr
        improved = acc > prev_acc
        stop = False
        if improved:
            prev_acc = acc
            lr *= 0.8
        else:
            early_stop -= 1
            lr *= 0.5
            stop = not early_stop
        torch.cuda.synchronize(dev)
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
    assert abs(got.loss - want.loss) <= 1e-6, (tag, got.loss, want.loss)


def test_trainer_against_the_loop_written_out():
    import torch
    from features import _native as nat
    from features.ensemble import EnsembleBatch
    from features.fit import Trainer
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    nat.require_device()
    dev = torch.device('cuda', 0)
    rate, train, val = _data()
    head = _head(dev)
    twin = copy.deepcopy(head)
    want = _hand_loop(dev, rate, train, val, twin)

    tb, eb = TrainBatch(rate, head), EnsembleBatch(rate, head, [])
    opt = DeviceAdam(list(head.parameters()), lr=LR0)
    trainer = Trainer(tb, eb, opt, N_CLASSES, wrong_capacity=64, head_kwargs={'dropout': False}, jitter_rng=random.Random(7))
    snaps, improved_at = [], []

    def on_epoch(entry):
        torch.cuda.synchronize(dev)
        snaps.append([p.detach().clone() for p in head.parameters()])
    feat = lambda clips: [(c, rate) for c in clips]
    hist = trainer.fit((feat(train[0]), train[1]), (feat(val[0]), val[1]), LR0, epochs=EPOCHS, batch_size=B,
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
        print(f'epoch {k}: lr {lr:g}, train loss {entry.train.loss:.6f} acc {entry.train.accuracy:.3f}, val acc {entry.val.accuracy:.3f}, '
              f'improved {improved}')
    assert improved_at == [k for k, w in enumerate(want) if w[3]]
    assert head.training and head.enc2.a == twin.enc2.a
    assert any(not _same_bits(p, q) for p, q in zip(snaps[0], snaps[-1]))                    # the second epoch trained
    # the cumulative order of reader.py:90
    order = list(range(12))
    for entry in hist:
        random.Random(0).shuffle(order)
        assert entry.train_order == order


def test_reset_then_step_equals_a_fresh_optimisers_first_step():
    import torch
    from features import _native as nat
    from features.optim import DeviceAdam
    nat.require_device()
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device='cpu').manual_seed(3)
    shapes = [(37,), (64, 33), (5, 7, 3)]
    params = [torch.randn(s, generator=gen).to(dev).requires_grad_(True) for s in shapes]
    opt = DeviceAdam(params, lr=1e-3)
    for k in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen).to(dev)
        opt.step()
    opt.reset()
    opt.set_lr(0.8e-3)
    torch.cuda.synchronize(dev)
    assert opt.device_state()[0] == 0 and not any(bool(m.any()) for m in opt.exp_avg + opt.exp_avg_sq)
    fresh_params = [p.detach().clone().requires_grad_(True) for p in params]
    fresh = DeviceAdam(fresh_params, lr=0.8e-3)
    grads = [torch.randn(p.shape, generator=gen).to(dev) for p in params]
    for p, q, g in zip(params, fresh_params, grads):
        p.grad, q.grad = g.clone(), g.clone()
    opt.step()
    fresh.step()
    torch.cuda.synchronize(dev)
    assert opt.device_state() == fresh.device_state() and opt.device_state()[0] == 1
    for a, b in zip(params + opt.exp_avg + opt.exp_avg_sq, fresh_params + fresh.exp_avg + fresh.exp_avg_sq):
        assert _same_bits(a, b)
