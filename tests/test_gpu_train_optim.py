"""``TrainBatch.capture(..., optimizer=DeviceAdam)``: refresh, front end, forward, loss, backward and the Adam step as ONE HIP
graph.  Three replays -- new clips, labels and jitter each, ``set_lr(0.8e-3)`` before the third -- against three eager
``TrainBatch.run`` + ``backward`` + ``DeviceAdam.step()`` steps from the same start: every parameter, both moments, the step
count and the loss of each step equal in every bit.  All five heads at B = 32, ``HMRNNHead`` at B = 5, ``TransformerHead`` at
B = 512.  ``capture()`` alone changes neither parameters nor state; an eager step on other gradients between two replays does
not mislead the next replay.  (Dropout off as in tests/test_gpu_train_capture.py: a replay and an eager step draw different
multipliers.)  ``DeviceAdam`` against ``torch.optim.Adam`` over three real steps is recorded, not asserted: the gradients feed
back, so no bound is derivable."""
import copy
import random

import numpy as np
import pytest

import adam_cases as ac
from conftest import record
from ensemble_cases import make_clips

pytestmark = pytest.mark.gpu

CASES = [(kind, 32) for kind in ac.HEADS] + [('HMRNNHead', 5), ('TransformerHead', 512)]
LRS = [1e-3, 1e-3, 0.8e-3]


def _head(kind, dev):
    import torch
    from features import classifier as C
    torch.manual_seed(0)
    head = getattr(C, kind)().train()
    C.fill_parameters(head, 3)
    for m in head.modules():
        if isinstance(m, C._DynEnc):
            m.gru.dropout = 0.0
    return head.to(dev)


def _content(tb, B, rate_clips, n):
    """n batches of the same clip lengths: (waves int16, labels, jitter) host arrays, and the sample offsets."""
    clips = [rate_clips[i % len(rate_clips)] for i in range(B)]
    so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
    flat = np.concatenate(clips).astype(np.int32)
    labels = np.random.default_rng(B).integers(0, 20, B).astype(np.int64)
    waves = [flat, -flat // 2, (3 * flat) // 4, -(flat // 3)]
    return so, [(waves[k % 4].astype(np.int16), (labels + 7 * k) % 20, tb.draw_jitter(B, random.Random(B + k))) for k in range(n)]


def _bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _eager_step(tb, opt, content, so, dev, kw):
    import torch
    buf, lab, jit = (torch.from_numpy(a).to(dev) for a in content)
    for p in opt.params:
        p.grad = None
    out = tb.run(buf, so, lab, jit, **kw)
    out.loss.backward()
    opt.step()
    return out.loss.detach().clone()


def _assert_same_state(head_a, opt_a, head_b, opt_b, step, lr):
    names = [n for n, _ in head_a.named_parameters()]
    bad = [n for n, p, q in zip(names, head_a.parameters(), head_b.parameters()) if not _bits(p, q)]
    bad += [n + '.exp_avg' for n, p, q in zip(names, opt_a.exp_avg, opt_b.exp_avg) if not _bits(p, q)]
    bad += [n + '.exp_avg_sq' for n, p, q in zip(names, opt_a.exp_avg_sq, opt_b.exp_avg_sq) if not _bits(p, q)]
    assert not bad, bad
    assert opt_a.device_state() == opt_b.device_state() == (step, lr, 0.9, 0.999, 1e-8)


@pytest.mark.parametrize('kind,B', CASES)
def test_three_replays_equal_three_eager_steps(kind, B):
    import torch
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    head = _head(kind, dev)
    twin = copy.deepcopy(head)                                     # the same start for the eager steps
    kw = {} if kind == 'RNNHead' else {'dropout': False}
    tb, tb_twin = TrainBatch(rate, head), TrainBatch(rate, twin)
    so, content = _content(tb, B, stored, 3)
    params = list(head.parameters())
    opt = DeviceAdam(params, lr=LRS[0])
    buf, lab, jit = (torch.from_numpy(a).to(dev) for a in content[0])
    start = [p.detach().clone() for p in params]
    versions = [p._version for p in params]
    g = tb.capture(buf, so, lab, jit, optimizer=opt, **kw)
    torch.cuda.synchronize(dev)
    # capture() alone: parameters and optimiser state untouched (the warm-up does not step, the recording runs nothing)
    assert all(_bits(p, q) for p, q in zip(params, start)) and [p._version for p in params] == versions
    assert all(not bool(m.any()) for m in opt.exp_avg + opt.exp_avg_sq)
    assert opt.device_state() == (0, LRS[0], 0.9, 0.999, 1e-8) and all(p.grad is None for p in params)
    losses = []
    for k, (w, l, j) in enumerate(content):
        buf.copy_(torch.from_numpy(w))
        lab.copy_(torch.from_numpy(l))
        jit.copy_(torch.from_numpy(j))
        if LRS[k] != opt.lr:
            opt.set_lr(LRS[k])
        before = [p._version for p in params]
        res = g.replay()
        assert all(p._version > v for p, v in zip(params, before)) and all(p.grad is gr for p, gr in zip(params, g.grads))
        losses.append(res.loss.clone())
    torch.cuda.synchronize(dev)
    assert int(res.n_clamped.cpu()[0]) == 0
    opt_twin = DeviceAdam(list(twin.parameters()), lr=LRS[0])
    want = []
    for k in range(3):
        if LRS[k] != opt_twin.lr:
            opt_twin.set_lr(LRS[k])
        want.append(_eager_step(tb_twin, opt_twin, content[k], so, dev, kw))
    torch.cuda.synchronize(dev)
    differing = [k for k in range(3) if not _bits(losses[k], want[k])]
    print(f'{kind} B={B}: losses {[float(x) for x in losses]}, differing from the eager steps in bits: {differing}')
    assert not differing
    _assert_same_state(head, opt, twin, opt_twin, 3, LRS[2])
    assert not any(_bits(p, q) for p, q in zip(params, start))     # ... and every parameter moved


def test_an_eager_step_between_two_replays_does_not_mislead_the_next():
    import torch
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    dev = torch.device('cuda', 0)
    kind, B, kw = 'TransformerHead', 32, {'dropout': False}
    stored, rate = make_clips()
    head = _head(kind, dev)
    twin = copy.deepcopy(head)
    tb, tb_twin = TrainBatch(rate, head), TrainBatch(rate, twin)
    so, content = _content(tb, B, stored, 2)
    params = list(head.parameters())
    gen = torch.Generator(device='cpu').manual_seed(11)
    other = [(1e-3 * torch.randn(p.shape, generator=gen)).to(dev) for p in params]
    opt, opt_twin = DeviceAdam(params), DeviceAdam(list(twin.parameters()))
    buf, lab, jit = (torch.from_numpy(a).to(dev) for a in content[0])
    g = tb.capture(buf, so, lab, jit, optimizer=opt, **kw)
    g.replay()
    for p, o in zip(params, other):                                # the caller's own gradients, elsewhere in memory
        p.grad = o.clone()
    opt.step()
    assert opt._bound != tuple(gr.data_ptr() for gr in g.grads)
    for t, a in zip((buf, lab, jit), content[1]):
        t.copy_(torch.from_numpy(a))
    loss = g.replay().loss.clone()
    assert opt._bound == tuple(gr.data_ptr() for gr in g.grads)
    _eager_step(tb_twin, opt_twin, content[0], so, dev, kw)
    for p, o in zip(opt_twin.params, other):
        p.grad = o.clone()
    opt_twin.step()
    want = _eager_step(tb_twin, opt_twin, content[1], so, dev, kw)
    torch.cuda.synchronize(dev)
    assert _bits(loss, want)
    _assert_same_state(head, opt, twin, opt_twin, 3, 1e-3)


def test_capture_refuses_another_optimizer_or_other_parameters():
    import torch
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    head = _head('TransformerHead', dev)
    tb = TrainBatch(rate, head)
    so, content = _content(tb, 32, stored, 1)
    buf, lab, jit = (torch.from_numpy(a).to(dev) for a in content[0])
    params = list(head.parameters())
    with pytest.raises(TypeError, match='DeviceAdam'):
        tb.capture(buf, so, lab, jit, optimizer=torch.optim.Adam(params), dropout=False)
    with pytest.raises(ValueError, match="the head's trainable parameters"):
        tb.capture(buf, so, lab, jit, optimizer=DeviceAdam(params[1:]), dropout=False)
    with pytest.raises(ValueError, match="the head's trainable parameters"):
        tb.capture(buf, so, lab, jit, optimizer=DeviceAdam(params[::-1]), dropout=False)


def test_three_real_steps_against_torch_adam_recorded():
    """Recorded, not asserted: each side's gradients come from its own parameters, so a last-bit difference feeds back."""
    import torch
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    dev = torch.device('cuda', 0)
    kind, B, kw = 'HMRNNHead', 5, {'dropout': False}
    stored, rate = make_clips()
    head = _head(kind, dev)
    twin = copy.deepcopy(head)
    tb, tb_twin = TrainBatch(rate, head), TrainBatch(rate, twin)
    so, content = _content(tb, B, stored, 3)
    opt = DeviceAdam(list(head.parameters()))
    t_opt = torch.optim.Adam(list(twin.parameters()), lr=1e-3)
    t_opt.params = list(twin.parameters())
    for k in range(3):
        _eager_step(tb, opt, content[k], so, dev, kw)
        _eager_step(tb_twin, t_opt, content[k], so, dev, kw)
    torch.cuda.synchronize(dev)
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(head.parameters(), twin.parameters()))
    record('adam_real_head_3_steps_vs_torch_max_abs_over_lr', worst / 1e-3)
    print(f'{kind} B={B}: DeviceAdam against torch.optim.Adam after 3 steps: max |dp| = {worst:.3g} ({worst / 1e-3:.3g} lr)')
    assert np.isfinite(worst)
