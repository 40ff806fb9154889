"""The recorded training step with the dropouts ON (features/train.py with ``rng=`` a ``features.dropout.DeviceRng``): the twin of
tests/test_gpu_train_capture.py's ``test_second_replay_equals_the_eager_step``.  The GRUs keep their inter-layer 0.2,
``dropout=True`` is passed, and every draw comes from the device generator, so the SECOND replay -- after an eager Adam step and
new clips, labels and jitter -- gives, bit for bit, the loss and every gradient of an eager ``TrainBatch.run`` + ``backward``
from the generator state that replay started from.  ``capture()`` leaves the generator where it found it.  Further: three
replays with a recorded ``DeviceAdam`` step against three eager steps, a capacity capture through ``MixedRateTrainBatch``, and a
checkpoint round trip (parameters, Adam state and the generator's two integers) that continues bit for bit.  Only head / size
pairs of ``CAPTURE_VERIFIED`` are recorded."""
import copy
import random

import numpy as np
import pytest

import capacity_cases as cc
import mixed_capacity_cases as mc
from ensemble_cases import make_clips
from golden_cases import make_signal

pytestmark = pytest.mark.gpu

SEED = 20261021
HEADS = ['RNNHead', 'HRNNHead', 'HRNNAttHead', 'TransformerHead', 'HMRNNHead']
CASES = [(kind, 32) for kind in HEADS] + [('HMRNNHead', 5), ('HRNNHead', 512)]


def _head(kind, dev):
    """In training mode, every dropout as the class builds it (enc1 of HRNNHead / HRNNAttHead: inter-layer 0.2)."""
    import torch
    from features import classifier as C
    torch.manual_seed(0)
    head = getattr(C, kind)().train()
    C.fill_parameters(head, 3)
    return head.to(dev)


def _kw(kind, rng):
    return {'rng': rng} if kind == 'RNNHead' else {'dropout': True, 'rng': rng}


def _bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _content(tb, B, rate_clips, n):
    """n batches of the same clip lengths: (waves int16, labels, jitter) host arrays, and the sample offsets."""
    clips = [rate_clips[i % len(rate_clips)] for i in range(B)]
    so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
    flat = np.concatenate(clips).astype(np.int32)
    labels = np.random.default_rng(B).integers(0, 20, B).astype(np.int64)
    waves = [flat, -flat // 2, (3 * flat) // 4, -(flat // 3)]
    return so, [(waves[k % 4].astype(np.int16), (labels + 7 * k) % 20, tb.draw_jitter(B, random.Random(B + k))) for k in range(n)]


def test_cases_are_verified_pairs():
    from features.train import CAPTURE_VERIFIED
    assert all(B in CAPTURE_VERIFIED[kind] for kind, B in CASES)


@pytest.mark.parametrize('kind,B', CASES)
def test_second_replay_equals_the_eager_step_with_dropout_on(kind, B):
    import torch
    from features.dropout import DeviceRng
    from features.train import TrainBatch
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    head = _head(kind, dev)
    tb = TrainBatch(rate, head)
    so, content = _content(tb, B, stored, 2)
    rng = DeviceRng(SEED, dev)
    rng.set_step(11)
    kw = _kw(kind, rng)
    buf, lab, jit = (torch.from_numpy(a).to(dev) for a in content[0])
    params = list(head.parameters())
    g = tb.capture(buf, so, lab, jit, **kw)
    assert rng.state_dict() == {'seed': SEED, 'step': 11} and g.rng is rng      # capture() left the generator where it was
    first = g.replay().logits.clone()
    torch.optim.Adam(params, lr=1e-3).step()
    for t, a in zip((buf, lab, jit), content[1]):
        t.copy_(torch.from_numpy(a))
    res = g.replay()
    torch.cuda.synchronize(dev)
    second, loss2, logits2 = [gr.clone() for gr in g.grads], res.loss.clone(), res.logits.clone()
    assert int(res.n_clamped.cpu()[0]) == 0
    s = rng.state_dict()['step']
    assert s == 13                                                             # one recorded advance per replay
    assert not _bits(first, logits2)
    rng.set_step(s - 1)
    for p in params:
        p.grad = None
    eager = tb.run(buf, so, lab, jit, **kw)
    eager.loss.backward()
    torch.cuda.synchronize(dev)
    assert rng.state_dict()['step'] == s
    bad = [n for (n, p), a in zip(head.named_parameters(), second) if not _bits(a, p.grad)]
    worst = max(float((a - p.grad).abs().max()) / max(1.0, float(p.grad.abs().max())) for a, p in zip(second, params))
    print(f'{kind} B={B}, dropouts on: second replay against eager: worst {worst:.3g}, differing in bits: {bad}')
    assert _bits(loss2, eager.loss) and _bits(logits2, eager.logits)
    assert not bad
    if kind != 'RNNHead':                                                      # the masks took part: some logit is a dropped +0.0
        assert bool((logits2 == 0).any())


def _assert_same_state(head_a, opt_a, head_b, opt_b):
    names = [n for n, _ in head_a.named_parameters()]
    bad = [n for n, p, q in zip(names, head_a.parameters(), head_b.parameters()) if not _bits(p, q)]
    bad += [n + '.exp_avg' for n, p, q in zip(names, opt_a.exp_avg, opt_b.exp_avg) if not _bits(p, q)]
    bad += [n + '.exp_avg_sq' for n, p, q in zip(names, opt_a.exp_avg_sq, opt_b.exp_avg_sq) if not _bits(p, q)]
    assert not bad, bad
    assert opt_a.device_state() == opt_b.device_state()


def test_three_replays_with_adam_equal_three_eager_steps_and_a_checkpoint_continues():
    """``TransformerHead`` at B = 32 with ``optimizer=DeviceAdam``: three replays against three eager steps in every parameter,
    moment and loss; and a run interrupted behind replay 2 -- parameters, Adam state and the generator's ``state_dict`` saved,
    loaded into fresh objects, a new capture, replay 3 -- ends in the same bits as the uninterrupted one."""
    import torch
    from features.dropout import DeviceRng
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    kind, B = 'TransformerHead', 32
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    head = _head(kind, dev)
    twin, resumed = copy.deepcopy(head), copy.deepcopy(head)
    tb, tb_twin, tb_res = TrainBatch(rate, head), TrainBatch(rate, twin), TrainBatch(rate, resumed)
    so, content = _content(tb, B, stored, 3)
    rng, rng_twin = DeviceRng(SEED, dev), DeviceRng(SEED, dev)
    opt = DeviceAdam(list(head.parameters()), lr=1e-3)
    buf, lab, jit = (torch.from_numpy(a).to(dev) for a in content[0])
    g = tb.capture(buf, so, lab, jit, optimizer=opt, **_kw(kind, rng))
    assert rng.state_dict() == {'seed': SEED, 'step': 0} and opt.device_state()[0] == 0
    losses, saved = [], None
    for k, c in enumerate(content):
        for t, a in zip((buf, lab, jit), c):
            t.copy_(torch.from_numpy(a))
        losses.append(g.replay().loss.clone())
        if k == 1:
            torch.cuda.synchronize(dev)
            saved = (copy.deepcopy(head.state_dict()), copy.deepcopy(opt.state_dict()), rng.state_dict())
    torch.cuda.synchronize(dev)
    assert rng.state_dict() == {'seed': SEED, 'step': 3} and saved[2] == {'seed': SEED, 'step': 2}
    # three eager steps from the same start
    opt_twin = DeviceAdam(list(twin.parameters()), lr=1e-3)
    want = []
    for c in content:
        for p in opt_twin.params:
            p.grad = None
        w, l, j = (torch.from_numpy(a).to(dev) for a in c)
        out = tb_twin.run(w, so, l, j, **_kw(kind, rng_twin))
        out.loss.backward()
        opt_twin.step()
        want.append(out.loss.detach().clone())
    torch.cuda.synchronize(dev)
    differing = [k for k in range(3) if not _bits(losses[k], want[k])]
    print(f'{kind} B={B}, dropouts on: losses {[float(x) for x in losses]}, differing from the eager steps in bits: {differing}')
    assert not differing
    _assert_same_state(head, opt, twin, opt_twin)
    assert rng_twin.state_dict() == rng.state_dict()
    # the checkpoint behind replay 2, loaded into fresh objects: replay 3 equals the uninterrupted run
    resumed.load_state_dict(saved[0])
    opt_res = DeviceAdam(list(resumed.parameters()), lr=1e-3)
    opt_res.load_state_dict(saved[1])
    rng_res = DeviceRng(0, dev)
    rng_res.load_state_dict(saved[2])
    buf_r, lab_r, jit_r = (torch.from_numpy(a).to(dev) for a in content[2])
    g_res = tb_res.capture(buf_r, so, lab_r, jit_r, optimizer=opt_res, **_kw(kind, rng_res))
    assert rng_res.state_dict() == saved[2]
    loss_res = g_res.replay().loss.clone()
    torch.cuda.synchronize(dev)
    assert _bits(loss_res, losses[2])
    _assert_same_state(resumed, opt_res, head, opt)
    assert rng_res.state_dict() == rng.state_dict()


def test_capacity_capture_of_a_mixed_rate_batch_with_dropout_on():
    """``MixedRateTrainBatch.capture(capacity=N)``, ``HMRNNHead`` at B = 5: the second replay -- other clips, lengths, rate
    assignments, labels and jitter -- against the eager ``run(capacity=N)`` from the state it started from."""
    import torch
    from features.dropout import DeviceRng
    from features.train import MixedRateTrainBatch
    kind, B = 'HMRNNHead', 5
    dev = torch.device('cuda', 0)
    head = _head(kind, dev)
    tb = MixedRateTrainBatch((44100, 48000), head)
    content = []
    for k in range(2):
        gen = np.random.default_rng(100 * B + k)
        rates = mc.rate_vector(B, (44100, 48000), 7 * B + k)
        clips = [make_signal(('vad', 900 + 40 * k + i, int(gen.uniform(0.5, 0.8) * r) + i, int(r), 0.6)) for i, r in enumerate(rates)]
        content.append((clips, rates, gen.integers(0, 20, B).astype(np.int64), tb.draw_jitter(rates, random.Random(B + k))))
    cap = (11 * max(sum(len(c) for c in b[0]) for b in content)) // 10

    def load(buf, clips, tail):
        flat = np.concatenate(clips)
        host = np.full(buf.numel(), tail, dtype=flat.dtype)
        host[:len(flat)] = flat
        buf.copy_(torch.from_numpy(host))
        return cc.offsets_of([len(c) for c in clips])

    rng = DeviceRng(SEED, dev)
    kw = _kw(kind, rng)
    buf = torch.zeros(cap, dtype=torch.int16, device=dev)
    so0 = load(buf, content[0][0], 77)
    lab, jit = torch.from_numpy(content[0][2]).to(dev), torch.from_numpy(content[0][3]).to(dev)
    g = tb.capture(buf, so0, content[0][1], lab, jit, capacity=cap, **kw)
    assert rng.state_dict() == {'seed': SEED, 'step': 0}
    first = g.replay().logits.clone()
    clips, rates, l, j = content[1]
    so = load(buf, clips, 78)
    g.sample_offsets.copy_(torch.from_numpy(so))
    g.rates.copy_(torch.from_numpy(rates))
    lab.copy_(torch.from_numpy(l))
    g.jitter.copy_(torch.from_numpy(j))
    res = g.replay()
    torch.cuda.synchronize(dev)
    second, loss2, logits2 = [gr.clone() for gr in g.grads], res.loss.clone(), res.logits.clone()
    assert int(res.n_clamped.cpu()[0]) == 0 and int(g.status.cpu()[0]) == 0 and rng.state_dict()['step'] == 2
    assert not _bits(first, logits2)
    rng.set_step(1)
    for p in head.parameters():
        p.grad = None
    eager = tb.run(buf, so, rates, lab, torch.from_numpy(j).to(dev), capacity=cap, **kw)
    eager.loss.backward()
    torch.cuda.synchronize(dev)
    bad = [n for (n, p), a in zip(head.named_parameters(), second) if not _bits(a, p.grad)]
    assert _bits(loss2, eager.loss) and _bits(logits2, eager.logits) and int(eager.status.cpu()[0]) == 0
    assert not bad
