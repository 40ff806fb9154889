"""``TrainBatch.capture`` at the sizes it serves (features/train.py: ``CAPTURE_VERIFIED``): for every head and batch size in
that table the SECOND replay -- after an eager Adam step and new clips, labels and jitter written into the captured buffers --
gives, bit for bit, the loss and every gradient of an eager ``TrainBatch.run`` + ``backward`` on the same parameters and
content.  A recorded reduction that goes wrong on replay, stale packed weights or accumulated gradients would all show.
(The GRUs' inter-layer dropout is set to 0 and ``dropout=False`` is passed: a replay and an eager step draw different
multipliers.)  Heads and sizes outside the table are refused by ``capture``."""
import random

import numpy as np
import pytest

from ensemble_cases import make_clips

pytestmark = pytest.mark.gpu


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


def _cases():
    from features.train import CAPTURE_VERIFIED
    return [(kind, B) for kind, sizes in sorted(CAPTURE_VERIFIED.items()) for B in sizes if B >= 32]


@pytest.mark.parametrize('kind,B', _cases())
def test_second_replay_equals_the_eager_step(kind, B):
    import torch
    from features.train import TrainBatch
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    clips = [stored[i % len(stored)] for i in range(B)]
    so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
    flat = np.concatenate(clips)
    head = _head(kind, dev)
    kw = {} if kind == 'RNNHead' else {'dropout': False}
    tb = TrainBatch(rate, head)
    labels = np.random.default_rng(B).integers(0, 20, B).astype(np.int64)
    buf, lab, jit = (torch.from_numpy(a).to(dev) for a in (flat, labels, tb.draw_jitter(B, random.Random(B))))
    params = list(head.parameters())
    g = tb.capture(buf, so, lab, jit, **kw)
    g.replay()
    torch.optim.Adam(params, lr=1e-3).step()
    buf.copy_(torch.from_numpy((-(flat.astype(np.int32)) // 2).astype(np.int16)))
    lab.copy_(torch.from_numpy((labels + 7) % 20))
    jit.copy_(torch.from_numpy(tb.draw_jitter(B, random.Random(B + 1))))
    res = g.replay()
    torch.cuda.synchronize(dev)
    second, loss2 = [None if gr is None else gr.clone() for gr in g.grads], res.loss.clone()
    assert int(res.n_clamped.cpu()[0]) == 0 and all(gr is not None for gr in second)
    for p in params:
        p.grad = None
    eager = tb.run(buf, so, lab, jit, **kw)
    eager.loss.backward()
    torch.cuda.synchronize(dev)
    bad = [n for (n, p), a in zip(head.named_parameters(), second) if not torch.equal(a.view(torch.int32), p.grad.view(torch.int32))]
    worst = max(float((a - p.grad).abs().max()) / max(1.0, float(p.grad.abs().max())) for a, p in zip(second, params))
    print(f'{kind} B={B}: second replay against eager: worst {worst:.3g}, differing in bits: {bad}')
    assert torch.equal(loss2.view(torch.int32), eager.loss.detach().view(torch.int32))
    assert not bad


def test_capture_refuses_what_was_not_verified():
    import torch
    from features.train import CAPTURE_VERIFIED, TrainBatch
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    B = 3
    assert all(B not in sizes for sizes in CAPTURE_VERIFIED.values())
    clips = stored[:B]
    so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
    buf = torch.from_numpy(np.concatenate(clips)).to(dev)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError, match='CAPTURE_VERIFIED'):
        TrainBatch(rate, _head('HMRNNHead', dev)).capture(buf, so, lab, None, dropout=False)
    with pytest.raises(NotImplementedError, match='CAPTURE_VERIFIED'):
        TrainBatch(rate, lambda *a, **k: None).capture(buf, so, lab, None)
