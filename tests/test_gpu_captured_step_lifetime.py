"""A recorded training step keeps its head alive (features/train.py::``_record``).

The head's modules own the native handles -- the packed copies of the weights that the recorded kernels read -- and a module's
``__del__`` destroys its handle (features/classifier.py::``_NativeHandle``).  A ``_CapturedStep`` therefore holds the head: the caller may
drop every reference of its own to the head and to the ``TrainBatch`` and go on replaying.

The case is also the one ``native_sums=True`` replay at a size INSIDE ``CAPTURE_VERIFIED`` (``HMRNNHead``, B = 32), where ``capture``
records into a plain graph, without ``keep_graph``: three replays -- with the head and the batch object dropped and collected
behind the capture -- equal three eager steps of a twin in every bit of every loss, parameter and Adam moment."""
import copy
import gc
import random

import numpy as np

import pytest

from ensemble_cases import make_clips

pytestmark = pytest.mark.gpu


def _bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def test_replays_behind_a_dropped_head_equal_eager_steps():
    import torch
    from features import classifier as C
    from features.optim import DeviceAdam
    from features.train import CAPTURE_VERIFIED, TrainBatch
    kind, B = 'HMRNNHead', 32
    assert B in CAPTURE_VERIFIED[kind]
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    torch.manual_seed(0)
    head = C.HMRNNHead().train()
    C.fill_parameters(head, 3)
    head = head.to(dev)
    twin = copy.deepcopy(head)
    tb, tb_twin = TrainBatch(rate, head), TrainBatch(rate, twin)
    clips = [stored[i % len(stored)] for i in range(B)]
    so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
    flat = np.concatenate(clips).astype(np.int32)
    labels = np.random.default_rng(B).integers(0, 20, B).astype(np.int64)
    content = [(w.astype(np.int16), (labels + 7 * k) % 20, tb.draw_jitter(B, random.Random(B + k)))
               for k, w in enumerate((flat, -flat // 2, (3 * flat) // 4))]
    kw = dict(loss='native', dropout=False, native_sums=True)
    params = list(head.parameters())
    opt = DeviceAdam(params, lr=1e-3)
    buf, lab, jit = (torch.from_numpy(a).to(dev) for a in content[0])
    g = tb.capture(buf, so, lab, jit, optimizer=opt, **kw)
    assert g.census is None                                        # a pair of the table: a plain graph, no census taken
    handles = [m for m in head.modules() if isinstance(m, C._NativeHandle)]
    assert handles and all(m._handle is not None for m in handles)
    del head, tb, handles
    gc.collect()
    losses = []
    for w, l, j in content:
        buf.copy_(torch.from_numpy(w))
        lab.copy_(torch.from_numpy(l))
        jit.copy_(torch.from_numpy(j))
        losses.append(g.replay().loss.clone())
    torch.cuda.synchronize(dev)
    opt_twin = DeviceAdam(list(twin.parameters()), lr=1e-3)
    want = []
    for w, l, j in content:
        for p in opt_twin.params:
            p.grad = None
        out = tb_twin.run(torch.from_numpy(w).to(dev), so, torch.from_numpy(l).to(dev), torch.from_numpy(j).to(dev), **kw)
        out.loss.backward()
        opt_twin.step()
        want.append(out.loss.detach().clone())
    torch.cuda.synchronize(dev)
    differing = [k for k in range(3) if not _bits(losses[k], want[k])]
    print(f'{kind} B={B}: losses {[float(x) for x in losses]}, differing from the eager steps in bits: {differing}')
    assert not differing and not _bits(losses[0], losses[1])
    names = [n for n, _ in twin.named_parameters()]
    bad = [n for n, p, q in zip(names, params, twin.parameters()) if not _bits(p, q)]
    bad += [n + '.exp_avg' for n, p, q in zip(names, opt.exp_avg, opt_twin.exp_avg) if not _bits(p, q)]
    bad += [n + '.exp_avg_sq' for n, p, q in zip(names, opt.exp_avg_sq, opt_twin.exp_avg_sq) if not _bits(p, q)]
    assert not bad, bad
    assert opt.device_state() == opt_twin.device_state() and opt.device_state()[0] == 3
