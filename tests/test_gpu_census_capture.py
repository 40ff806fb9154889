"""``capture(..., census=True)`` on the five batch classes (features/train.py, features/ensemble.py, features/model_glue.py), and the
gate that a capture outside ``CAPTURE_VERIFIED`` puts in front of a recorded step (features/train.py::``_record``).

  * ``ModelFeatureBatch`` (exact layout and ``capacity=``) and ``EnsembleBatch``: ``g.census`` counts the nodes of the recorded graph,
    which is a chain without a memset node of more than 4 bytes; a replay of the graph recorded with ``census=True`` equals, in
    every bit, a replay of the graph recorded without it (``g.census`` is None there);
  * ``TrainBatch`` (``TransformerHead`` and ``HMRNNHead`` at B = 32), ``MixedRateTrainBatch`` (``HMRNNHead`` at B = 5) and
    ``AdvTrainBatch`` (B = 32) on the DEFAULT route at sizes of the tables: the census is attached and printed -- it shows what the
    verified graphs are made of (reductions of torch's, and whether any memset node) --, its counts add up, and a
    replay gives the loss of the graph recorded without it in every bit;
  * the gate: a head of a library class whose forward adds one reduction of torch's is refused outside the table with a
    RuntimeError that carries the census, although ``native_sums=True`` and ``loss='native'`` are given.  (Kernels the runtime
    gives no name for -- '?': the library GEMMs, launched from code objects -- are counted and printed, not refused.)"""
import random

import numpy as np
import pytest

import mixed_capacity_cases as mc
from ensemble_cases import make_clips
from golden_cases import make_signal

pytestmark = pytest.mark.gpu


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


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


def _bits(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach().reshape(-1).view(torch.uint8), b.detach().reshape(-1).view(torch.uint8))


def _check(c, what):
    print(f'{what}: {c.nodes} nodes = {c.kernels} kernels + {c.memsets} memsets (wide {c.wide_memsets}, widest {c.widest_memset_bytes} B) + '
          f'{c.memcpys} memcpys + {c.others} others; {c.roots} root(s), fan-out {c.max_fanout}; reductions of torch\'s: {len(c.torch_reductions())}, nameless: {len(c.kernels_named("?"))}')
    assert c.nodes == c.kernels + c.memsets + c.memcpys + c.others and c.kernels > 0 and len(c.kernel_names) == c.kernels, (what, c)
    assert c.roots >= 1 and c.max_fanout >= 1 and c.wide_memsets <= c.memsets and (c.widest_memset_bytes > 0) == (c.memsets > 0), (what, c)


def test_feature_and_ensemble_graphs():
    import torch
    from features import _native as nat
    from features.ensemble import EnsembleBatch
    from features.model_glue import ModelFeatureBatch
    nat.require_device()
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    clips = stored[:5]
    flat, so = np.concatenate(clips), _offsets(clips)
    buf = torch.from_numpy(flat).to(dev)
    mfb = ModelFeatureBatch(rate=rate)
    pairs = {'exact': [mfb.capture(buf, mfb.pipe.prepare(so, 0), census=c) for c in (True, False)]}
    cap = (5 * len(flat)) // 4
    big = torch.zeros(cap, dtype=torch.int16, device=dev)
    big[:len(flat)].copy_(buf)
    pairs['capacity'] = [mfb.capture(big, so, capacity=cap, census=c) for c in (True, False)]
    for tag, (g, plain) in pairs.items():
        assert plain.census is None
        _check(g.census, f'ModelFeatureBatch {tag}')
        assert g.census.is_chain and g.census.wide_memsets == 0 and g.census.torch_reductions() == (), (tag, g.census)
        a, b = g.replay(), plain.replay()
        torch.cuda.synchronize(dev)
        assert all(_bits(x, y) for x, y in zip(a, b)), tag
    head = _head('HMRNNHead', dev).eval()
    eb = EnsembleBatch(rate, head, [])
    g, plain = (eb.capture(buf, so, dropout=False, census=c) for c in (True, False))
    assert plain.census is None
    _check(g.census, 'EnsembleBatch HMRNNHead B=5')
    assert g.census.is_chain and g.census.wide_memsets == 0, g.census
    a, b = g.replay(), plain.replay()
    torch.cuda.synchronize(dev)
    assert _bits(a.logits, b.logits) and _bits(a.pred, b.pred) and _bits(a.len0, b.len0)


@pytest.mark.parametrize('kind,B', [('TransformerHead', 32), ('HMRNNHead', 32)])
def test_train_batch_default_route_at_a_verified_size(kind, B):
    import torch
    from features.train import CAPTURE_VERIFIED, TrainBatch
    assert B in CAPTURE_VERIFIED[kind]
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    clips = [stored[i % len(stored)] for i in range(B)]
    buf, so = torch.from_numpy(np.concatenate(clips)).to(dev), _offsets(clips)
    lab = torch.from_numpy(np.random.default_rng(B).integers(0, 20, B).astype(np.int64)).to(dev)
    head = _head(kind, dev)
    tb = TrainBatch(rate, head)
    jit = torch.from_numpy(tb.draw_jitter(B, random.Random(B))).to(dev)
    g, plain = (tb.capture(buf, so, lab, jit, dropout=False, census=c) for c in (True, False))
    assert plain.census is None
    _check(g.census, f'TrainBatch {kind} B={B}, default route')
    a, b = g.replay().loss.clone(), plain.replay().loss.clone()
    torch.cuda.synchronize(dev)
    assert _bits(a, b) and all(_bits(x, y) for x, y in zip(g.grads, plain.grads))


def test_mixed_rate_and_adversarial_default_routes():
    import torch
    from features.train import AdvTrainBatch, MixedRateTrainBatch
    dev = torch.device('cuda', 0)
    B = 5
    head = _head('HMRNNHead', dev)
    tb = MixedRateTrainBatch((44100, 48000), head)
    rates = mc.rate_vector(B, (44100, 48000), 7 * B)
    clips = [make_signal(('vad', 900 + i, int(0.6 * r) + i, int(r), 0.6)) for i, r in enumerate(rates)]
    flat, so = np.concatenate(clips), _offsets(clips)
    cap = (11 * len(flat)) // 10
    buf = torch.zeros(cap, dtype=torch.int16, device=dev)
    buf[:len(flat)].copy_(torch.from_numpy(flat))
    lab = torch.from_numpy(np.arange(B, dtype=np.int64)).to(dev)
    jit = torch.from_numpy(tb.draw_jitter(rates, random.Random(B))).to(dev)
    g = tb.capture(buf, so, rates, lab, jit, capacity=cap, dropout=False, census=True)
    _check(g.census, 'MixedRateTrainBatch HMRNNHead B=5, default route')
    loss = g.replay().loss.clone()
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(loss)) and int(g.status.cpu()[0]) == 0

    B = 32
    stored, rate = make_clips()
    clips = [stored[i % len(stored)] for i in range(B)]
    buf, so = torch.from_numpy(np.concatenate(clips)).to(dev), _offsets(clips)
    r = np.random.default_rng(B)
    lab, spk = (torch.from_numpy(r.integers(0, n, B).astype(np.int64)).to(dev) for n in (20, 35))
    adv = _head('AdvHRNNHead', dev)
    ab = AdvTrainBatch(rate, adv)
    jit = torch.from_numpy(ab.draw_jitter(B, random.Random(B))).to(dev)
    g, plain = (ab.capture(buf, so, lab, spk, jit, dropout=False, census=c) for c in (True, False))
    assert plain.census is None
    _check(g.census, 'AdvTrainBatch B=32, default route (torch discriminator, torch loss)')
    a, b = g.replay().loss.clone(), plain.replay().loss.clone()
    torch.cuda.synchronize(dev)
    assert _bits(a, b)


def test_a_step_with_a_reduction_of_torchs_is_refused_outside_the_table():
    import torch
    from features import classifier as C
    from features.graphcheck import Census
    from features.train import CAPTURE_VERIFIED, TrainBatch
    dev = torch.device('cuda', 0)

    class RNNHead(C.RNNHead):                    # a library class by name; its forward adds what the switch is there to keep out
        def forward(self, inp, len0, **kw):
            return super().forward(inp, len0, **kw) + 0.0 * inp.sum(0).sum()

    B = 7
    assert B not in CAPTURE_VERIFIED['RNNHead']
    torch.manual_seed(0)
    head = RNNHead().train()
    C.fill_parameters(head, 3)
    head = head.to(dev)
    stored, rate = make_clips()
    clips = [stored[i % len(stored)] for i in range(B)]
    buf, so = torch.from_numpy(np.concatenate(clips)).to(dev), _offsets(clips)
    lab = torch.from_numpy(np.arange(B, dtype=np.int64)).to(dev)
    tb = TrainBatch(rate, head)
    jit = torch.from_numpy(tb.draw_jitter(B, random.Random(B))).to(dev)
    from features.optim import DeviceAdam
    opt = DeviceAdam(list(head.parameters()), lr=1e-3)
    bound, before = opt._bound, [p.detach().clone() for p in head.parameters()]
    with pytest.raises(RuntimeError, match=r"reduction kernel\(s\) of torch's.*Census\(") as e:
        tb.capture(buf, so, lab, jit, optimizer=opt, loss='native', native_sums=True)
    torch.cuda.synchronize(dev)
    # a refused capture leaves the optimiser and the parameters as it found them
    assert opt._bound is bound and opt.device_state()[0] == 0 and all(p.grad is None for p in head.parameters())
    assert all(torch.equal(p, q) for p, q in zip(head.parameters(), before))
    assert 'reduce_kernel' in str(e.value)
    c = Census(nodes=2, kernels=2, memsets=0, memcpys=0, others=0, wide_memsets=0, widest_memset_bytes=0, roots=1, max_fanout=1,
               kernel_names=('?', 'adam_step_kernel'))
    assert c.kernels_named('?') == ('?',) and c.torch_reductions() == ()
