"""``device_len=True, device_grad=True`` on the five classifier heads and ``features.train.TrainBatch``: a training step whose
lengths never leave the device (features/classifier.py, features/train.py).

The reference route is the same head with HOST lengths and every native flag on (``native_enc=True, native_attn=True,
native=True``), whose gradients tests/test_gpu_bigru_train.py, tests/test_gpu_hmlstm_train.py and tests/test_gpu_attn_train.py
pin to fp64 autograd.  Fixtures as in tests/test_gpu_device_lengths.py: the inputs of tests/golden/rnn_golden.npz (B = 8,
T = 200), weights by ``fill_parameters``, heads in ``.train()``, ``dropout=False``.

  (a) all five heads on the full batch (max(len0) = 200 = the buffer's rows, so both routes run the same T and -- after the
      same ``torch.manual_seed`` -- draw the same inter-layer multipliers): every parameter gradient and the input's within
      2e-5 max(1, max |ref|) per tensor, the project's bar between two fp32 routes;
  (b) columns [1, 2, 4, 5, 7] (lengths 57, 131, 12, 99, 64: the device route runs 200 rows, the host route 131), the GRUs'
      inter-layer dropout set to 0 because the two routes would draw multipliers of different shapes: the same bar, no column
      left out;
  (c) ``device_len=True`` without ``device_grad`` still raises, ``device_grad=True`` alone is a ValueError;
  (d) ``TrainBatch`` with ``HMRNNHead`` on the stored 0.5 - 0.9 s clips of tests/ensemble_cases.py: ``run`` + ``backward``
      against host features (``ModelFeatureBatch.run`` with the same jitter) and the host-length native head; then
      ``capture``, a replay, an eager Adam step, new clips, labels and jitter written into the captured buffers, a second
      replay -- whose ``.grad``s must be, bit for bit, those of an eager ``run`` + ``backward`` on the updated parameters and the
      new content (stale packed weights or accumulated gradients would show).  Recording itself proves that nothing
      synchronises or reads device memory from the host.
"""
import os

import numpy as np
import pytest

import hmrnn_cases as hc
from conftest import record
from ensemble_cases import make_clips

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 2e-5                 # between two fp32 routes (tests/test_gpu_device_lengths.py)
KINDS = ['rnn', 'hrnn', 'hrnn_att', 'transformer', 'hmrnn']
SUB = [1, 2, 4, 5, 7]
HOST_KW = {'rnn': dict(native_enc=True), 'hrnn': dict(dropout=False, native_enc=True),
           'hrnn_att': dict(dropout=False, native_enc=True, native_attn=True),
           'transformer': dict(dropout=False, native_enc=True, native_attn=True),
           'hmrnn': dict(dropout=False, native=True, native_enc=True)}


def _err(got, ref):
    ref = ref.detach().cpu().numpy().astype(np.float64)
    return float(np.max(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


@pytest.fixture(scope='module')
def env():
    import types
    import torch
    from features import classifier as C
    dev = torch.device('cuda', 0)
    rg = np.load(os.path.join(HERE, 'golden', 'rnn_golden.npz'))
    cg = np.load(os.path.join(HERE, 'golden', 'clf_golden.npz'))
    hg = hc.load_golden()
    spec = {'rnn': (C.RNNHead, int(rg['seed'])), 'hrnn': (C.HRNNHead, int(cg['seed'])), 'hrnn_att': (C.HRNNAttHead, int(cg['seed']) + 1),
            'transformer': (C.TransformerHead, int(cg['seed']) + 2), 'hmrnn': (C.HMRNNHead, int(hg['head_seed']))}
    heads = {}
    for kind, (cls, seed) in spec.items():
        torch.manual_seed(0)
        head = cls().train()
        C.fill_parameters(head, seed)
        heads[kind] = head.to(dev)
    return types.SimpleNamespace(dev=dev, heads=heads, inp=rg['inp'], len0=np.asarray(rg['len0']))


def _step(head, kind, inp, len0, device, seed=5):
    """One forward + backward of ``logits.square().sum()`` -> (logits, [the input's gradient] + the parameters' gradients)."""
    import torch
    x = inp.clone().requires_grad_(True)
    head.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    if device:
        kw = {} if kind == 'rnn' else {'dropout': False}
        out = head(x, len0, device_len=True, device_grad=True, **kw)
    else:
        out = head(x, len0, **HOST_KW[kind])
    logits = out if kind == 'rnn' else out[0]
    logits.square().sum().backward()
    grads = [x.grad] + [p.grad for p in head.parameters()]
    assert all(g is not None for g in grads)
    return logits.detach(), [g.clone() for g in grads]


def _compare(tag, kind, head, dev_res, host_res):
    names = ['inp'] + [n for n, _ in head.named_parameters()]
    e = record(f'device_grad_{kind}_logits_{tag}', _err(dev_res[0], host_res[0]))
    assert e <= BAR, (kind, 'logits', e)
    worst = 0.0
    for name, a, b in zip(names, dev_res[1], host_res[1]):
        e = _err(a, b)
        worst = max(worst, e)
        assert e <= BAR, (kind, name, e)
    record(f'device_grad_{kind}_grads_{tag}', worst)
    print(f'{kind} {tag}: worst gradient error {worst:.3g}')


@pytest.mark.parametrize('kind', KINDS)
def test_a_all_heads_full_batch(env, kind):
    import torch
    assert env.len0.max() == 200 == env.inp.shape[0]
    inp = torch.from_numpy(env.inp).to(env.dev)
    len_d = torch.from_numpy(env.len0.astype(np.int32)).to(env.dev)
    head = env.heads[kind]
    _compare('full_batch', kind, head, _step(head, kind, inp, len_d, True), _step(head, kind, inp, env.len0, False))
    handles = [m._handle for m in head.modules() if hasattr(m, '_native_handle')]
    assert handles and all(h is not None for h in handles)
    # a second step after the parameters were written in place: the handles are kept
    with torch.no_grad():
        for p in head.parameters():
            p.mul_(1.0)
    _step(head, kind, inp, len_d, True)
    assert [m._handle for m in head.modules() if hasattr(m, '_native_handle')] == handles


@pytest.mark.parametrize('kind', KINDS)
def test_b_shorter_columns_than_the_buffer(env, kind):
    import torch
    from features.classifier import _DynEnc
    len0 = env.len0[SUB]
    assert len0.tolist() == [57, 131, 12, 99, 64]          # max(len0) = 131 < the buffer's 200 rows
    inp = torch.from_numpy(np.ascontiguousarray(env.inp[:, SUB])).to(env.dev)
    len_d = torch.from_numpy(len0.astype(np.int32)).to(env.dev)
    head = env.heads[kind]
    encs = [m for m in head.modules() if isinstance(m, _DynEnc)]
    keep = [m.gru.dropout for m in encs]
    try:
        for m in encs:                                      # the routes would draw multipliers of different shapes
            m.gru.dropout = 0.0
        _compare('sub_batch', kind, head, _step(head, kind, inp, len_d, True), _step(head, kind, inp, len0, False))
    finally:
        for m, p in zip(encs, keep):
            m.gru.dropout = p


@pytest.mark.parametrize('kind', KINDS)
def test_c_the_flag_is_opt_in(env, kind):
    import torch
    inp = torch.from_numpy(np.ascontiguousarray(env.inp[:, SUB])).to(env.dev)
    len_d = torch.from_numpy(env.len0[SUB].astype(np.int32)).to(env.dev)
    head = env.heads[kind]
    kw = {} if kind == 'rnn' else {'dropout': False}
    assert torch.is_grad_enabled() and any(p.requires_grad for p in head.parameters())
    with pytest.raises(RuntimeError, match='a gradient is required'):
        head(inp, len_d, device_len=True, **kw)
    with pytest.raises(ValueError, match='device_grad=True needs device_len=True'):
        head(inp, env.len0[SUB], device_grad=True, **kw)
    head.eval()                                             # (the forward-only path does not draw inter-layer multipliers)
    try:
        with torch.no_grad():                               # no gradient required: the forward-only path, flag or no flag
            a = head(inp, len_d, device_len=True, device_grad=True, **kw)
            b = head(inp, len_d, device_len=True, **kw)
    finally:
        head.train()
    a, b = (a, b) if kind == 'rnn' else (a[0], b[0])
    assert torch.equal(a, b)


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


def test_d_train_batch_run_capture_and_replay():
    import random
    import torch
    from features import _native as nat
    from features.classifier import HMRNNHead, fill_parameters
    from features.model_glue import ModelFeatureBatch
    from features.train import TrainBatch
    nat.require_device()
    dev = torch.device('cuda', 0)
    B = 5
    clips, rate = make_clips()
    clips = clips[:B]
    so, flat = _offsets(clips), np.concatenate(clips)
    torch.manual_seed(0)
    head = HMRNNHead().train()
    fill_parameters(head, 3)
    head = head.to(dev)
    tb = TrainBatch(rate, head)
    rng = np.random.default_rng(2)
    labels = rng.integers(0, 20, B).astype(np.int64)
    jitter = tb.draw_jitter(B, random.Random(5))
    assert jitter.shape == (B, 2) and (jitter[:, 0] <= 0).all() and (jitter[:, 1] >= 0).all() and np.abs(jitter).max() > 0
    params = list(head.parameters())

    # 1. run + backward against host features and the host-length native head, the same jitter given explicitly
    head.zero_grad(set_to_none=True)
    out = tb.run(flat, so, labels, jitter, dropout=False)
    assert out.loss.requires_grad and out.len0.is_cuda and out.len0.dtype == torch.int32
    out.loss.backward()
    got = [p.grad.clone() for p in params]
    inp_h, len0_h, _ = ModelFeatureBatch(rate).run(flat, so, jitter=jitter)
    head.zero_grad(set_to_none=True)
    logits_h = head(inp_h, len0_h, dropout=False, native=True, native_enc=True)[0]
    loss_h = torch.nn.functional.cross_entropy(logits_h, torch.from_numpy(labels).to(dev))
    loss_h.backward()
    assert np.array_equal(out.len0.cpu().numpy(), len0_h)
    assert int(out.n_clamped.cpu()[0]) == 0
    assert record('train_batch_logits_vs_host_route', _err(out.logits, logits_h)) <= BAR
    assert record('train_batch_loss_vs_host_route', _err(out.loss, loss_h)) <= BAR
    worst = 0.0
    for (name, p), g in zip(head.named_parameters(), got):
        e = _err(g, p.grad)
        worst = max(worst, e)
        assert e <= BAR, (name, e)
    record('train_batch_grads_vs_host_route', worst)
    # without a jitter: the test path's front end, other lengths
    plain = tb.run(flat, so, labels, dropout=False)
    assert not np.array_equal(plain.len0.cpu().numpy(), len0_h) or not torch.equal(plain.inp, out.inp)

    # 2. capture (recording raises on any synchronisation or host read of device memory) and a first replay
    del out, plain, logits_h, loss_h, inp_h                 # the eager steps' graphs and buffers go before the recording
    head.zero_grad(set_to_none=True)
    buf = torch.from_numpy(flat).to(dev)
    lab_buf = torch.from_numpy(labels).to(dev)
    jit_buf = torch.from_numpy(jitter).to(dev)
    handles = [m._handle for m in head.modules() if hasattr(m, '_native_handle')]
    g = tb.capture(buf, so, lab_buf, jit_buf, dropout=False)
    assert [m._handle for m in head.modules() if hasattr(m, '_native_handle')] == handles
    res = g.replay()
    torch.cuda.synchronize(dev)
    assert all(p.grad is gr for p, gr in zip(g.params, g.grads))
    worst = max(_err(gr, want) for gr, want in zip(g.grads, got))
    assert record('train_batch_replay_grads_vs_eager', worst) <= BAR
    assert int(res.n_clamped.cpu()[0]) == 0

    # 3. an eager optimiser step, 4. new content in the same buffers, 5. the second replay
    opt = torch.optim.Adam(params, lr=1e-3)
    opt.step()
    before = [gr.clone() for gr in g.grads]
    other = (-(flat.astype(np.int32)) // 2).astype(np.int16)
    labels2 = (labels + 7) % 20
    jitter2 = tb.draw_jitter(B, random.Random(11))
    assert not np.array_equal(jitter2, jitter)
    buf.copy_(torch.from_numpy(other))
    lab_buf.copy_(torch.from_numpy(labels2))
    jit_buf.copy_(torch.from_numpy(jitter2))
    opt.zero_grad()                                          # drops .grad: the replay puts the graph's tensors back
    res = g.replay()
    torch.cuda.synchronize(dev)
    second = [gr.clone() for gr in g.grads]
    loss2, len2 = res.loss.clone(), res.len0.clone()
    assert all(p.grad is gr for p, gr in zip(g.params, g.grads))
    moved = [not torch.equal(a, b) for a, b in zip(second, before)]
    print('gradients equal in both replays:', [n for (n, _), m in zip(head.named_parameters(), moved) if not m])
    assert moved[0] and moved[-1]                            # (the first GRU weight and the output bias; an all-zero gradient may stay)
    assert int(res.n_clamped.cpu()[0]) == 0

    # 6. the same step eagerly on the updated parameters and the new content: the replay's bits
    for p in params:
        p.grad = None
    eager = tb.run(buf, so, lab_buf, jit_buf, dropout=False)
    eager.loss.backward()
    torch.cuda.synchronize(dev)
    assert torch.equal(eager.len0, len2)
    worst = max(_err(a, p.grad) for a, p in zip(second, params))
    print(f'second replay against the eager step: worst gradient difference {worst:.3g}, '
          f'loss {float(loss2):.9g} against {float(eager.loss.detach()):.9g}')
    record('train_batch_second_replay_grads_vs_eager', worst)
    assert torch.equal(loss2.view(torch.int32), eager.loss.detach().view(torch.int32))
    for (name, p), a in zip(head.named_parameters(), second):
        assert torch.equal(a.view(torch.int32), p.grad.view(torch.int32)), name
    assert [m._handle for m in head.modules() if hasattr(m, '_native_handle')] == handles      # never rebuilt

    with pytest.raises(TypeError, match='device tensor'):
        tb.capture(flat, so, lab_buf, jit_buf, dropout=False)
    with pytest.raises(TypeError, match='int64 device tensor'):
        tb.capture(buf, so, labels, jit_buf, dropout=False)
