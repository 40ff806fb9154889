"""``native_wgrad=True`` on the five classifier heads and ``features.train.TrainBatch`` (features/classifier.py, features/wgrad.py):
the products behind the GRU and HM-LSTM backward recurrences as native launches bounded by a row count read on the device.

Fixtures as in tests/test_gpu_device_train.py: columns [1, 2, 4, 5, 7] of tests/golden/rnn_golden.npz (B = 5, T = 200 buffers,
lengths 57, 131, 12, 99, 64), ``dropout=False``, ``fill_parameters``, the GRUs' inter-layer dropout 0.

  (a) all five heads, on the device route (``device_len=True, device_grad=True``) and on the host-length native route: equal
      logits, and every gradient with ``native_wgrad=True`` within 2e-5 max(1, max |ref|) of the same route without it;
  (b) one ``_DynEnc`` case with caller-given inter-layer multipliers, on both routes;
  (c) with ``native_wgrad`` unset the gradients equal, under ==, those of the parent route computed in the test -- the autograd
      functions and the torch products the parent commit ran: the default path is untouched;
  (d) ``TrainBatch.capture(..., native_wgrad=True)`` with a ``DeviceAdam`` inside, ``HMRNNHead`` at B = 5 and ``TransformerHead``
      at B = 32: two replays with new clips, labels and jitter equal two eager steps in every parameter, gradient and the
      loss, bit for bit."""
import copy
import os
import random

import numpy as np
import pytest

import hmrnn_cases as hc
from conftest import record
from ensemble_cases import make_clips

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 2e-5                 # between two fp32 routes (tests/test_gpu_device_train.py)
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
        for m in head.modules():
            if isinstance(m, C._DynEnc):
                m.gru.dropout = 0.0
        heads[kind] = head.to(dev)
    len0 = np.asarray(rg['len0'])[SUB]
    assert len0.tolist() == [57, 131, 12, 99, 64]
    inp = torch.from_numpy(np.ascontiguousarray(rg['inp'][:, SUB])).to(dev)
    return types.SimpleNamespace(dev=dev, heads=heads, inp=inp, len0=len0, len_d=torch.from_numpy(len0.astype(np.int32)).to(dev))


def _step(env, kind, device, **extra):
    """One forward + backward of ``logits.square().sum()`` -> (logits, [the input's gradient] + the parameters' gradients)."""
    import torch
    head = env.heads[kind]
    x = env.inp.clone().requires_grad_(True)
    head.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    if device:
        kw = {} if kind == 'rnn' else {'dropout': False}
        out = head(x, env.len_d, device_len=True, device_grad=True, **kw, **extra)
    else:
        out = head(x, env.len0, **HOST_KW[kind], **extra)
    logits = out if kind == 'rnn' else out[0]
    logits.square().sum().backward()
    grads = [x.grad] + [p.grad for p in head.parameters()]
    assert all(g is not None for g in grads)
    return logits.detach().clone(), [g.clone() for g in grads]


@pytest.mark.parametrize('device', [True, False], ids=['device_route', 'host_route'])
@pytest.mark.parametrize('kind', KINDS)
def test_a_every_head_on_both_routes(env, kind, device):
    import torch
    plain, native = _step(env, kind, device), _step(env, kind, device, native_wgrad=True)
    assert torch.equal(plain[0], native[0]), (kind, 'logits')
    names = ['inp'] + [n for n, _ in env.heads[kind].named_parameters()]
    worst = 0.0
    for name, a, b in zip(names, native[1], plain[1]):
        assert torch.isfinite(a).all(), (kind, name)
        e = _err(a, b)
        worst = max(worst, e)
        assert e <= BAR, (kind, name, e)
    record(f"wgrad_{kind}_grads_{'device' if device else 'host'}_route", worst)
    print(f"{kind} {'device' if device else 'host'} route: worst gradient difference with native_wgrad {worst:.3g}")


@pytest.mark.parametrize('device', [True, False], ids=['device_route', 'host_route'])
def test_b_dynenc_with_given_multipliers(env, device):
    """A 3-layer ``_DynEnc`` whose inter-layer multipliers the caller gives: dx of layers 2 and 1 goes through ``dx * drop``."""
    import torch
    from features.classifier import _DynEnc, fill_parameters
    dev = env.dev
    torch.manual_seed(0)
    enc = _DynEnc(39, 200, 3, dropout=0.2).train()
    fill_parameters(enc, 9)
    enc = enc.to(dev)
    T = env.inp.shape[0] if device else int(env.len0.max())
    g = torch.Generator().manual_seed(3)
    drop = ((torch.rand(2, T, 5, 400, generator=g) < 0.8).to(torch.float32) / 0.8).to(dev)
    rows = torch.tensor([int(env.len0.max())], dtype=torch.int32, device=dev)
    res = []
    for wgrad in (False, True):
        x = env.inp.clone().requires_grad_(True)
        enc.zero_grad(set_to_none=True)
        if device:
            y, hn = enc._run_device_train(x, env.len_d, drop=drop, wgrad=wgrad, d_rows=rows if wgrad else None)
        else:
            y, hn = enc._run_native_train(x, torch.as_tensor(env.len0), drop=drop, wgrad=wgrad)
        (y.square().sum() + hn.sum()).backward()
        res.append((y.detach().clone(), [x.grad.clone()] + [p.grad.clone() for p in enc.parameters()]))
    assert torch.equal(res[0][0], res[1][0])
    worst = max(_err(a, b) for a, b in zip(res[1][1], res[0][1]))
    record(f"wgrad_dynenc_drop_grads_{'device' if device else 'host'}_route", worst)
    assert worst <= BAR, worst


def _parent_functions():
    """The autograd functions of the native training paths as the parent commit had them: the same forward launches, and in
    the backward the torch products (``gru_param_grads`` with the route's column sum, ``hm_param_grads``), nothing else."""
    import torch
    from features import _native as nat
    from features import classifier as C

    class DynEncParent(torch.autograd.Function):
        @staticmethod
        def forward(ctx, col_sum, mod, T, d_len, drop, x, *params):
            ctx.set_materialize_grads(False)
            B, H, L, dev = x.shape[1], mod.hidden_size, mod.gru.num_layers, x.device
            f32 = dict(dtype=torch.float32, device=dev)
            xc = x.detach().contiguous()
            handle, lib = mod._native_handle(dev), nat.load()
            nbytes = nat.c_i64(0)
            nat.check(lib.dsp_bigru_tape_bytes(handle, T, B, nat.C.byref(nbytes)))
            tape = torch.empty(nbytes.value // 4, **f32)
            y, hn = torch.empty(T, B, H, **f32), torch.empty(2 * L, B, H, **f32)
            nat.check(lib.dsp_bigru_forward_train(handle, xc.data_ptr(), T, B, d_len.data_ptr(), C._ptr(drop), y.data_ptr(), hn.data_ptr(),
                                                  tape.data_ptr(), nbytes.value, torch.cuda.current_stream(dev).cuda_stream))
            ctx.mod, ctx.tape_bytes, ctx.col_sum = mod, nbytes.value, col_sum
            ctx.save_for_backward(xc, d_len, tape, *params)
            return y, hn

        @staticmethod
        def backward(ctx, g_y, g_hn):
            mod = ctx.mod
            xc, d_len, tape = ctx.saved_tensors[:3]
            params = [p.detach() for p in ctx.saved_tensors[3:]]
            T, B, _ = xc.shape
            H, L, dev = mod.hidden_size, mod.gru.num_layers, xc.device
            grads = [None] * (1 + 8 * L)
            gp = lambda g: None if g is None else g.to(torch.float32).contiguous()
            g, g_hn = gp(g_y), gp(g_hn)
            lib = nat.load()
            off, rows = nat.c_i64(0), []
            for l in range(L):
                nat.check(lib.dsp_bigru_tape_rows(mod._handle, l, T, B, nat.C.byref(off)))
                rows.append(tape[off.value // 4:off.value // 4 + T * B * 2 * H].view(T, B, 2 * H))
            for l in range(L - 1, -1, -1):
                da = torch.empty(T, B, 2, 4 * H, dtype=torch.float32, device=dev)
                nat.check(lib.dsp_bigru_backward(mod._handle, l, T, B, d_len.data_ptr(), tape.data_ptr(), ctx.tape_bytes, C._ptr(g),
                                                 None if g_hn is None else g_hn[2 * l:].data_ptr(), da.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream))
                need = [l > 0 or ctx.needs_input_grad[5]] + list(ctx.needs_input_grad[6 + 8 * l:14 + 8 * l])
                res = C.gru_param_grads(params[8 * l:8 * l + 8], xc if l == 0 else rows[l - 1], rows[l], da, None, need, ctx.col_sum)
                grads[1 + 8 * l:9 + 8 * l] = res[1:]
                g = res[0]
            grads[0] = g
            return (None,) * 5 + tuple(grads)
    return DynEncParent


@pytest.mark.parametrize('kind', ['rnn', 'hmrnn'])
def test_c_unset_is_the_parent_route_bit_for_bit(env, kind, monkeypatch):
    """``native_wgrad`` unset against the parent route computed here.  The GRU encoders run through a copy of the parent's autograd
    function (its torch products, ``_ones_col_sum`` on the device route, ``a.sum(0)`` on the host route); the HM-LSTM through
    ``_HMLSTMTrain`` with ``hm_param_grads`` called directly, as the parent did.  Every gradient equal under ==."""
    import torch
    from features import classifier as C
    Parent = _parent_functions()
    for device in (True, False):
        ours = _step(env, kind, device)
        with monkeypatch.context() as mp:
            mp.setattr(C._DynEnc, '_run_device_train',
                       lambda self, x, d_len, drop=None, wgrad=False, d_rows=None:
                       (self._native_handle(x.device, refresh=True), Parent.apply(C._ones_col_sum, self, x.shape[0], d_len, None, x, *self._params()))[1])
            mp.setattr(C._DynEnc, '_run_native_train',
                       lambda self, x, lens, drop=None, wgrad=False:
                       (self._native_handle(x.device), Parent.apply(None, self, int(lens.max()), lens.to(torch.int32).to(x.device), None,
                                                                    x[:int(lens.max())], *self._params()))[1])
            called = []
            real = C.hm_param_grads
            mp.setattr(C, 'hm_param_grads', lambda *a, **k: (called.append(1), real(*a, **k))[1])
            parent = _step(env, kind, device)
            assert bool(called) == (kind == 'hmrnn')
        assert torch.equal(ours[0], parent[0]), (kind, device)
        for k, (a, b) in enumerate(zip(ours[1], parent[1])):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (kind, device, k)


def _bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


@pytest.mark.parametrize('kind,B', [('HMRNNHead', 5), ('TransformerHead', 32)])
def test_d_two_replays_equal_two_eager_steps(kind, B):
    import torch
    from features import classifier as C
    from features.optim import DeviceAdam
    from features.train import CAPTURE_VERIFIED, TrainBatch
    assert B in CAPTURE_VERIFIED[kind]
    dev = torch.device('cuda', 0)
    stored, rate = make_clips()
    torch.manual_seed(0)
    head = getattr(C, kind)().train()
    C.fill_parameters(head, 3)
    for m in head.modules():
        if isinstance(m, C._DynEnc):
            m.gru.dropout = 0.0
    head = head.to(dev)
    twin = copy.deepcopy(head)
    kw = dict(dropout=False, native_wgrad=True)
    tb, tb_twin = TrainBatch(rate, head), TrainBatch(rate, twin)
    clips = [stored[i % len(stored)] for i in range(B)]
    so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
    flat = np.concatenate(clips).astype(np.int32)
    labels = np.random.default_rng(B).integers(0, 20, B).astype(np.int64)
    content = [((flat if k == 0 else -flat // 2).astype(np.int16), (labels + 7 * k) % 20, tb.draw_jitter(B, random.Random(B + k))) for k in range(2)]
    params = list(head.parameters())
    opt = DeviceAdam(params, lr=1e-3)
    buf, lab, jit = (torch.from_numpy(a).to(dev) for a in content[0])
    g = tb.capture(buf, so, lab, jit, optimizer=opt, **kw)
    got = []
    for w, l, j in content:
        buf.copy_(torch.from_numpy(w))
        lab.copy_(torch.from_numpy(l))
        jit.copy_(torch.from_numpy(j))
        res = g.replay()
        got.append((res.loss.clone(), [gr.clone() for gr in g.grads], [p.detach().clone() for p in params]))
    torch.cuda.synchronize(dev)
    opt_twin = DeviceAdam(list(twin.parameters()), lr=1e-3)
    names = [n for n, _ in head.named_parameters()]
    for k, (w, l, j) in enumerate(content):
        for p in opt_twin.params:
            p.grad = None
        out = tb_twin.run(torch.from_numpy(w).to(dev), so, torch.from_numpy(l).to(dev), torch.from_numpy(j).to(dev), **kw)
        out.loss.backward()
        grads = [p.grad.clone() for p in opt_twin.params]
        opt_twin.step()
        torch.cuda.synchronize(dev)
        assert _bits(got[k][0], out.loss), (kind, k, float(got[k][0]), float(out.loss))
        bad = [n for n, a, b in zip(names, got[k][1], grads) if not _bits(a, b)]
        bad += [n + ' (parameter)' for n, a, b in zip(names, got[k][2], twin.parameters()) if not _bits(a, b)]
        assert not bad, (kind, k, bad)
    assert not _bits(got[0][0], got[1][0])                       # the second replay saw the new content
