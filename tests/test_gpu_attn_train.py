"""The native gradients of the attention blocks on the device (csrc/kernels_attn_bwd.h): the Transformer encoder layer
(``dsp_attn_forward_train`` / ``dsp_attn_backward`` behind ``_AttnTrain``) and the SelfAttn pooling
(``dsp_selfattn_pool_train_batch`` / ``dsp_selfattn_pool_backward_batch`` behind ``_SelfAttnTrain``).

Parity: per tensor max |got - ref| / max |ref| against fp64 autograd of the torch chain on the CPU with the same weights, at
hmrnn_cases.BAR (2e-5, the project's bar for the gradients of a native fp32 kernel); a tensor whose max |ref| is below 1e-9 of
the case's largest is measured against that largest value (gradients that are zero in exact arithmetic: the pooling's v.bias,
w_qs / w_ks at B = 1).  The torch fp32 route's error on the same device is recorded beside the native one.  The cases and their
references are tests/attn_train_cases.py's, shared with the CPU emulation test.

Mechanics: forward_train's output is bitwise the forward's; optional gradients; canaries behind every buffer the launches write
and full writes from a NaN prefill; the same bits twice, from a non-contiguous gradient, on a side stream and from a replayed
graph; routing."""
import copy

import numpy as np
import pytest

from conftest import record

import attn_train_cases as cases
import attn_bwd_emul as em
from test_gpu_attn import DIMS, SHAPES, _fill, _input

pytestmark = pytest.mark.gpu
BAR = cases.BAR


def _dev():
    import torch
    return torch.device('cuda', 0)


def _grads(mod, x, gw, native, dev, x_grad=True):
    """One forward + backward of a copy of ``mod`` on the device -> ([dx, parameter gradients ..] as NumPy or None, output)."""
    import torch
    m = copy.deepcopy(mod).to(dev)
    xt = torch.from_numpy(x).to(dev).requires_grad_(x_grad)
    out = m(xt, native=native)
    (out * torch.from_numpy(gw).to(dev)).sum().backward()
    g = [xt.grad] + [p.grad for p in m.parameters()]
    return [None if v is None else v.cpu().numpy() for v in g], out


def _check_case(kind, name, mod, x, gw, names):
    dev = _dev()
    ref = cases.reference(name, mod, x, gw)
    got, out = _grads(mod, x, gw, True, dev)
    assert type(out.grad_fn).__name__.startswith('_AttnTrain' if kind == 'block' else '_SelfAttnTrain')
    tor, _ = _grads(mod, x, gw, False, dev)
    e_nat, e_tor = em.errors(got, ref), em.errors(tor, ref)
    print(f'{kind} {name}: native {max(e_nat):.3g} ({names[int(np.argmax(e_nat))]}), torch fp32 {max(e_tor):.3g}')
    record(f'attn_{kind}_grad_native_vs_fp64', max(e_nat))
    record(f'attn_{kind}_grad_torch_vs_fp64', max(e_tor))
    for n, g, v in zip(names, got, e_nat):
        assert g is None or np.isfinite(g).all(), n
        assert v <= BAR, (n, v)


# ---- 1, 2: the block's gradients ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fill', cases.FILLS)
@pytest.mark.parametrize('dims', list(DIMS))
@pytest.mark.parametrize('T,B', SHAPES)
def test_block_gradients_equal_fp64_autograd(T, B, dims, fill):
    _check_case('block', *cases.block_case(dims, T, B, fill), cases.BLOCK_NAMES)


def test_block_gradients_with_scores_beyond_88():
    dims, T, B, fill, k = cases.OVERFLOW
    name, enc, x, gw = cases.block_case(dims, T, B, fill, k)
    smax = cases.max_score(enc, x)
    print(f'w_ks x {k:g}: max |s| {smax:.1f}')
    assert smax > 88
    _check_case('block', name, enc, x, gw, cases.BLOCK_NAMES)


# ---- raw calls ----------------------------------------------------------------------------------------------------------------

def _raw(enc, T, B, dev):
    """The handle and the byte counts of the raw training calls."""
    from features import _native as nat
    lib, handle = nat.load(), enc._native_handle(dev)
    tb, wb, db = nat.c_i64(0), nat.c_i64(0), nat.c_i64(0)
    nat.check(lib.dsp_attn_tape_bytes(handle, T, B, nat.C.byref(tb)))
    nat.check(lib.dsp_attn_backward_bytes(handle, T, B, nat.C.byref(wb), nat.C.byref(db)))
    return handle, tb.value, wb.value, db.value


def _stream(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


# ---- 3 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dims,T,B', [('head', 33, 17), ('small', 17, 2), ('head', 1, 3)])
def test_forward_train_output_is_bitwise_the_forwards(dims, T, B):
    import torch
    dev = _dev()
    _, enc, x, _ = cases.block_case(dims, T, B, 'wide')
    enc = copy.deepcopy(enc).to(dev)
    xd = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        want = enc(xd, native=True)
    y = enc(xd, native=True)
    assert y.requires_grad and not want.requires_grad and type(y.grad_fn).__name__.startswith('_AttnTrain')
    assert torch.equal(y.detach(), want)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------

def test_optional_gradients(monkeypatch):
    import torch
    from features import _native as nat
    dev = _dev()
    name, enc, x, gw = cases.block_case('head', 33, 17, 'wide')
    full, _ = _grads(enc, x, gw, True, dev)
    part, _ = _grads(enc, x, gw, True, dev, x_grad=False)          # d_gx = NULL: three launches
    assert part[0] is None
    for n, a, b in zip(cases.BLOCK_NAMES[1:], full[1:], part[1:]):
        assert np.array_equal(a, b), n
    m = copy.deepcopy(enc).to(dev)
    for n, p in m.named_parameters():
        p.requires_grad_(n == 'slf_attn.w_qs')
    y = m(torch.from_numpy(x).to(dev), native=True)
    (y * torch.from_numpy(gw).to(dev)).sum().backward()
    assert [p.grad is not None for p in m.parameters()] == [True] + [False] * 12
    assert np.array_equal(m.slf_attn.w_qs.grad.cpu().numpy(), full[1])
    # all outputs unused: backward hands out Nones without a launch
    m = copy.deepcopy(enc).to(dev)
    y = m(torch.from_numpy(x).to(dev), native=True)
    lib = nat.load()
    called = []
    real = lib.dsp_attn_backward
    monkeypatch.setattr(lib, 'dsp_attn_backward', lambda *a: called.append(1) or real(*a))
    from features.classifier import _AttnTrain
    assert _AttnTrain.backward(y.grad_fn, None) == (None,) * 15 and not called


# ---- 5 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dims,T,B', [('head', 33, 17), ('small', 17, 2), ('head', 1, 3)])
def test_block_canaries_full_writes_and_two_runs(dims, T, B):
    import torch
    from features import _native as nat
    from test_gpu_canaries import _guarded
    dev = _dev()
    lib = nat.load()
    _, enc, x, gw = cases.block_case(dims, T, B, 'wide')
    enc = copy.deepcopy(enc).to(dev)
    d = DIMS[dims][0]
    xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(gw).to(dev)
    handle, tb, wb, db = _raw(enc, T, B, dev)
    what = f'{dims} T {T} B {B}'
    _, yp, ycheck = _guarded(T * B * d * 4, dev)
    _, tp, tcheck = _guarded(tb, dev)
    nat.check(lib.dsp_attn_forward_train(handle, xd.data_ptr(), T, B, yp, tp, tb, _stream(dev)))
    y = ycheck('d_y ' + what).view(np.float32)
    tcheck('d_tape after forward_train ' + what)
    with torch.no_grad():
        assert np.array_equal(y.reshape(T, B, d), enc(xd, native=True).cpu().numpy())
    runs = []
    for _ in range(2):
        _, wp, wcheck = _guarded(wb, dev)
        _, ap, acheck = _guarded(db, dev)
        _, xp, xcheck = _guarded(T * B * d * 4, dev)
        nat.check(lib.dsp_attn_backward(handle, T, B, tp, tb, gd.data_ptr(), xp, ap, db, wp, wb, _stream(dev)))
        wcheck('d_work ' + what)
        tcheck('d_tape after backward ' + what)
        runs.append((xcheck('d_gx ' + what).copy(), acheck('d_da ' + what).copy()))
    for v in runs[0]:
        assert np.isfinite(v.view(np.float32)).all()                # every element written: the fill is a NaN pattern
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # without d_gx: the same d_da
    _, wp, wcheck = _guarded(wb, dev)
    _, ap, acheck = _guarded(db, dev)
    nat.check(lib.dsp_attn_backward(handle, T, B, tp, tb, gd.data_ptr(), None, ap, db, wp, wb, _stream(dev)))
    wcheck('d_work, no d_gx ' + what)
    assert np.array_equal(acheck('d_da, no d_gx ' + what), runs[0][1])
    # a live handle still checks its buffers
    assert lib.dsp_attn_backward(handle, T, B, tp, tb - 1, gd.data_ptr(), None, ap, db, wp, wb, _stream(dev)) == nat.EINVAL
    assert lib.dsp_attn_backward(handle, T, B, tp, tb, gd.data_ptr(), None, ap, db - 1, wp, wb, _stream(dev)) == nat.EINVAL
    assert lib.dsp_attn_backward(handle, T, B, tp, tb, gd.data_ptr(), None, ap, db, wp, wb - 1, _stream(dev)) == nat.EINVAL


def _module_step(m, xd, g):
    import torch
    m.zero_grad(set_to_none=True)
    xt = xd.detach().clone().requires_grad_(True)
    out = m(xt, native=True)
    torch.autograd.backward(out, g)
    return [xt.grad.clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]


def _same_bits_everywhere(m, xd, g, dev):
    """Two runs, a non-contiguous gradient and a side stream give the same bits."""
    import torch
    a, b = _module_step(m, xd, g), _module_step(m, xd, g)
    wide = torch.zeros(g.shape[0], 2 * g.shape[1], *g.shape[2:], device=dev)
    wide[:, ::2] = g
    assert not wide[:, ::2].is_contiguous()
    c = _module_step(m, xd, wide[:, ::2])
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        e = _module_step(m, xd, g)
    side.synchronize()
    for other in (b, c, e):
        assert len(other) == len(a) and all(torch.equal(u, v) for u, v in zip(a, other))


def test_block_two_runs_a_strided_gradient_and_a_side_stream_give_the_same_bits():
    import torch
    dev = _dev()
    _, enc, x, gw = cases.block_case('head', 33, 17, 'wide')
    _same_bits_everywhere(copy.deepcopy(enc).to(dev), torch.from_numpy(x).to(dev), torch.from_numpy(gw).to(dev), dev)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------

def test_forward_train_and_backward_captured_into_one_graph_replay_on_new_data():
    import torch
    from features import _native as nat
    dev = _dev()
    lib = nat.load()
    T, B, d = 33, 17, 39
    _, enc, x, gw = cases.block_case('head', T, B, 'wide')
    enc = copy.deepcopy(enc).to(dev)
    rng = np.random.default_rng(5)
    xs = [torch.from_numpy(x).to(dev), torch.from_numpy(_input(T, B, d, 5)).to(dev)]
    gs = [torch.from_numpy(gw).to(dev), torch.from_numpy(rng.standard_normal((T, B, d)).astype(np.float32)).to(dev)]
    handle, tb, wb, db = _raw(enc, T, B, dev)                        # (the handle is built here, outside the capture)
    new = lambda nbytes: torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)

    def calls(xb, gb, y, tape, gx, da, work):
        st = _stream(dev)
        nat.check(lib.dsp_attn_forward_train(handle, xb.data_ptr(), T, B, y.data_ptr(), tape.data_ptr(), tb, st))
        nat.check(lib.dsp_attn_backward(handle, T, B, tape.data_ptr(), tb, gb.data_ptr(), gx.data_ptr(), da.data_ptr(), db,
                                        work.data_ptr(), wb, st))

    want = []
    for k in (0, 1):
        bufs = (torch.zeros(T, B, d, device=dev), new(tb), torch.zeros(T, B, d, device=dev), new(db), new(wb))
        calls(xs[k], gs[k], *bufs)
        torch.cuda.synchronize(dev)
        want.append(bufs)
    xb, gb = xs[0].clone(), gs[0].clone()
    bufs = (torch.zeros(T, B, d, device=dev), new(tb), torch.zeros(T, B, d, device=dev), new(db), new(wb))
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls(xb, gb, *bufs)
    for k in (1, 0):
        xb.copy_(xs[k]); gb.copy_(gs[k])
        for v in bufs:
            v.zero_()
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        for i in (0, 2, 3):                                          # y, dx, da
            assert torch.equal(bufs[i], want[k][i]), (k, i)


# ---- 7: the pooling ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('T,B,H', cases.POOL_SHAPES)
def test_pooling_gradients_equal_fp64_autograd(T, B, H):
    import torch
    from features import _native as nat
    from test_gpu_canaries import _guarded
    dev = _dev()
    lib = nat.load()
    name, pool, y, gw = cases.pool_case(T, B, H)
    _check_case('pool', name, pool, y, gw, cases.POOL_NAMES)
    # raw calls: the train forward's out is bitwise the forward's; canaries; full writes; two runs
    m = copy.deepcopy(pool).to(dev)
    yd, gd = torch.from_numpy(y).to(dev), torch.from_numpy(gw).to(dev)
    par = (m.attn.weight.data_ptr(), m.attn.bias.data_ptr(), m.v.weight.data_ptr())
    _, op, ocheck = _guarded(B * H * 4, dev)
    _, wp, wcheck = _guarded(T * B * 4, dev)
    nat.check(lib.dsp_selfattn_pool_train_batch(yd.data_ptr(), T, B, H, *par, m.v.bias.data_ptr(), op, wp, _stream(dev)))
    with torch.no_grad():
        want = m(yd, native=True).cpu().numpy()
    assert np.array_equal(ocheck('d_out').view(np.float32).reshape(B, H), want)
    w = wcheck('d_w').view(np.float32).reshape(T, B)
    assert np.isfinite(w).all() and np.max(np.abs(w.sum(0) - 1)) <= 1e-5
    out = m(yd, native=True)
    assert type(out.grad_fn).__name__.startswith('_SelfAttnTrain') and np.array_equal(out.detach().cpu().numpy(), want)
    runs = []
    for _ in range(2):
        guards = [_guarded(n * 4, dev) for n in (T * B * H, T * B * H, T * B, B * H)]
        nat.check(lib.dsp_selfattn_pool_backward_batch(yd.data_ptr(), T, B, H, *par, wp, gd.data_ptr(), *[g[1] for g in guards], _stream(dev)))
        runs.append([g[2](f'pool backward buffer {i}').copy() for i, g in enumerate(guards)])
        wcheck('d_w after backward')
    for a, b in zip(*runs):
        assert np.isfinite(a.view(np.float32)).all() and np.array_equal(a, b)
    guards = [_guarded(n * 4, dev) for n in (T * B * H, T * B, B * H)]
    nat.check(lib.dsp_selfattn_pool_backward_batch(yd.data_ptr(), T, B, H, *par, wp, gd.data_ptr(), None, *[g[1] for g in guards], _stream(dev)))
    for g, want_bits in zip(guards, runs[0][1:]):
        assert np.array_equal(g[2]('pool backward without d_gy'), want_bits)


def test_pooling_two_runs_a_strided_gradient_and_a_side_stream_give_the_same_bits():
    import torch
    dev = _dev()
    _, pool, y, gw = cases.pool_case(40, 17, 200)
    _same_bits_everywhere(copy.deepcopy(pool).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(gw).to(dev), dev)


# ---- 8: the heads -----------------------------------------------------------------------------------------------------------

ZERO_IN_EXACT_ARITHMETIC = ('attn.v.bias',)      # the softmax is shift-invariant: both fp32 routes hold rounding noise only


@pytest.mark.parametrize('native_enc', [None, True])
@pytest.mark.parametrize('kind', ['transformer', 'hrnn_att'])
def test_head_training_step_with_the_native_attention(kind, native_enc):
    """TransformerHead / HRNNAttHead on the golden input cut to B 8, T 30, dropout=False: logits and every parameter gradient
    with native_attn=True against native_attn=False on the same device, in .train() (the encoder's native training path serves
    training mode, and so does MIOpen's GRU backward).  HRNNAttHead's first encoder has inter-layer dropout: with
    native_enc=True its multipliers are drawn with torch from the same seed on both steps; on the nn.GRU route, whose draws
    cannot be repeated from a seed, that dropout is switched off, so that both steps see the same network."""
    import os
    import torch
    from test_gpu_attn import HERE, _make
    dev = _dev()
    g, rnn_g = np.load(os.path.join(HERE, 'golden', 'clf_golden.npz')), np.load(os.path.join(HERE, 'golden', 'rnn_golden.npz'))
    head = _make(kind, g).to(dev)
    head = head.train()
    if native_enc is None and kind == 'hrnn_att':
        head.enc1.gru.dropout = 0.0
    T = 30
    inp = torch.from_numpy(np.ascontiguousarray(rnn_g['inp'][:T])).to(dev)
    len0 = np.minimum(np.asarray(rnn_g['len0']), T)
    assert tuple(inp.shape) == (T, 8, 39)
    w = torch.from_numpy(np.random.default_rng(2).standard_normal((8, 20)).astype(np.float32)).to(dev)
    res = {}
    for na in (True, False):
        head.zero_grad(set_to_none=True)
        torch.manual_seed(3)
        lo = head(inp, len0, dropout=False, native_enc=native_enc, native_attn=na)[0]
        (lo * w).sum().backward()
        res[na] = (lo.detach(), {n: p.grad.detach().clone() for n, p in head.named_parameters()})
    d_lo = float((res[True][0] - res[False][0]).abs().max()) / max(1.0, float(res[False][0].abs().max()))
    top = max(float(v.abs().max()) for v in res[False][1].values())
    errs = {}
    for n, gr in res[True][1].items():
        ref = res[False][1][n]
        scale = float(ref.abs().max())
        if scale < 1e-9 * top or n in ZERO_IN_EXACT_ARITHMETIC:
            scale = top
        errs[n] = float((gr - ref).abs().max()) / scale
    worst = max(errs, key=errs.get)
    print(f'{kind} head, native_enc={native_enc}: logits {d_lo:.3g}, worst parameter gradient {errs[worst]:.3g} ({worst})')
    record(f'attn_{kind}_head_grad_native_vs_torch_path', errs[worst])
    assert d_lo <= BAR
    for n, v in errs.items():
        assert v <= BAR, (n, v)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------

def test_routing():
    import torch
    from features.classifier import _SelfAttn, _TransformerEncoder
    dev = _dev()
    assert _TransformerEncoder.native_train_default is False and _SelfAttn.native_train_default is False
    _, enc, x, _ = cases.block_case('small', 17, 2, 'wide')
    _, pool, y, _ = cases.pool_case(9, 5, 12)
    for mod, inp, fn in ((enc, x, '_AttnTrain'), (pool, y, '_SelfAttnTrain')):
        m = copy.deepcopy(mod).to(dev)
        v = torch.from_numpy(inp).to(dev)
        is_native = lambda t: type(t.grad_fn).__name__.startswith(fn)
        for mode in (m.train(), m.eval()):                           # no mode-dependent behaviour: both are served
            assert is_native(mode(v, native=True))
            out = mode(v)                                            # a gradient is required (the parameters'), native=None: torch
            assert out.requires_grad and not is_native(out)
            assert not is_native(mode(v, native=False))
        m.native_train_default = True                                # (an instance attribute: the class default stays False)
        try:
            assert is_native(m(v))
        finally:
            del m.native_train_default
        with torch.no_grad():                                        # without a gradient nothing changes
            a = m(v, native=True)
            assert not a.requires_grad and a.grad_fn is None and not m(v).requires_grad
        assert torch.equal(m(v, native=True).detach(), a)
        with pytest.raises(RuntimeError, match='a gradient is required.*not on a GPU'):
            copy.deepcopy(mod)(torch.from_numpy(inp), native=True)
        # a parameter written in place between forward and backward
        out = m(v, native=True)
        with torch.no_grad():
            next(m.parameters()).mul_(1.0)
        with pytest.raises(RuntimeError, match='modified'):
            out.sum().backward()
        out = m(v, native=True)                                      # and the next step is served again
        out.sum().backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters())
