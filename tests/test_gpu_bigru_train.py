"""The native training path of the bidirectional GRU encoder on the GPU (dsp_bigru_forward_train + dsp_bigru_backward,
csrc/kernels_bigru_bwd.h, features/classifier.py::_DynEncTrain): gradients against autograd of the fp64 nn.GRU route on the CPU
with the same weights, the properties of the two calls (optional gradients, lengths, dropout multipliers, bitwise
repeatability, buffer edges, graph capture), whole training steps of two heads and the routing.

A GRU has no thresholds: no column is ever left out.  The metric is max |got - ref| / max |ref| per tensor, the bar
hmrnn_cases.BAR (2e-5, the project's bar for the gradients of a native fp32 recurrence)."""
import copy
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

import hmrnn_cases as hc
from conftest import ROOT, record

pytestmark = pytest.mark.gpu

# (input, hidden, layers, B, T): one tile with seven idle waves and T = 1; three layers; the shipped shape with three slices
# and B not a multiple of 16; the largest instantiation (maximum LDS); the widest input with mixed chunks; four layers
GRAD_CASES = [(1, 4, 1, 1, 1), (13, 20, 3, 5, 3), (39, 200, 2, 37, 24), (5, 256, 2, 19, 7), (512, 132, 1, 16, 12), (24, 100, 4, 21, 5)]
SEED = 20261000


def _dev():
    import torch
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def emul():
    spec = importlib.util.spec_from_file_location('_bigru_bwd_emul', os.path.join(ROOT, 'tools', 'bigru_bwd_emul.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def names(L):
    return ['x'] + [f'gru.{n}_l{l}{sfx}' for l in range(L) for sfx in ('', '_reverse') for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


def _module(I, H, L, seed=SEED):
    import torch
    from features.classifier import _DynEnc, fill_parameters
    torch.manual_seed(0)
    m = _DynEnc(I, H, L).train()                         # the native training path serves training mode; no dropout is configured
    fill_parameters(m, seed)
    return m


@functools.lru_cache(maxsize=None)
def truth(I, H, L, B, T, lens_kind='ragged', only=None, with_drop=False):
    """The case's inputs (float32) and the gradients of the fp64 nn.GRU route on the CPU (``_DynEnc._run_torch``; with
    multipliers: single-layer fp64 ``_DynEnc``s with the same d_drop applied by hand between them).  Computed once, shared,
    never modified."""
    import torch
    m = _module(I, H, L)
    rng = np.random.default_rng(SEED + 1)
    x = rng.standard_normal((T, B, I)).astype(np.float32)
    lens = rng.integers(1, T + 1, B)
    if lens_kind == 'edges':
        lens[0], lens[-1] = 1, T
    elif lens_kind == 'full':
        lens[:] = T
    lens[B // 2] = T                                     # y has T rows in every case
    w_y, w_hn = rng.standard_normal((T, B, H)).astype(np.float32), rng.standard_normal((2 * L, B, H)).astype(np.float32)
    drop = ((rng.random((L - 1, T, B, 2 * H)) < 0.8) / 0.8).astype(np.float32) if with_drop else None
    if only == 'y':
        w_hn = None
    elif only == 'hn':
        w_y = None
    t64 = lambda a: None if a is None else torch.from_numpy(a).double()
    ref = emul().autograd_reference([p.detach().double() for p in m._params()], t64(x), torch.from_numpy(lens), t64(w_y), t64(w_hn), t64(drop))
    return dict(module=m, x=x, lens=lens, w_y=w_y, w_hn=w_hn, drop=drop, ref=[g.numpy() for g in ref], L=L)


def device_grads(case, native, dev=None):
    """-> (gradients of x and of every gru.* parameter as numpy, y, h_n) of the fp32 module on the device."""
    import torch
    dev = dev or _dev()
    m = copy.deepcopy(case['module']).to(dev)
    x = torch.from_numpy(case['x']).to(dev).requires_grad_(True)
    lens = torch.from_numpy(case['lens'])
    if case['drop'] is not None:
        assert native
        y, hn = m._run_native_train(x, lens, drop=torch.from_numpy(case['drop']).to(dev))
    else:
        y, hn = m.run(x, lens, native=native)
    loss = sum((o * torch.from_numpy(v).to(dev)).sum() for o, v in ((y, case['w_y']), (hn, case['w_hn'])) if v is not None)
    grads = torch.autograd.grad(loss, [x] + m._params())
    return [g.detach().cpu().numpy() for g in grads], y.detach(), hn.detach()


def rel_errors(got, ref, L):
    return {n: float(np.max(np.abs(a.astype(np.float64) - b))) / (float(np.max(np.abs(b))) or 1.0) for n, a, b in zip(names(L), got, ref)}


def check_against_truth(case, tag, with_gru_path=True):
    L = case['L']
    got, _, _ = device_grads(case, native=True)
    e_nat = rel_errors(got, case['ref'], L)
    worst = record('bigru_grad_native_vs_fp64', max(e_nat.values()))
    line = f'{tag}: native {worst:.3g}'
    if with_gru_path:
        gru, _, _ = device_grads(case, native=False)
        worst_gru = record('bigru_grad_gru_path_vs_fp64', max(rel_errors(gru, case['ref'], L).values()))
        line += f', nn.GRU path on the device {worst_gru:.3g}, ratio {worst / max(worst_gru, 1e-300):.2f}'
    print(line + ': ' + ', '.join(f'{n} {v:.2g}' for n, v in e_nat.items()))
    for n, v in e_nat.items():
        assert v <= hc.BAR, (n, v)
    return got


@pytest.mark.parametrize('I,H,L,B,T', GRAD_CASES)
def test_gradients_equal_the_fp64_route(I, H, L, B, T):
    """dx and every gru.* gradient, loss = a random-weighted sum of y and h_n; the nn.GRU path's own error on the same device
    is recorded beside the native one."""
    check_against_truth(truth(I, H, L, B, T), f'{I} -> {H} x {L} B {B} T {T}')


def test_lengths_one_and_T():
    case = truth(39, 200, 2, 37, 24, lens_kind='edges')
    assert case['lens'][0] == 1 and case['lens'][-1] == 24
    check_against_truth(case, 'len 1 and len T')


# ---- the two calls on raw pointers ---------------------------------------------------------------------------------------

def _raw_train(m, x, T, B, d_len=None, drop=None, guarded=False):
    """dsp_bigru_forward_train on raw pointers -> dict of buffers (with ``guarded`` the tape sits between sentinel words)."""
    import torch
    from features import _native as nat
    from test_gpu_canaries import PAD, _guarded
    dev = x.device
    H, L = m.hidden_size, m.gru.num_layers
    handle, lib = m._native_handle(dev), nat.load()
    n = nat.c_i64(0)
    nat.check(lib.dsp_bigru_tape_bytes(handle, T, B, C.byref(n)))
    o = dict(y=torch.empty(T, B, H, device=dev), hn=torch.empty(2 * L, B, H, device=dev), tape_bytes=n.value, handle=handle, len=d_len)
    if guarded:
        buf, o['tape_ptr'], o['tape_check'] = _guarded(n.value, dev)
        o['tape'] = buf.view(torch.float32)[PAD // 4:PAD // 4 + n.value // 4]
    else:
        o['tape'] = torch.empty(n.value // 4, device=dev)
        o['tape_ptr'] = o['tape'].data_ptr()
    ptr = lambda t: None if t is None else t.data_ptr()
    nat.check(lib.dsp_bigru_forward_train(handle, x.data_ptr(), T, B, ptr(d_len), ptr(drop), o['y'].data_ptr(), o['hn'].data_ptr(),
                                          o['tape_ptr'], n.value, torch.cuda.current_stream(dev).cuda_stream))
    off = nat.c_i64(0)
    o['rows'] = []
    for l in range(L):
        nat.check(lib.dsp_bigru_tape_rows(handle, l, T, B, C.byref(off)))
        o['rows'].append(o['tape'][off.value // 4:off.value // 4 + T * B * 2 * H].view(T, B, 2 * H))
    return o


def _raw_backward(o, l, T, B, g, g_hn, da):
    """g, g_hn, da: pointers (or None)."""
    import torch
    from features import _native as nat
    return nat.load().dsp_bigru_backward(o['handle'], l, T, B, None if o['len'] is None else o['len'].data_ptr(), o['tape_ptr'],
                                         o['tape_bytes'], g, g_hn, da, torch.cuda.current_stream().cuda_stream)


def _raw_grads(m, o, x, T, B, g_y, g_hn, da_of=None):
    """Every layer's backward call and its GEMMs, top down -> (dx and the parameter gradients, the da of every layer)."""
    import torch
    from features import _native as nat
    from features.classifier import gru_param_grads
    H, L = m.hidden_size, m.gru.num_layers
    ps = [p.detach() for p in m._params()]
    grads, das, g = [None] * (1 + 8 * L), [None] * L, g_y
    for l in range(L - 1, -1, -1):
        da = torch.empty(T, B, 2, 4 * H, device=x.device) if da_of is None else da_of(l)
        nat.check(_raw_backward(o, l, T, B, g.data_ptr(), None if g_hn is None else g_hn[2 * l:].data_ptr(), da.data_ptr()))
        res = gru_param_grads(ps[8 * l:8 * l + 8], x if l == 0 else o['rows'][l - 1], o['rows'][l], da)
        grads[1 + 8 * l:9 + 8 * l], g, das[l] = res[1:], res[0], da
    grads[0] = g
    return grads, das


def test_full_lengths_with_a_null_length_pointer():
    """All-full lengths: against the fp64 route through the module, and d_len = NULL on raw pointers gives the same bits as
    the module's call with lengths T everywhere."""
    import torch
    dev = _dev()
    I, H, L, B, T = 13, 20, 3, 5, 3
    case = truth(I, H, L, B, T, lens_kind='full')
    got = check_against_truth(case, 'full lengths')
    m = copy.deepcopy(case['module']).to(dev)
    x = torch.from_numpy(case['x']).to(dev)
    o = _raw_train(m, x, T, B, d_len=None)
    raw, _ = _raw_grads(m, o, x, T, B, torch.from_numpy(case['w_y']).to(dev), torch.from_numpy(case['w_hn']).to(dev))
    for n, a, b in zip(names(L), raw, got):
        assert np.array_equal(a.cpu().numpy(), b), n


def test_each_loss_gradient_alone_and_their_sum():
    """g_y alone and g_hn alone (the other one reaches the kernel as NULL): each against the fp64 route, and the two parts add
    up to the combined call's gradients (the backward pass is linear in g; fp32 rounding under BAR)."""
    args = (13, 20, 3, 5, 3)
    parts = []
    for only in ('y', 'hn'):
        case = truth(*args, only=only)
        got, _, _ = device_grads(case, native=True)
        for n, v in rel_errors(got, case['ref'], 3).items():
            assert v <= hc.BAR, (only, n, v)
        parts.append(got)
    whole, _, _ = device_grads(truth(*args), native=True)
    for n, w, a, b in zip(names(3), whole, *parts):
        assert float(np.max(np.abs(a + b - w))) <= hc.BAR * float(np.max(np.abs(w))), n


@pytest.mark.parametrize('I,H,L,B,T', [(13, 20, 3, 5, 6), (39, 200, 2, 37, 24)])
def test_dropout_multipliers(I, H, L, B, T):
    """The same d_drop applied by hand between single-layer fp64 encoders on the CPU is the truth; a mask of all ones gives the
    bits of the NULL call."""
    case = truth(I, H, L, B, T, with_drop=True)
    assert 0.1 < float((case['drop'] == 0).mean()) < 0.3
    check_against_truth(case, f'dropout {I} -> {H} x {L}', with_gru_path=False)
    plain = dict(truth(I, H, L, B, T), drop=None)
    ones = dict(plain, drop=np.ones_like(case['drop']))
    a, b = device_grads(plain, native=True), device_grads(ones, native=True)
    for n, u, v in zip(names(L), a[0], b[0]):
        assert np.array_equal(u, v), n
    import torch
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize('I,H,L', [(13, 20, 3), (24, 100, 4), (39, 200, 2), (5, 256, 2)])
def test_forward_train_outputs_are_bitwise_those_of_forward(I, H, L):
    """One shape per forward instantiation, ragged lengths, B not a multiple of the slice."""
    import torch
    dev = _dev()
    B, T = 19, 7
    m = _module(I, H, L, 11).to(dev)
    x = torch.from_numpy(np.random.default_rng(12).standard_normal((T, B, I)).astype(np.float32)).to(dev)
    lens = np.random.default_rng(13).integers(1, T + 1, B)
    with torch.no_grad():
        y, hn = m.run(x, lens, native=True)
    yt, hnt = m.run(x.clone().requires_grad_(True), lens, native=True)
    assert yt.requires_grad and hnt.requires_grad and type(yt.grad_fn).__name__.startswith('_DynEncTrain')
    assert torch.equal(yt.detach(), y) and torch.equal(hnt.detach(), hn)


@pytest.mark.parametrize('B,T', [(37, 9), (16, 5), (1, 3)])
@pytest.mark.parametrize('I,H,L', [(13, 20, 3), (39, 200, 2)])
def test_canaries_full_writes_and_bitwise_repeatability(I, H, L, B, T):
    """The tape, d_da and the g buffers between sentinel words: the sentinels stay intact (nothing is written outside, the g
    buffers are not written at all), every element of d_da is written, and a second backward gives the same bits.  Error
    returns of the calls on a live handle: a tape one byte short, no gradient."""
    import torch
    from features import _native as nat
    from test_gpu_canaries import PAD, _guarded
    dev = _dev()
    m = _module(I, H, L, 7).to(dev)
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((T, B, I)).astype(np.float32)).to(dev)
    lens = np.random.default_rng(9).integers(1, T + 1, B)
    d_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    o = _raw_train(m, x, T, B, d_len, guarded=True)
    o['tape_check']('tape after forward_train')
    r = np.random.default_rng(10)
    gs = []
    for shp in ((T, B, H), (2 * L, B, H)):
        buf, p, check = _guarded(int(np.prod(shp)) * 4, dev)
        v = torch.from_numpy(r.standard_normal(shp).astype(np.float32)).to(dev)
        view = buf.view(torch.float32)[PAD // 4:PAD // 4 + v.numel()].view(shp)
        view.copy_(v)
        gs.append((view, check, v))
    runs = []
    for _ in range(2):
        guards = {}

        def da_of(l):
            buf, p, check = _guarded(T * B * 2 * 4 * H * 4, dev)
            guards[l] = check
            return buf.view(torch.float32)[PAD // 4:PAD // 4 + T * B * 8 * H].view(T, B, 2, 4 * H)

        _raw_grads(m, o, x, T, B, gs[0][0], gs[1][0], da_of)
        runs.append([guards[l](f'da of layer {l}').copy() for l in range(L)])
    for l in range(L):
        assert np.isfinite(runs[0][l].view(np.float32)).all(), f'da of layer {l} is not fully written'     # the fill is a NaN pattern
        assert np.array_equal(runs[0][l], runs[1][l]), f'da of layer {l} differs between two runs'
        da = runs[0][l].view(np.float32).reshape(T, B, 8 * H)
        for b in range(B):
            assert not da[lens[b]:, b].view(np.uint32).any(), (l, b)                                          # exact zeros behind the end
    o['tape_check']('tape after backward')
    for view, check, v in gs:
        assert np.array_equal(check('g').view(np.float32), v.cpu().numpy().ravel())
    lib = nat.load()
    da = torch.empty(T, B, 2, 4 * H, device=dev)
    short = dict(o, tape_bytes=o['tape_bytes'] - 1)
    assert _raw_backward(short, L - 1, T, B, gs[0][0].data_ptr(), None, da.data_ptr()) == nat.EINVAL and b'short' in lib.dsp_last_error()
    assert _raw_backward(o, L - 1, T, B, None, None, da.data_ptr()) == nat.EINVAL and b'no gradient' in lib.dsp_last_error()
    assert _raw_backward(o, L, T, B, gs[0][0].data_ptr(), None, da.data_ptr()) == nat.EINVAL and b'layer' in lib.dsp_last_error()


def test_graph_capture_of_forward_train_and_backward_replays_on_new_data():
    """forward_train and both layers' backward captured once (layer 0 on a given [T, B, 2 H] gradient, so that no GEMM sits in
    the capture) and replayed on new data: the bits of the eager calls."""
    import torch
    from features import _native as nat
    dev = _dev()
    I, H, L, B, T = 39, 200, 2, 19, 7
    m = _module(I, H, L, 7).to(dev)
    rng = np.random.default_rng(21)
    new = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)
    xs, g1s, g0s, ghs = ([new(*s) for _ in range(2)] for s in ((T, B, I), (T, B, H), (T, B, 2 * H), (2 * L, B, H)))
    d_len = torch.from_numpy(np.random.default_rng(22).integers(1, T + 1, B).astype(np.int32)).to(dev)

    def calls(o, x, g1, g0, gh, das, first=True):
        lib, st = nat.load(), torch.cuda.current_stream(dev).cuda_stream
        if not first:
            nat.check(lib.dsp_bigru_forward_train(o['handle'], x.data_ptr(), T, B, d_len.data_ptr(), None, o['y'].data_ptr(), o['hn'].data_ptr(),
                                                  o['tape_ptr'], o['tape_bytes'], st))
        nat.check(_raw_backward(o, 1, T, B, g1.data_ptr(), gh[2:].data_ptr(), das[1].data_ptr()))
        nat.check(_raw_backward(o, 0, T, B, g0.data_ptr(), gh.data_ptr(), das[0].data_ptr()))

    want = []
    for k in (0, 1):                                             # (also builds the handle and raises the LDS limit outside the capture)
        o = _raw_train(m, xs[k], T, B, d_len)
        das = [torch.empty(T, B, 2, 4 * H, device=dev) for _ in range(L)]
        calls(o, xs[k], g1s[k], g0s[k], ghs[k], das)
        torch.cuda.synchronize(dev)
        want.append((o['y'], o['hn'], das))
    x, g1, g0, gh = xs[0].clone(), g1s[0].clone(), g0s[0].clone(), ghs[0].clone()
    das = [torch.zeros(T, B, 2, 4 * H, device=dev) for _ in range(L)]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        o = _raw_train(m, x, T, B, d_len)                        # allocates its buffers outside the capture; runs once eagerly
        torch.cuda.synchronize(dev)
        with torch.cuda.graph(graph, stream=s):
            calls(o, x, g1, g0, gh, das, first=False)
    for k in (1, 0):
        x.copy_(xs[k]); g1.copy_(g1s[k]); g0.copy_(g0s[k]); gh.copy_(ghs[k])
        for v in das:
            v.zero_()
        o['tape'].zero_(); o['y'].zero_(); o['hn'].zero_()
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(o['y'], want[k][0]) and torch.equal(o['hn'], want[k][1])
        assert torch.equal(das[0], want[k][2][0]) and torch.equal(das[1], want[k][2][1])


# ---- the heads -----------------------------------------------------------------------------------------------------------

def _head_step(head, x, len0, w, **kw):
    head.zero_grad(set_to_none=True)
    lo = head(x, len0, **kw)
    lo = lo[0] if isinstance(lo, tuple) else lo
    (lo * w).sum().backward()
    return lo.detach(), {n: p.grad.detach().clone() for n, p in head.named_parameters()}


@pytest.mark.parametrize('kind', ['rnn', 'hmrnn'])
def test_head_training_step_on_the_native_encoder(kind):
    """RNNHead (39 -> 200 x 3) and HMRNNHead (without its dropouts, native HM-LSTM), B 8, T 30: logits and every parameter
    gradient with native_enc=True against native_enc=False on the same device."""
    import torch
    from features.classifier import RNNHead, fill_parameters
    from test_gpu_hmlstm_train import HEAD_SEED, _head_case
    dev = _dev()
    head, inp, len0, wl = _head_case(HEAD_SEED)
    kw = dict(dropout=False, native=True)
    if kind == 'rnn':
        torch.manual_seed(0)
        head, kw = RNNHead(), {}
        fill_parameters(head, HEAD_SEED)
    head = head.to(dev)
    x, w = torch.from_numpy(inp).to(dev), torch.from_numpy(wl).to(dev)
    res = {ne: _head_step(head, x, len0, w, native_enc=ne, **kw) for ne in (True, False)}
    if kind == 'hmrnn':                                          # HEAD_SEED's rule: no decision of the HM-LSTM inside the guard on this device
        with torch.no_grad():
            zh = head.enc2.run(head.enc1(x, len0), None, lens=len0, native=False).z_hat.cpu().numpy()
        assert (hc.cuts(zh) == zh.shape[0]).all(), 'the seed has a decision inside the guard on this device'
    d_lo = float((res[True][0] - res[False][0]).abs().max())
    worst = 0.0
    for n, g in res[True][1].items():
        ref = res[False][1][n]
        worst = max(worst, float((g - ref).abs().max() / ref.abs().max()))
    record(f'bigru_{kind}_head_grad_native_vs_gru_path', worst)
    print(f'{kind}: logits {d_lo:.3g}, worst parameter gradient {worst:.3g}')
    assert d_lo <= hc.BAR
    for n, g in res[True][1].items():
        ref = res[False][1][n]
        assert float((g - ref).abs().max() / ref.abs().max()) <= hc.BAR, n


def test_routing():
    import torch
    from features.classifier import _DynEnc
    dev = _dev()
    assert _DynEnc.native_train_default is False
    m = _module(13, 20, 2, 3).to(dev)
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((9, 5, 13)).astype(np.float32)).to(dev)
    lens = np.array([3, 9, 1, 5, 9])
    is_native = lambda t: type(t.grad_fn).__name__.startswith('_DynEncTrain')
    y, hn = m.run(x, lens)                                       # a gradient is required (the parameters'), native=None: nn.GRU
    assert y.requires_grad and not is_native(y) and not is_native(hn)
    y, hn = m.run(x, lens, native=True)
    assert is_native(y) and is_native(hn)
    assert not is_native(m.run(x, lens, native=False)[0])
    with pytest.raises(RuntimeError, match='not on a GPU'):
        m.cpu().run(x.cpu().requires_grad_(True), lens, native=True)
    m = m.to(dev)
    m.native_train_default = True                                # (an instance attribute: the class default stays False)
    try:
        assert is_native(m.run(x, lens)[0])
    finally:
        del m.native_train_default
    with torch.no_grad():                                        # without a gradient nothing changes
        a, b = m.run(x, lens, native=True), m.run(x, lens)
        assert not a[0].requires_grad and not b[0].requires_grad
    m.eval()                                                     # eval mode keeps its contract: a required gradient is a reason to decline
    with pytest.raises(RuntimeError, match='gradient'):
        m.run(x, lens, native=True)
    assert not is_native(m.run(x, lens)[0])
    m.train()
    # inter-layer dropout in training mode: the training path draws the multipliers, the no-gradient path still declines
    md = _DynEnc(13, 20, 2, dropout=0.2).to(dev).train()
    yd, _ = md.run(x, lens, native=True)
    assert is_native(yd) and torch.isfinite(yd).all()
    with torch.no_grad(), pytest.raises(RuntimeError, match='dropout'):
        md.run(x, lens, native=True)
    # a parameter written between forward and backward
    y, hn = m.run(x, lens, native=True)
    with torch.no_grad():
        m.gru.weight_hh_l0.mul_(1.0)
    with pytest.raises(RuntimeError, match='modified'):
        (y.sum() + hn.sum()).backward()
