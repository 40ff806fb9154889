"""The native HM-LSTM training path on the GPU (dsp_hmlstm_forward_train + dsp_hmlstm_backward, csrc/kernels_hmlstm_bwd.h,
features/classifier.py::_HMLSTMTrain): gradients against the fp64 step loop on the CPU with the same weights, the
properties of the two calls (optional gradients, state, lengths, bitwise repeatability, buffer edges, graph capture), the
whole HMRNNHead training step and the routing.

The threshold rule of tests/hmrnn_cases.py extended to gradients: a batch column is KEPT if the fp64 loop holds, in that
column, no decision inside GUARD of 0.5 (the bit may fall either way in fp32) and no unsaturated z_hat within GUARD of 0
or 1 (the clamp's mask may).  The loss is a random-weighted sum of h_1, h_2 and last_h2 over kept columns only; columns
are independent, so a dropped column contributes nothing to any gradient on either side.  At most 10 % of the columns
may be dropped."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import hmrnn_cases as hc
from conftest import record
from test_gpu_hmlstm import SHAPES as FORWARD_SHAPES

# e: one cell needs two chunks of owner slots per wave, the other one (the backward kernel's mixed case)
SHAPES = dict(FORWARD_SHAPES, e=(24, (132, 64)))
pytestmark = pytest.mark.gpu

NAMES = ('x', 'cell_1.U_11', 'cell_1.U_21', 'cell_1.W_01', 'cell_1.bias', 'cell_2.U_11', 'cell_2.W_01', 'cell_2.bias')
MAX_DROPPED = 0.10
# (B, T, shape, seed): the first seed from 20260900 at which the fp64 loop on the CPU drops no column under the rule above
# (tools/kbench_hmlstm.py --scan-train-seeds prints the table with the boundary rates).  b has cell 2 always flushing; c, d
# and a have mixed boundary rates and saturated z_hat.  B = 1, B not a multiple of 16, T = 1, more than one slice.
GRAD_CASES = [
    (1, 1, 'b', 20260900), (5, 3, 'b', 20260900), (37, 24, 'b', 20260900),
    (19, 7, 'c', 20260900), (16, 12, 'd', 20260900), (8, 40, 'a', 20260900), (21, 5, 'e', 20260900),
]
HEAD_SEED = 20260905      # HMRNNHead, B 8, T 30: no decision of the fp32 loop on the CPU within 1e-3 of 0.5 (same scan)


def _dev():
    import torch
    return torch.device('cuda', 0)


def _module(shape, seed):
    import torch
    from features.classifier import HMLSTM, fill_parameters
    I, sizes = SHAPES[shape]
    torch.manual_seed(0)
    m = HMLSTM(1.0, I, list(sizes))
    fill_parameters(m, seed)
    return m


def kept_columns(z_hat, g=hc.GUARD):
    """z_hat [T, 2, B] of the fp64 loop -> bool [B]."""
    z = np.asarray(z_hat, dtype=np.float64)
    bad = (np.abs(z - 0.5) < g) | ((z > 0) & (z < g)) | ((z < 1) & (z > 1 - g))
    return ~bad.any(axis=(0, 1))


@functools.lru_cache(maxsize=None)
def truth(B, T, shape, seed, with_state=False, lens_kind='ragged', only=None):
    """The case's inputs (float32) and the gradients of the fp64 loop on the CPU.  Computed once, shared, never modified."""
    import torch
    I, (H1, H2) = SHAPES[shape]
    m = _module(shape, seed)
    x = np.random.default_rng(seed + 1).standard_normal((T, B, I)).astype(np.float32)
    lens = np.random.default_rng(seed + 2).integers(1, T + 1, B)
    if lens_kind == 'edges':
        lens[0], lens[-1] = 1, T
    state = None
    if with_state:
        r = np.random.default_rng(seed + 3)
        val = lambda n: (0.5 * r.standard_normal((n, B))).astype(np.float32)
        bit = lambda: (r.random((1, B)) > 0.5).astype(np.float32)
        state = (val(H1), val(H1), bit(), val(H2), val(H2), bit())
    r = np.random.default_rng(seed + 4)
    w = [r.standard_normal(s).astype(np.float32) for s in ((B, T, H1), (B, T, H2), (B, H2))]
    m64 = copy.deepcopy(m).double()
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    st64 = None if state is None else tuple(torch.from_numpy(v).double() for v in state)
    res = m64._run_torch(x64, st64, lens)
    keep = kept_columns(res.z_hat.numpy())
    w = [v * keep.reshape((B,) + (1,) * (v.ndim - 1)).astype(np.float32) for v in w]
    if only is not None:
        w = [v if k == only else None for k, v in enumerate(w)]
    loss = sum((o * torch.from_numpy(v).double()).sum() for o, v in zip((res.h_1, res.h_2, res.last_h2), w) if v is not None)
    ps = [x64] + m64._params()
    ref = [np.zeros(tuple(p.shape)) if g is None else g.numpy() for p, g in zip(ps, torch.autograd.grad(loss, ps, allow_unused=True))]
    rates = (float((res.z_hat[:, 0] > 0.5).double().mean()), float((res.z_hat[:, 1] > 0.5).double().mean()))
    return dict(module=m, x=x, lens=lens, state=state, w=w, keep=keep, ref=ref, rates=rates)


def device_grads(case, native, dev=None):
    """-> (gradients of x and the seven parameters as numpy, the HMLSTMResult) of the fp32 module on the device."""
    import torch
    dev = dev or _dev()
    m = copy.deepcopy(case['module']).to(dev)
    x = torch.from_numpy(case['x']).to(dev).requires_grad_(True)
    st = None if case['state'] is None else tuple(torch.from_numpy(v).to(dev) for v in case['state'])
    r = m.run(x, st, lens=case['lens'], native=native)
    loss = sum((o * torch.from_numpy(v).to(dev)).sum() for o, v in zip((r.h_1, r.h_2, r.last_h2), case['w']) if v is not None)
    grads = torch.autograd.grad(loss, [x] + m._params(), allow_unused=True)
    return [np.zeros(tuple(p.shape), np.float32) if g is None else g.detach().cpu().numpy() for p, g in zip([x] + m._params(), grads)], r


def rel_errors(got, ref):
    """max |got - ref| / max |ref| per tensor (the absolute deviation where the reference gradient is identically zero)."""
    return {n: float(np.max(np.abs(a.astype(np.float64) - b))) / (float(np.max(np.abs(b))) or 1.0) for n, a, b in zip(NAMES, got, ref)}


def check_against_truth(case, tag):
    assert 1.0 - case['keep'].mean() <= MAX_DROPPED, 'the seed drops too many columns'
    got, _ = device_grads(case, native=True)
    loop, _ = device_grads(case, native=False)
    e_nat, e_loop = rel_errors(got, case['ref']), rel_errors(loop, case['ref'])
    worst, worst_loop = max(e_nat.values()), max(e_loop.values())
    record('hmlstm_grad_native_vs_fp64', worst)
    record('hmlstm_grad_torch_loop_vs_fp64', worst_loop)
    print(f'{tag}: boundary rates {case["rates"][0]:.2f} / {case["rates"][1]:.2f}, dropped {int((~case["keep"]).sum())}, '
          f'native {worst:.3g}, device loop {worst_loop:.3g}: ' + ', '.join(f'{n} {v:.2g}' for n, v in e_nat.items()))
    for n, v in e_nat.items():
        assert v <= hc.BAR, (n, v)


@pytest.mark.parametrize('B,T,shape,seed', GRAD_CASES)
def test_gradients_equal_the_fp64_loop(B, T, shape, seed):
    """dx and the seven parameter gradients, max |got - ref| / max |ref| <= BAR per tensor; the device loop's own error is
    recorded beside the native path's."""
    check_against_truth(truth(B, T, shape, seed), f'B {B} T {T} {shape}')


def test_nonzero_initial_state():
    check_against_truth(truth(19, 7, 'c', 20260900, with_state=True), 'state_in')


def test_lengths_one_and_T():
    case = truth(19, 7, 'c', 20260900, lens_kind='edges')
    assert case['lens'][0] == 1 and case['lens'][-1] == 7 and case['keep'][0] and case['keep'][-1]
    check_against_truth(case, 'len 1 and len T')


def test_each_loss_gradient_alone_and_their_sum():
    """g_h1, g_h2 and g_last one at a time (the other two reach the kernel as NULL): each against the fp64 loop, and the
    three parts add up to the combined call's gradients (the backward pass is linear in g; fp32 rounding under BAR)."""
    args = (5, 3, 'b', 20260900)
    parts = []
    for only in (0, 1, 2):
        case = truth(*args, only=only)
        got, _ = device_grads(case, native=True)
        for n, v in rel_errors(got, case['ref']).items():
            assert v <= hc.BAR, (only, n, v)
        parts.append(got)
    whole, _ = device_grads(truth(*args), native=True)
    for n, w, a, b, c in zip(NAMES, whole, *parts):
        assert float(np.max(np.abs(a + b + c - w))) <= hc.BAR * float(np.max(np.abs(w))), n


def _raw_train(m, x, lens=None, state_in=None, guarded=False):
    """dsp_hmlstm_forward_train on raw pointers -> dict of buffers (torch tensors; with ``guarded`` the tape sits between
    sentinel words and 'tape_check' verifies them)."""
    import torch
    from features import _native as nat
    from test_gpu_canaries import _guarded
    dev = x.device
    T, B, _ = x.shape
    H1, H2 = m.size_list
    handle, lib = m._native_handle(dev), nat.load()
    n = nat.c_i64(0)
    nat.check(lib.dsp_hmlstm_tape_bytes(handle, T, B, C.byref(n)))
    f32 = dict(dtype=torch.float32, device=dev)
    o = dict(h1=torch.empty(B, T, H1, **f32), h2=torch.empty(B, T, H2, **f32), z1=torch.empty(B, T, dtype=torch.uint8, device=dev),
             z2=torch.empty(B, T, dtype=torch.uint8, device=dev), zhat=torch.empty(T, 2, B, **f32), last=torch.empty(B, H2, **f32),
             state=torch.empty((2 * H1 + 2 * H2 + 2) * B, **f32), tape_bytes=n.value, handle=handle)
    if guarded:
        o['tape_buf'], o['tape_ptr'], o['tape_check'] = _guarded(n.value, dev)
    else:
        o['tape_buf'] = torch.empty(n.value // 4, **f32)
        o['tape_ptr'] = o['tape_buf'].data_ptr()
    o['len'] = None if lens is None else torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(dev)
    o['state_in'] = state_in
    ptr = lambda t: None if t is None else t.data_ptr()
    nat.check(lib.dsp_hmlstm_forward_train(handle, x.data_ptr(), T, B, 1.0, ptr(o['len']), ptr(state_in), o['state'].data_ptr(),
                                           o['h1'].data_ptr(), o['h2'].data_ptr(), o['z1'].data_ptr(), o['z2'].data_ptr(),
                                           o['zhat'].data_ptr(), o['last'].data_ptr(), o['tape_ptr'], n.value,
                                           torch.cuda.current_stream(dev).cuda_stream))
    return o


def _raw_backward(o, T, B, g, dfs):
    """g: three pointers (or None), dfs: two pointers."""
    import torch
    from features import _native as nat
    ptr = lambda t: None if t is None else t.data_ptr()
    return nat.load().dsp_hmlstm_backward(o['handle'], T, B, 1.0, ptr(o['len']), ptr(o['state_in']), o['tape_ptr'], o['tape_bytes'],
                                          o['h1'].data_ptr(), o['h2'].data_ptr(), o['z1'].data_ptr(), o['z2'].data_ptr(), *g, *dfs,
                                          torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('shape', ['a', 'b', 'c', 'd'])
def test_forward_train_outputs_are_bitwise_those_of_forward(shape):
    """All four instantiations, ragged lengths, a non-zero initial state, B not a multiple of the slice."""
    import torch
    dev = _dev()
    B, T = 19, 7
    I, (H1, H2) = SHAPES[shape]
    m = _module(shape, 11).to(dev)
    x = torch.from_numpy(np.random.default_rng(12).standard_normal((T, B, I)).astype(np.float32)).to(dev)
    lens = np.random.default_rng(13).integers(1, T + 1, B)
    r = np.random.default_rng(14)
    hid = tuple(torch.from_numpy(v.astype(np.float32)).to(dev) for v in
                (0.5 * r.standard_normal((H1, B)), 0.5 * r.standard_normal((H1, B)), r.random((1, B)) > 0.5,
                 0.5 * r.standard_normal((H2, B)), 0.5 * r.standard_normal((H2, B)), r.random((1, B)) > 0.5))
    with torch.no_grad():
        want = m.run(x, hid, lens=lens, native=True)
    got = m.run(x.clone().requires_grad_(True), hid, lens=lens, native=True)
    assert got.h_2.requires_grad and got.h_1.requires_grad and got.last_h2.requires_grad
    assert not got.z_1.requires_grad and not got.z_hat.requires_grad and not got.hidden[0].requires_grad
    for k in ('h_1', 'h_2', 'z_1', 'z_2', 'z_hat', 'last_h2'):
        assert torch.equal(getattr(got, k).detach(), getattr(want, k)), k
    for a, b in zip(got.hidden, want.hidden):
        assert torch.equal(a, b)


@pytest.mark.parametrize('B,T,shape', [(37, 9, 'b'), (16, 5, 'c'), (1, 3, 'a'), (50, 4, 'd')])
def test_canaries_full_writes_and_bitwise_repeatability(B, T, shape):
    """The tape, dfs1 / dfs2 and the three g buffers between sentinel words: the sentinels stay intact (nothing is written
    outside, the g buffers are not written at all), every element of dfs is written, and a second backward call gives the
    same bits.  Error returns of the calls on a live handle: a tape one byte short, no gradient."""
    import torch
    from features import _native as nat
    from test_gpu_canaries import _guarded
    dev = _dev()
    I, (H1, H2) = SHAPES[shape]
    m = _module(shape, 7).to(dev)
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((T, B, I)).astype(np.float32)).to(dev)
    lens = np.random.default_rng(9).integers(1, T + 1, B)
    o = _raw_train(m, x, lens, guarded=True)
    o['tape_check']('tape after forward_train')
    r = np.random.default_rng(10)
    gs = []
    for shp in ((B, T, H1), (B, T, H2), (B, H2)):
        buf, p, check = _guarded(int(np.prod(shp)) * 4, dev)
        v = torch.from_numpy(r.standard_normal(shp).astype(np.float32)).to(dev)
        buf.view(torch.uint8)[4096:4096 + v.numel() * 4] = v.view(-1).view(torch.uint8)
        gs.append((buf, p, check, v))
    runs = []
    for _ in range(2):
        d = [_guarded(T * B * (4 * H + 1) * 4, dev) for H in (H1, H2)]
        nat.check(_raw_backward(o, T, B, [g[1] for g in gs], [v[1] for v in d]))
        runs.append([v[2](f'dfs{k + 1}').copy() for k, v in enumerate(d)])
    for k in (0, 1):
        assert np.isfinite(runs[0][k].view(np.float32)).all(), f'dfs{k + 1} is not fully written'     # the fill is a NaN pattern
        assert np.array_equal(runs[0][k], runs[1][k]), f'dfs{k + 1} differs between two runs'
    o['tape_check']('tape after backward')
    for buf, p, check, v in gs:
        assert np.array_equal(check('g').view(np.float32), v.cpu().numpy().ravel())
    lib = nat.load()
    d = [torch.empty(T, B, 4 * H + 1, device=dev) for H in (H1, H2)]
    short = dict(o, tape_bytes=o['tape_bytes'] - 1)
    assert _raw_backward(short, T, B, [g[1] for g in gs], [v.data_ptr() for v in d]) == nat.EINVAL and b'short' in lib.dsp_last_error()
    assert _raw_backward(o, T, B, [None] * 3, [v.data_ptr() for v in d]) == nat.EINVAL and b'no gradient' in lib.dsp_last_error()


def test_graph_capture_of_forward_train_and_backward_replays_on_new_data():
    import torch
    from features import _native as nat
    dev = _dev()
    B, T, shape = 19, 7, 'c'
    I, (H1, H2) = SHAPES[shape]
    m = _module(shape, 7).to(dev)
    rng = np.random.default_rng(21)
    new = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)
    xs, g1s, g2s = [new(T, B, I) for _ in range(2)], [new(B, T, H1) for _ in range(2)], [new(B, T, H2) for _ in range(2)]

    def eager(k):
        o = _raw_train(m, xs[k])
        d = [torch.empty(T, B, 4 * H + 1, device=dev) for H in (H1, H2)]
        nat.check(_raw_backward(o, T, B, [g1s[k].data_ptr(), g2s[k].data_ptr(), None], [v.data_ptr() for v in d]))
        torch.cuda.synchronize(dev)
        return o['h2'], d

    want = [eager(0), eager(1)]                                  # (also builds the handle and raises the LDS limit outside the capture)
    x, g1, g2 = xs[0].clone(), g1s[0].clone(), g2s[0].clone()
    d = [torch.zeros(T, B, 4 * H + 1, device=dev) for H in (H1, H2)]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        o = _raw_train(m, x)                                     # allocates its buffers outside the capture; runs once eagerly
        torch.cuda.synchronize(dev)
        with torch.cuda.graph(graph, stream=s):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(nat.load().dsp_hmlstm_forward_train(o['handle'], x.data_ptr(), T, B, 1.0, None, None, o['state'].data_ptr(),
                                                          o['h1'].data_ptr(), o['h2'].data_ptr(), o['z1'].data_ptr(), o['z2'].data_ptr(),
                                                          o['zhat'].data_ptr(), o['last'].data_ptr(), o['tape_ptr'], o['tape_bytes'], st))
            nat.check(nat.load().dsp_hmlstm_backward(o['handle'], T, B, 1.0, None, None, o['tape_ptr'], o['tape_bytes'], o['h1'].data_ptr(),
                                                     o['h2'].data_ptr(), o['z1'].data_ptr(), o['z2'].data_ptr(), g1.data_ptr(), g2.data_ptr(),
                                                     None, d[0].data_ptr(), d[1].data_ptr(), st))
    for k in (1, 0):
        x.copy_(xs[k]); g1.copy_(g1s[k]); g2.copy_(g2s[k])
        for v in d:
            v.zero_()
        o['tape_buf'].zero_(); o['h2'].zero_()
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(o['h2'], want[k][0])
        assert torch.equal(d[0], want[k][1][0]) and torch.equal(d[1], want[k][1][1])


def _head_case(seed=HEAD_SEED):
    import torch
    from features.classifier import HMRNNHead, fill_parameters
    torch.manual_seed(0)
    head = HMRNNHead()
    fill_parameters(head, seed)
    B, T = 8, 30
    inp = np.random.default_rng(seed + 1).standard_normal((T, B, 39)).astype(np.float32)
    len0 = np.random.default_rng(seed + 2).integers(5, T + 1, B)
    len0[0] = T
    for b in range(B):
        inp[len0[b]:, b] = 0.0
    wl = np.random.default_rng(seed + 3).standard_normal((B, 20)).astype(np.float32)
    return head, inp, len0, wl


def test_head_training_step_native_equals_the_loop():
    """HMRNNHead without its dropouts, B 8, T 30: logits under the forward bar, every parameter gradient -- enc1.gru.* included,
    which the head reaches through dx -- under the gradient bar, native=True against native=False on the same device."""
    import torch
    dev = _dev()
    head, inp, len0, wl = _head_case()
    head = head.to(dev)
    x, w = torch.from_numpy(inp).to(dev), torch.from_numpy(wl).to(dev)
    res = {}
    for native in (True, False):
        head.zero_grad(set_to_none=True)
        lo, _ = head(x, len0, dropout=False, native=native)
        (lo * w).sum().backward()
        res[native] = (lo.detach(), {n: p.grad.detach().clone() for n, p in head.named_parameters()})
    with torch.no_grad():
        enc = head.enc1(x, len0)
        zh = head.enc2.run(enc, None, lens=len0, native=False).z_hat.cpu().numpy()
    assert (hc.cuts(zh) == zh.shape[0]).all(), 'the seed has a decision inside the guard on this device'
    assert float((res[True][0] - res[False][0]).abs().max()) <= hc.BAR
    worst = 0.0
    for n, g in res[True][1].items():
        ref = res[False][1][n]
        err = float((g - ref).abs().max() / ref.abs().max())
        worst = max(worst, err)
        assert err <= hc.BAR, (n, err)
    record('hmrnn_head_grad_native_vs_torch_loop', worst)


def test_routing():
    import torch
    dev = _dev()
    from features.classifier import HMLSTM
    assert HMLSTM.native_train_default is False
    m = _module('b', 3).to(dev)
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((5, 3, 24)).astype(np.float32)).to(dev)
    loop = m.run(x)                                              # a gradient is required (the parameters'), native=None: the loop
    assert loop.h_2.requires_grad and loop.z_1.requires_grad     # (only the loop's z carries the straight-through gradient)
    nat_r = m.run(x, native=True)
    assert nat_r.h_2.requires_grad and not nat_r.z_1.requires_grad and type(nat_r.h_2.grad_fn).__name__.startswith('_HMLSTMTrain')
    hid = tuple(v.detach().clone() for v in nat_r.hidden)
    assert m.run(x, hid, native=True).h_2.requires_grad          # a detached state is fine
    hid[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match='initial hidden requires a gradient'):
        m.run(x, hid, native=True)
    assert m.run(x, hid).h_2.requires_grad                       # native=None: the loop serves it
    with pytest.raises(RuntimeError, match='not on a GPU'):
        m.run(x.cpu().requires_grad_(True), native=True)
    m.native_train_default = True                                # (an instance attribute: the class default stays False)
    try:
        assert type(m.run(x).h_2.grad_fn).__name__.startswith('_HMLSTMTrain')
    finally:
        del m.native_train_default
    with torch.no_grad():
        assert not m.run(x).h_2.requires_grad                    # without a gradient nothing changes: the forward kernel
