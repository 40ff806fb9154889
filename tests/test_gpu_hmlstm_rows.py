"""The HM-LSTM's training pair under a row bound read on the device (include/dsp_frontend.h: dsp_hmlstm_forward_train_rows,
dsp_hmlstm_backward_rows; csrc/kernels_hmlstm.h, csrc/kernels_hmlstm_bwd.h; features/classifier.py::_HMLSTMTrain, HMLSTM.run
with ``d_rows``, HMRNNHead).

The contract is an equality, not a tolerance: with the word r behind ``d_rows`` the bounded call at T does, on the rows t < r,
the arithmetic of the plain call at T = r in the same order (one kernel, one template), and writes exact zeros behind.  So
everything here is compared under ``torch.equal`` / on the bit patterns.  Every buffer a test hands to a kernel is
pre-filled: floats with NaN, bytes with 0xFF, the tape with SENTINEL -- what a call does not write shows."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_hmlstm import SHAPES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0x7FC0BEEF                    # a quiet NaN's bit pattern, as int32
T0, B0 = 12, 20                          # shape b: two slices of 16 columns, the second partial
SUB = [1, 2, 4, 5, 7]                    # columns of tests/golden/rnn_golden.npz with lengths 57, 131, 12, 99, 64


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
    return m.to(_dev())


def _randn(rng, *shape):
    import torch
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(_dev())


def _state(rng, H1, H2, B):
    """The flat h1 | c1 | z1 | h2 | c2 | z2 buffer with random contents (z in {0, 1})."""
    import torch
    parts = [0.5 * rng.standard_normal(H1 * B), 0.5 * rng.standard_normal(H1 * B), rng.random(B) > 0.5,
             0.5 * rng.standard_normal(H2 * B), 0.5 * rng.standard_normal(H2 * B), rng.random(B) > 0.5]
    return torch.from_numpy(np.concatenate([np.asarray(p, dtype=np.float32) for p in parts])).to(_dev())


def _word(r):
    import torch
    return torch.tensor([r], dtype=torch.int32, device=_dev())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _buffers(m, T, B):
    import torch
    from features import _native as nat
    dev = _dev()
    H1, H2 = m.size_list
    handle, lib = m._native_handle(dev), nat.load()
    n = nat.c_i64(0)
    nat.check(lib.dsp_hmlstm_tape_bytes(handle, T, B, C.byref(n)))
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    ff = lambda *s: torch.full(s, 255, dtype=torch.uint8, device=dev)
    return dict(h1=nan(B, T, H1), h2=nan(B, T, H2), z1=ff(B, T), z2=ff(B, T), zhat=nan(T, 2, B), last=nan(B, H2),
                state=nan((2 * H1 + 2 * H2 + 2) * B), tape=torch.full((n.value // 4,), SENTINEL, dtype=torch.int32, device=dev),
                tape_bytes=n.value, handle=handle, T=T, B=B)


def _launch_forward(o, x, rows, stream):
    """``rows``: 'plain' -> dsp_hmlstm_forward_train; None or a one-element int32 tensor -> dsp_hmlstm_forward_train_rows."""
    from features import _native as nat
    lib = nat.load()
    tail = (_ptr(o['state_in']), o['state'].data_ptr(), o['h1'].data_ptr(), o['h2'].data_ptr(), o['z1'].data_ptr(), o['z2'].data_ptr(),
            o['zhat'].data_ptr(), o['last'].data_ptr(), o['tape'].data_ptr(), o['tape_bytes'], stream)
    head = (o['handle'], x.data_ptr(), o['T'], o['B'], 1.0, _ptr(o['len']))
    if isinstance(rows, str):
        nat.check(lib.dsp_hmlstm_forward_train(*head, *tail))
    else:
        nat.check(lib.dsp_hmlstm_forward_train_rows(*head, _ptr(rows), *tail))


def _launch_backward(o, g, dfs, rows, stream):
    from features import _native as nat
    lib = nat.load()
    tail = (_ptr(o['state_in']), o['tape'].data_ptr(), o['tape_bytes'], o['h1'].data_ptr(), o['h2'].data_ptr(), o['z1'].data_ptr(),
            o['z2'].data_ptr(), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), dfs[0].data_ptr(), dfs[1].data_ptr(), stream)
    head = (o['handle'], o['T'], o['B'], 1.0, _ptr(o['len']))
    if isinstance(rows, str):
        nat.check(lib.dsp_hmlstm_backward(*head, *tail))
    else:
        nat.check(lib.dsp_hmlstm_backward_rows(*head, _ptr(rows), *tail))


def _forward(m, x, lens, rows='plain', state_in=None):
    """One forward-train call on fresh pre-filled buffers.  x [T, B, I] contiguous, lens: numpy ints or None."""
    import torch
    T, B, _ = x.shape
    o = _buffers(m, T, B)
    o['len'] = None if lens is None else torch.as_tensor(np.asarray(lens), dtype=torch.int32).to(x.device)
    o['state_in'], o['rows'] = state_in, rows
    _launch_forward(o, x, rows, torch.cuda.current_stream(x.device).cuda_stream)
    torch.cuda.synchronize(x.device)
    return o


def _backward(m, o, g):
    """The backward call that belongs to ``o`` on fresh NaN-filled dfs1 / dfs2 -> [dfs1, dfs2]."""
    import torch
    dev = _dev()
    dfs = [torch.full((o['T'], o['B'], 4 * H + 1), float('nan'), dtype=torch.float32, device=dev) for H in m.size_list]
    _launch_backward(o, g, dfs, o['rows'], torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return dfs


def _bits(t):
    import torch
    return t if t.dtype in (torch.uint8, torch.int32) else t.contiguous().view(torch.int32)


def _all_zero_bits(t):
    return bool((_bits(t) == 0).all())


def _tape_steps(m, o):
    """The tape as [slices, T, floats per step] (int32 bit patterns)."""
    H1, H2 = m.size_list
    return o['tape'].view((o['B'] + 15) // 16, o['T'], 80 * (H1 + H2) + 32)


def _case_b():
    m = _module('b', 31)
    I, (H1, H2) = SHAPES['b']
    rng = np.random.default_rng(32)
    x = _randn(rng, T0, B0, I)
    lens = rng.integers(1, T0 + 1, B0)
    lens[3], lens[17] = T0, 1                                   # the extremes, one in each slice
    st = _state(rng, H1, H2, B0)
    g = [_randn(rng, B0, T0, H1), _randn(rng, B0, T0, H2), _randn(rng, B0, H2)]
    return m, x, lens, st, g


def _short_g(g, r):
    return [g[0][:, :r].contiguous(), g[1][:, :r].contiguous(), g[2]]


def _nan_behind(g, r):
    g1, g2 = g[0].clone(), g[1].clone()
    g1[:, r:] = float('nan')
    g2[:, r:] = float('nan')
    return [g1, g2, g[2]]


def _check_forward(m, got, short, r):
    import torch
    assert torch.equal(got['state'], short['state']) and torch.equal(got['last'], short['last'])
    assert bool(torch.isfinite(got['last']).all()) and bool(torch.isfinite(got['state']).all())
    for k in ('h1', 'h2', 'z1', 'z2'):
        assert torch.equal(_bits(got[k][:, :r]), _bits(short[k])), k
        assert _all_zero_bits(got[k][:, r:]), f'{k} behind row {r}'
    assert torch.equal(_bits(got['zhat'][:r]), _bits(short['zhat'])) and _all_zero_bits(got['zhat'][r:])
    assert bool(torch.isfinite(got['h1']).all()) and bool(torch.isfinite(got['h2']).all()) and bool(torch.isfinite(got['zhat']).all())
    # the stop is real: the steps behind r keep the sentinel, the steps in front are the short call's (the stride stays T)
    tape, tape_s = _tape_steps(m, got), _tape_steps(m, short)
    assert bool((tape[:, r:] == SENTINEL).all()), 'tape steps behind the bound were written'
    assert torch.equal(tape[:, :r], tape_s)
    assert not bool((tape_s == SENTINEL).any()), 'the tape of the steps that ran has unwritten words'


def _check_backward(got, short, r):
    import torch
    for k in (0, 1):
        assert torch.equal(_bits(got[k][:r]), _bits(short[k])), f'dfs{k + 1}'
        assert _all_zero_bits(got[k][r:]), f'dfs{k + 1} behind row {r}'
        assert bool(torch.isfinite(got[k]).all()), f'dfs{k + 1}'


@pytest.mark.parametrize('with_state', [True, False])
@pytest.mark.parametrize('r', [1, 5, 11, 12])
def test_bounded_pair_equals_the_short_pair_bitwise(r, with_state):
    """Assertions 1 - 3 of the contract at shape b, T 12, B 20: forward outputs, state, last_h2 and tape of the rows < r equal
    the plain call at T = r, zeros behind, the tape's steps >= r untouched; the backward with g_h1 / g_h2 NaN behind r gives
    the short call's dfs in front of r and exact zeros behind."""
    m, x, lens, st, g = _case_b()
    st = st if with_state else None
    got = _forward(m, x, lens, _word(r), st)
    short = _forward(m, x[:r].contiguous(), np.minimum(lens, r), 'plain', st)
    _check_forward(m, got, short, r)
    _check_backward(_backward(m, got, _nan_behind(g, r)), _backward(m, short, _short_g(g, r)), r)


def _same_pair(m, a, da, b, db):
    import torch
    for k in ('state', 'last', 'h1', 'h2', 'z1', 'z2', 'zhat', 'tape'):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    for k in (0, 1):
        assert torch.equal(_bits(da[k]), _bits(db[k])), f'dfs{k + 1}'


@pytest.mark.parametrize('word,means', [(0, 1), (-7, 1), (99, T0), (-2 ** 31, 1), (2 ** 31 - 1, T0)])
def test_the_word_is_clamped_to_1_T(word, means):
    m, x, lens, st, g = _case_b()
    g = _nan_behind(g, means)
    a = _forward(m, x, lens, _word(word), st)
    b = _forward(m, x, lens, _word(means), st)
    _same_pair(m, a, _backward(m, a, g), b, _backward(m, b, g))
    if means == T0:                                             # ... and r = T is the plain call
        c = _forward(m, x, lens, 'plain', st)
        _same_pair(m, a, _backward(m, a, g), c, _backward(m, c, g))


def test_null_rows_is_the_plain_pair_bitwise():
    m, x, lens, st, g = _case_b()
    a = _forward(m, x, lens, None, st)                          # the _rows entry points with d_rows = NULL
    b = _forward(m, x, lens, 'plain', st)
    _same_pair(m, a, _backward(m, a, g), b, _backward(m, b, g))
    assert not bool((a['tape'] == SENTINEL).any())


def test_production_shape_once():
    """Input 200, sizes (200, 200), T 200, B 5, lengths up to 90, the word 90: last_h2, dfs1 and dfs2."""
    import torch
    m = _module('a', 41)
    T, B, r = 200, 5, 90
    rng = np.random.default_rng(42)
    x = _randn(rng, T, B, 200)
    lens = np.array([57, 90, 12, 88, 64])
    g = [None, None, _randn(rng, B, 200)]
    got = _forward(m, x, lens, _word(r))
    short = _forward(m, x[:r].contiguous(), lens, 'plain')
    assert torch.equal(got['last'], short['last']) and bool(torch.isfinite(got['last']).all())
    _check_backward(_backward(m, got, g), _backward(m, short, g), r)


def test_graph_replays_follow_the_word():
    """forward-train-rows + backward-rows as a graph of two launches: the word is written between replays, and each replay is
    the eager pair at that value.  During the capture the word holds a third value, which no replay shows."""
    import torch
    m, x, lens, st, g = _case_b()
    dev = _dev()
    want = {}
    for r in (5, 11):
        o = _forward(m, x, lens, _word(r), st)                  # (also builds the handle and raises the LDS limit outside the capture)
        want[r] = (o, _backward(m, o, g))
    word = _word(3)
    o = _buffers(m, T0, B0)
    o['len'] = torch.as_tensor(lens, dtype=torch.int32).to(dev)
    o['state_in'] = st
    dfs = [torch.full((T0, B0, 4 * H + 1), float('nan'), dtype=torch.float32, device=dev) for H in m.size_list]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            st_ptr = torch.cuda.current_stream(dev).cuda_stream
            _launch_forward(o, x, word, st_ptr)
            _launch_backward(o, g, dfs, word, st_ptr)
    torch.cuda.synchronize(dev)
    assert bool((o['tape'] == SENTINEL).all()) and bool(torch.isnan(dfs[0]).all()), 'the capture ran the kernels'
    for r in (11, 5):
        word.fill_(r)
        o['tape'].fill_(SENTINEL)
        for v in dfs:
            v.fill_(float('nan'))
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        _same_pair(m, o, dfs, *want[r])


class _NanEmpty:
    """torch.empty with the float results NaN-filled and the byte results 0xFF-filled: an element a kernel leaves unwritten shows."""

    def __init__(self, torch):
        self.torch, self.real = torch, torch.empty

    def __call__(self, *a, **kw):
        t = self.real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float('nan'))
        elif t.is_cuda and t.dtype == self.torch.uint8:
            t.fill_(255)
        return t


def test_head_with_the_bound_equals_the_head_without(monkeypatch):
    """HMRNNHead, dropout=False, B 5, inp [200, 5, 39], lengths up to 131, device_len=True, device_grad=True: logits, feat and
    every parameter gradient (and the input's) equal under == those of the same head whose HMLSTM.run drops ``d_rows`` -- the
    unbounded backward leaves zeros behind the longest clip, so nothing but the sign of a zero can differ.  Every
    ``torch.empty`` buffer is NaN-filled: the bounded kernels' zero fill is what keeps ``hm_param_grads`` finite."""
    import torch
    from features import classifier as Cl
    import hmrnn_cases as hc
    dev = _dev()
    rg = np.load(os.path.join(HERE, 'golden', 'rnn_golden.npz'))
    len0 = np.asarray(rg['len0'])[SUB]
    assert len0.tolist() == [57, 131, 12, 99, 64] and rg['inp'].shape[0] == 200
    inp = torch.from_numpy(np.ascontiguousarray(rg['inp'][:, SUB])).to(dev)
    len_d = torch.from_numpy(len0.astype(np.int32)).to(dev)
    torch.manual_seed(0)
    head = Cl.HMRNNHead().train()
    Cl.fill_parameters(head, int(hc.load_golden()['head_seed']))
    head = head.to(dev)

    seen = []

    class Unbounded(Cl.HMLSTM):
        def run(self, *a, d_rows=None, **kw):
            seen.append(d_rows)
            return Cl.HMLSTM.run(self, *a, **kw)

    monkeypatch.setattr(torch, 'empty', _NanEmpty(torch))

    def step():
        x = inp.clone().requires_grad_(True)
        head.zero_grad(set_to_none=True)
        torch.manual_seed(5)                                    # the GRU's inter-layer multipliers: the same on both sides
        logits, feat = head(x, len_d, dropout=False, device_len=True, device_grad=True)
        logits.square().sum().backward()
        return [logits.detach(), feat.detach(), x.grad] + [p.grad.clone() for p in head.parameters()]

    got = step()
    head.enc2.__class__ = Unbounded
    try:
        ref = step()
    finally:
        head.enc2.__class__ = Cl.HMLSTM
    assert len(seen) == 1 and seen[0] is not None and seen[0].dtype == torch.int32 and seen[0].numel() == 1
    assert int(seen[0].item()) == 131
    names = ['logits', 'feat', 'inp'] + [n for n, _ in head.named_parameters()]
    for n, a, b in zip(names, got, ref):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), n
        assert bool((a == b).all()), (n, float((a - b).abs().max()))
    assert float(got[2][131:].abs().max()) == 0.0               # nothing reaches the rows behind the longest clip


def test_d_rows_is_checked():
    import torch
    m = _module('b', 31)
    x = _randn(np.random.default_rng(1), 4, 3, 24).requires_grad_(True)
    lens = torch.tensor([4, 2, 1], dtype=torch.int32, device=_dev())
    with pytest.raises(ValueError, match='d_rows needs'):
        m.run(x, lens=lens, device_len=True, d_rows=_word(4))
    with pytest.raises(TypeError, match='one-element int32'):
        m.run(x, lens=lens, device_len=True, device_grad=True, d_rows=torch.tensor([4, 4], dtype=torch.int32, device=_dev()))
    with pytest.raises(TypeError, match='one-element int32'):
        m.run(x, lens=lens, device_len=True, device_grad=True, d_rows=4)
    a = m.run(x, lens=lens, device_len=True, device_grad=True, d_rows=_word(4)).last_h2
    b = m.run(x, lens=lens, device_len=True, device_grad=True).last_h2
    assert a.requires_grad and torch.equal(a.detach(), b.detach())
