"""The native attention blocks on the device (csrc/kernels_attn.h): the Transformer encoder layer (``dsp_attn_forward``) and the
SelfAttn pooling (``dsp_selfattn_pool_batch``).

Three kinds of evidence:
  * pinned to the REAL reference: TransformerHead / HRNNAttHead with ``native_attn=True`` against tests/golden/clf_golden.npz, at
    the bar tests/test_classifier_golden.py uses on the device (2e-4 max(1, |ref|), 200 x that for the sum over time);
  * parity of the blocks against their fp64 stand-ins on the CPU at 2e-5 max(1, |ref|) -- the project's bar for these stand-ins
    and for the recurrent kernels; fp32 arithmetic of this depth sits two orders below it -- on the smallest shapes at which
    the kernels can go wrong: both LayerNorm skips (T = 1, B = 1), ragged 16-row tiles, more than one tile in t and u, more
    batch columns than statistics waves, an odd d_model, d_k != d_v, scores beyond +-88;
  * mechanics: the same bits twice, on a view, on a side stream and from a replayed graph; canaries behind every buffer the
    launches write; a parameter written in place rebuilds the handle.
"""
import copy
import os

import numpy as np
import pytest

from conftest import record

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 2e-5
DIMS = {'head': (39, 200, 100, 100), 'small': (6, 8, 4, 12)}          # d_model, d_inner, d_k, d_v
SHAPES = [(1, 3), (5, 1), (17, 2), (33, 17), (200, 3)]                # (T, B)


def _dev():
    import torch
    return torch.device('cuda', 0)


def _err(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


def _fill(mod, seed, fill='wide'):
    """'golden': the project's fill_parameters, uniform(-0.08, 0.08) everywhere, as the golden fixtures fill the heads (small
    scores: a nearly flat softmax).  'wide': matrices uniform(-0.3, 0.3) (scores of order one: a softmax that is neither flat
    nor one-hot) and LayerNorm gains near 1."""
    import torch
    if fill == 'golden':
        from features.classifier import fill_parameters
        fill_parameters(mod, seed)
        return mod
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            v = rng.uniform(-0.3, 0.3, size=tuple(p.shape))
            if name.endswith('a_2'):
                v = 1.0 + v
            p.copy_(torch.from_numpy(v.astype(np.float32)))
    return mod


def _input(T, B, d, seed):
    """[T, B, d] with zero rows behind half the columns (odd b ends at max(1, T // 2))."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, B, d)).astype(np.float32)
    x[max(1, T // 2):, 1::2] = 0.0
    return x


_CACHE = {}


def _block_case(dims, T, B, k_scale=1.0, fill='wide'):
    """(module on the CPU, fp32; x; the fp64 stand-in's output), computed once per case and left unchanged."""
    import torch
    from features.classifier import _TransformerEncoder
    key = (dims, T, B, k_scale, fill)
    if key not in _CACHE:
        d, di, dk, dv = DIMS[dims]
        enc = _fill(_TransformerEncoder(d, di, 1, dk, dv).eval(), 11, fill)
        if k_scale != 1.0:
            with torch.no_grad():
                enc.slf_attn.w_ks.mul_(k_scale)
        x = _input(T, B, d, 1000 * T + B)
        with torch.no_grad():
            ref = copy.deepcopy(enc).double()(torch.from_numpy(x).double()).numpy()
        _CACHE[key] = (enc, x, ref)
    return _CACHE[key]


def _native_block(enc, x):
    import torch
    dev = _dev()
    with torch.no_grad():
        return copy.deepcopy(enc).to(dev)(torch.from_numpy(x).to(dev), native=True).cpu().numpy()


# ---- pinned to the real reference ---------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def goldens():
    return np.load(os.path.join(HERE, 'golden', 'clf_golden.npz')), np.load(os.path.join(HERE, 'golden', 'rnn_golden.npz'))


def _make(kind, g):                                         # as tests/test_classifier_golden.py::_make fills the heads
    import torch
    from features import classifier as C
    cls, k = {'hrnn_att': (C.HRNNAttHead, 1), 'transformer': (C.TransformerHead, 2)}[kind]
    torch.manual_seed(0)
    head = cls().eval()
    names = C.fill_parameters(head, int(g['seed']) + k)
    assert names == [str(n) for n in g[kind + '_names']], kind
    return head


@pytest.mark.parametrize('native_enc', [None, True])
def test_transformer_head_with_the_native_block_reproduces_the_reference(goldens, native_enc):
    import torch
    g, rnn_g = goldens
    dev, tol = _dev(), 2e-4
    head = _make('transformer', g).to(dev)
    inp = torch.from_numpy(rnn_g['inp']).to(dev)
    assert tuple(inp.shape) == (200, 8, 39)
    scale = lambda a: max(1.0, float(np.max(np.abs(a))))
    with torch.no_grad():
        lo, feat, a = [v.cpu().numpy() for v in head(inp, rnn_g['len0'], dropout=False, native_enc=native_enc, native_attn=True)]
    e_rows = np.max(np.abs(a[[0, 11, 56, 130, 199]] - g['transformer_attn_rows'])) / scale(g['transformer_attn_rows'])
    e_sum = np.max(np.abs(a.astype(np.float64).sum(0) - g['transformer_attn_sum'])) / scale(g['transformer_attn_rows'])
    e_feat = np.max(np.abs(feat - g['transformer_feat_nodrop'])) / scale(g['transformer_feat_nodrop'])
    e_lo = np.max(np.abs(lo - g['transformer_logits_nodrop'])) / scale(g['transformer_logits_nodrop'])
    print(f'transformer head, native block (native_enc={native_enc}): rows {e_rows:.3g} sum {e_sum:.3g} feat {e_feat:.3g} logits {e_lo:.3g}')
    record('attn_head_golden_rows', e_rows)
    record('attn_head_golden_logits', e_lo)
    assert e_rows <= tol and e_sum <= 200 * tol and e_feat <= tol and e_lo <= tol


def test_hrnn_att_head_with_the_native_pooling_reproduces_the_reference(goldens):
    import torch
    g, rnn_g = goldens
    dev, tol = _dev(), 2e-4
    head = _make('hrnn_att', g).to(dev)
    inp = torch.from_numpy(rnn_g['inp']).to(dev)
    with torch.no_grad():
        lo, feat = [v.cpu().numpy() for v in head(inp, rnn_g['len0'], dropout=False, native_attn=True)]
    e_feat, e_lo = _err(feat, g['hrnn_att_feat_nodrop']), _err(lo, g['hrnn_att_logits_nodrop'])
    print(f'hrnn_att head, native pooling: feat {e_feat:.3g} logits {e_lo:.3g}')
    record('selfattn_head_golden_logits', e_lo)
    assert e_feat <= tol and e_lo <= tol


# ---- parity of the block against the fp64 stand-in ----------------------------------------------------------------------------

@pytest.mark.parametrize('fill', ['golden', 'wide'])
@pytest.mark.parametrize('dims', list(DIMS))
@pytest.mark.parametrize('T,B', SHAPES)
def test_block_matches_the_fp64_standin(T, B, dims, fill):
    enc, x, ref = _block_case(dims, T, B, fill=fill)
    got = _native_block(enc, x)
    assert got.shape == ref.shape == (T, B, DIMS[dims][0])
    e = _err(got, ref)
    print(f'block {dims} {fill} T {T} B {B}: {e:.3g}')
    record('attn_block_vs_fp64', e)
    assert np.isfinite(got).all() and e <= BAR


def test_scores_beyond_88_do_not_overflow_and_columns_are_coupled():
    import torch
    T, B = 33, 17
    enc, x, ref = _block_case('head', T, B, k_scale=300.0, fill='golden')
    with torch.no_grad():                                   # what the case is about: scores far beyond exp's fp32 range
        a = enc.slf_attn
        xb = torch.from_numpy(x).double().transpose(0, 1)
        s = torch.bmm(torch.tanh(xb @ a.w_qs[0].double()), (xb @ a.w_ks[0].double()).transpose(1, 2)) / np.sqrt(x.shape[2])
    assert float(s.abs().max()) > 100 and np.isfinite(ref).all()
    got = _native_block(enc, x)
    e = _err(got, ref)
    print(f'block, w_ks x 300: max |s| {float(s.abs().max()):.1f}, error {e:.3g}')
    record('attn_block_overflow_vs_fp64', e)
    assert np.isfinite(got).all() and e <= BAR
    # the softmax runs over the batch axis: another column's input changes this column's output
    x2 = x.copy()
    x2[:, 5] = _input(T, 1, x.shape[2], 99)[:, 0]
    got2 = _native_block(enc, x2)
    others = [b for b in range(B) if b != 5]
    assert np.max(np.abs(got2[:, others] - got[:, others])) > 1e-3


# ---- pooling ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('T,B,H', [(1, 1, 200), (7, 3, 200), (40, 17, 200), (40, 33, 200), (9, 5, 12)])
def test_pooling_matches_the_fp64_standin(T, B, H):
    import torch
    from features.classifier import _SelfAttn
    dev = _dev()
    pool = _fill(_SelfAttn(H).eval(), 5)
    y = _input(T, B, H, 7 * T + B)
    if B >= 3:
        y[:, 2] = 0.0                                       # an all-zero column: uniform weights over zero rows, not a masked softmax
    with torch.no_grad():
        ref = copy.deepcopy(pool).double()(torch.from_numpy(y).double()).numpy()
        got = copy.deepcopy(pool).to(dev)(torch.from_numpy(y).to(dev), native=True).cpu().numpy()
    assert got.shape == ref.shape == (B, H)
    e = _err(got, ref)
    print(f'pooling T {T} B {B} H {H}: {e:.3g}')
    record('selfattn_pool_vs_fp64', e)
    assert np.isfinite(got).all() and e <= BAR
    if B >= 3:
        assert np.array_equal(got[2], np.zeros(H, np.float32))
        # a column whose rows behind its end are zero still spends weight on them: the result is NOT the masked softmax's
        yt = torch.from_numpy(y).double()
        n = max(1, T // 2)
        with torch.no_grad():
            masked = copy.deepcopy(pool).double()(yt[:n]).numpy()
        if T >= 7:
            assert np.max(np.abs(masked[1] - ref[1])) > 1e-3 and _err(got[1], ref[1]) <= BAR


# ---- mechanics ----------------------------------------------------------------------------------------------------------------------

def test_two_runs_a_view_and_a_side_stream_give_the_same_bits():
    import torch
    from features.classifier import _SelfAttn
    dev = _dev()
    enc, x, _ = _block_case('head', 33, 17)
    enc = copy.deepcopy(enc).to(dev)
    xd = torch.from_numpy(x).to(dev)
    pool = _fill(_SelfAttn(200).eval(), 5).to(dev)
    yd = torch.from_numpy(_input(40, 17, 200, 3)).to(dev)
    with torch.no_grad():
        a, b = enc(xd, native=True), enc(xd, native=True)
        pa, pb = pool(yd, native=True), pool(yd, native=True)
        assert torch.equal(a, b) and torch.equal(pa, pb)
        # strided views: every other column of a wider tensor, and a [B, T, .] tensor seen as [T, B, .]
        wide = torch.randn(33, 34, 39, device=dev)
        wide[:, ::2] = xd
        assert not wide[:, ::2].is_contiguous() and torch.equal(enc(wide[:, ::2], native=True), a)
        yt = yd.transpose(0, 1).contiguous().transpose(0, 1)
        assert not yt.is_contiguous() and torch.equal(pool(yt, native=True), pa)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            c, pc = enc(xd, native=True), pool(yd, native=True)
        side.synchronize()
        assert torch.equal(c, a) and torch.equal(pc, pa)


def _raw(enc, T, B, dev):
    """The handle and caller-owned buffers of a raw dsp_attn_forward call."""
    import torch
    from features import _native as nat
    handle = enc._native_handle(dev)
    nb = nat.c_i64(0)
    nat.check(nat.load().dsp_attn_workspace_bytes(handle, T, B, nat.C.byref(nb)))
    return handle, nb.value


def test_forward_captured_into_a_graph_replays_on_new_data():
    import torch
    from features import _native as nat
    dev = _dev()
    T, B = 33, 17
    enc, x, _ = _block_case('head', T, B)
    enc = copy.deepcopy(enc).to(dev)
    xs = [torch.from_numpy(x).to(dev), torch.from_numpy(_input(T, B, 39, 5)).to(dev)]
    with torch.no_grad():
        want = [enc(v, native=True) for v in xs]
    handle, nbytes = _raw(enc, T, B, dev)
    xb, y = xs[0].clone(), torch.zeros(T, B, 39, device=dev)
    work = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        nat.check(nat.load().dsp_attn_forward(handle, xb.data_ptr(), T, B, y.data_ptr(), work.data_ptr(), nbytes,
                                              torch.cuda.current_stream(dev).cuda_stream))
    for k in (1, 0):
        xb.copy_(xs[k])
        y.zero_(); work.zero_()
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(y, want[k])


def test_canaries_behind_the_outputs_and_the_workspace_survive():
    import torch
    from features import _native as nat
    from features.classifier import _SelfAttn
    from test_gpu_canaries import _guarded
    dev = _dev()
    lib = nat.load()
    st = lambda: torch.cuda.current_stream(dev).cuda_stream
    for dims, T, B in (('head', 33, 17), ('small', 17, 2), ('head', 1, 3)):
        enc, x, ref = _block_case(dims, T, B)
        enc = copy.deepcopy(enc).to(dev)
        d = DIMS[dims][0]
        xd = torch.from_numpy(x).to(dev)
        handle, nbytes = _raw(enc, T, B, dev)
        ybuf, yptr, ycheck = _guarded(T * B * d * 4, dev)
        wbuf, wptr, wcheck = _guarded(nbytes, dev)
        nat.check(lib.dsp_attn_forward(handle, xd.data_ptr(), T, B, yptr, wptr, nbytes, st()))
        got = ycheck(f'd_y {dims} T {T} B {B}').view(np.float32).reshape(T, B, d)
        wcheck(f'd_work {dims} T {T} B {B}')
        assert np.isfinite(got).all() and _err(got, ref) <= BAR        # every element written: the fill is a NaN pattern
    for T, B, H in ((40, 17, 200), (9, 5, 12)):
        pool = _fill(_SelfAttn(H).eval(), 5).to(dev)
        yd = torch.from_numpy(_input(T, B, H, 1)).to(dev)
        obuf, optr, ocheck = _guarded(B * H * 4, dev)
        nat.check(lib.dsp_selfattn_pool_batch(yd.data_ptr(), T, B, H, pool.attn.weight.data_ptr(), pool.attn.bias.data_ptr(),
                                              pool.v.weight.data_ptr(), pool.v.bias.data_ptr(), optr, st()))
        got = ocheck(f'd_out T {T} B {B} H {H}').view(np.float32).reshape(B, H)
        with torch.no_grad():
            assert np.array_equal(got, pool(yd, native=True).cpu().numpy())


def test_a_parameter_written_in_place_rebuilds_the_handle():
    import torch
    dev = _dev()
    enc, x, _ = _block_case('small', 17, 2)
    enc = copy.deepcopy(enc).to(dev)
    xd = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        a = enc(xd, native=True)
        h0, k0, v0 = enc._handle, enc._handle_key, enc.pos_ffn.w_2.bias._version
        assert h0 is not None and torch.equal(enc(xd, native=True), a) and enc._handle == h0      # unchanged parameters: the same handle
        enc.pos_ffn.w_2.bias.add_(0.25)
        assert enc.pos_ffn.w_2.bias._version != v0
        b = enc(xd, native=True)
        assert enc._handle is not None and enc._handle_key != k0
        want = enc(xd, native=False)
    assert not torch.equal(a, b)
    assert float((b - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    clone = copy.deepcopy(enc)
    assert clone._handle is None                            # a copy builds its own
