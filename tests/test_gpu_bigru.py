"""The native bidirectional GRU encoder (csrc/kernels_bigru.h behind dsp_bigru_forward, features/classifier.py::_DynEnc) on
the GPU: against what the reference's layers.DynamicEncoder produced (tests/golden/bigru_golden.npz), against the nn.GRU path
on the same device, and the properties of the call itself (ragged semantics, repeatability, optional outputs, buffer edges,
argument errors, handle caching, graph capture) and of the heads that sit on it."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import bigru_cases as bc
import hmrnn_cases as hc
from conftest import record

pytestmark = pytest.mark.gpu

# (input_size, hidden, layers).  Tiles per wave = ceil(hidden / 32): 4 and 20 run the <2> instantiation of the kernel, 100 the
# <4> one, 132 and 200 the <7> one, 256 the <8> one; 1, 5, 13, 39, 78 are inputs whose rows are not 16 bytes, 512 the widest.
SHAPES = [(39, 200, 2), (78, 200, 1), (200, 200, 1), (13, 20, 3), (1, 4, 1), (5, 256, 2), (512, 132, 1), (24, 100, 4)]
GRID = [(B, T) for B in (1, 8, 37, 50) for T in (1, 7, 40)]
LOOP_CASES = [(B, T, s, 'ragged') for B, T in GRID for s in range(len(SHAPES))]          # the whole product: 96 small cases
LOOP_CASES += [(37, 7, 3, 'ones'), (50, 40, 0, 'full'), (50, 40, 5, 'short_slice')]


def _dev():
    import torch
    return torch.device('cuda', 0)


def _np(t):
    return t.detach().cpu().numpy()


def _enc(shape, seed, dev, dropout=0.0):
    import torch
    from features.classifier import _DynEnc, fill_parameters
    I, H, L = shape
    torch.manual_seed(0)
    enc = _DynEnc(I, H, L, dropout=dropout).eval()
    fill_parameters(enc, seed)
    return enc.to(dev)


def _lens(B, T, mode, seed):
    lens = np.random.default_rng(seed).integers(1, T + 1, B)
    if mode == 'ones':
        lens[:] = 1
    elif mode == 'full':
        lens[:] = T
    elif mode == 'short_slice':
        lens[16:32] = np.minimum(lens[16:32], T // 2)          # the second 16-column slice stops early
        lens[0] = T
    return lens.astype(np.int64)


def _x(T, B, I, seed, dev):
    import torch
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((T, B, I)).astype(np.float32)).to(dev)


@pytest.fixture(scope='module')
def g():
    return bc.load_golden()


@pytest.mark.parametrize('tag', bc.TAGS)
def test_native_reproduces_the_reference_encoder(tag, g):
    import torch
    dev = _dev()
    enc = bc.encoder(g, tag).to(dev)
    x, lens, _ = bc.maker().inputs(tag, np)
    with torch.no_grad():
        y, hn = enc.run(torch.from_numpy(x).to(dev), lens, native=True)
    assert y.is_contiguous() and hn.is_contiguous()
    worst = record('bigru_native_vs_reference', bc.deviation(g, tag, _np(y), _np(hn)))
    print(f'{tag}: native vs reference, worst deviation / scale = {worst:.3g}')
    assert worst <= bc.BAR


@pytest.mark.parametrize('B,T,s,mode', LOOP_CASES)
def test_native_equals_the_gru_path_on_the_device(B, T, s, mode):
    import torch
    dev = _dev()
    shape = SHAPES[s]
    enc = _enc(shape, 20260930 + s, dev)
    x = _x(T, B, shape[0], 1000 * B + T, dev)
    lens = _lens(B, T, mode, 7 * B + T)
    with torch.no_grad():
        y_ref, hn_ref = enc.run(x, lens, native=False)
        y, hn = enc.run(x, lens, native=True)
    assert y.shape == y_ref.shape == (int(lens.max()), B, shape[1]) and hn.shape == hn_ref.shape
    worst = max(float((y - y_ref).abs().max()) / hc.scale(_np(y_ref)), float((hn - hn_ref).abs().max()) / hc.scale(_np(hn_ref)))
    record('bigru_native_vs_miopen', worst)
    print(f'B {B} T {T} shape {shape} {mode}: native vs nn.GRU on the device = {worst:.3g}')
    assert worst <= bc.ROCM_BAR


def test_ragged_semantics_are_exact():
    import torch
    dev = _dev()
    shape = (39, 200, 2)
    enc = _enc(shape, 11, dev)
    B, T = 37, 23
    lens = _lens(B, T, 'ragged', 5)
    lens[:3] = (T, 1, 2)
    x = _x(T + 4, B, shape[0], 6, dev)                                         # four rows more than any length
    with torch.no_grad():
        y, hn = enc.run(x, lens, native=True)
        y_cut, hn_cut = enc.run(x[:T].contiguous(), lens, native=True)
    assert y.shape == (T, B, 200)
    assert torch.equal(y, y_cut) and torch.equal(hn, hn_cut)                    # trailing rows of the input change nothing
    yb = _np(y).view(np.uint32)
    for b in range(B):
        assert not yb[lens[b]:, b].any(), b                                     # bitwise +0.0 behind the column's end
        assert np.abs(_np(y)[:lens[b], b]).max() > 0
    # a column depends on no other column: subsets give the same bits
    for cols in ([3, 17, 18, 30, 36], [0]):
        with torch.no_grad():
            ys, hs = enc.run(x[:, cols].contiguous(), lens[cols], native=True)
        n = int(lens[cols].max())
        assert torch.equal(ys, y[:n, cols]) and torch.equal(hs, hn[:, cols]), cols
        assert not _np(y[n:, cols]).view(np.uint32).any()


def test_h_n_of_the_forward_direction_is_the_row_at_len_minus_one():
    import torch
    dev = _dev()
    enc = _enc((13, 20, 1), 12, dev)
    with torch.no_grad():
        for n, p in enc.gru.named_parameters():
            if n.endswith('_reverse'):
                p.zero_()                                                       # the reverse direction then stays at h = 0
    B, T = 21, 12
    lens = _lens(B, T, 'ragged', 8)
    lens[:2] = (T, 1)
    x = _x(T, B, 13, 9, dev)
    with torch.no_grad():
        y, hn = enc.run(x, lens, native=True)
    want = y[torch.from_numpy(lens - 1).to(dev), torch.arange(B, device=dev)]
    assert torch.equal(hn[0], want)
    assert not _np(hn[1]).view(np.uint32).any()


def test_the_same_call_twice_is_bitwise_identical(g):
    import torch
    dev = _dev()
    enc = bc.encoder(g, 'a').to(dev)
    x, lens, _ = bc.maker().inputs('a', np)
    xt = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        y1, h1 = enc.run(xt, lens, native=True)
        y2, h2 = enc.run(xt, lens, native=True)
    assert torch.equal(y1, y2) and torch.equal(h1, h2)


def _raw(enc, x, T, B, d_len=None, y=None, hn=None, work=None, work_bytes=0):
    """dsp_bigru_forward on raw pointers."""
    import torch
    from features import _native as nat
    return nat.load().dsp_bigru_forward(enc._native_handle(x.device), x.data_ptr(), T, B, d_len, y, hn, work, work_bytes,
                                        torch.cuda.current_stream(x.device).cuda_stream)


def _work_bytes(enc, T, B, dev):
    from features import _native as nat
    n = nat.c_i64(0)
    nat.check(nat.load().dsp_bigru_workspace_bytes(enc._native_handle(dev), T, B, C.byref(n)))
    return n.value


@pytest.mark.parametrize('B,T', [(37, 9), (16, 5), (1, 3)])
@pytest.mark.parametrize('s', [0, 3, 6])
def test_optional_outputs_and_canaries(B, T, s):
    """d_y, d_hn and the workspace inside larger allocations of sentinel words: the sentinels stay intact, the outputs are fully
    written (the fill is a NaN pattern), and each output is the same whether or not the other one is requested."""
    from features import _native as nat
    from test_gpu_canaries import _guarded
    dev = _dev()
    I, H, L = SHAPES[s]
    enc = _enc(SHAPES[s], 7, dev)
    x = _x(T, B, I, 8, dev)
    lens = _lens(B, T, 'ragged', 9)
    lens[0] = T
    import torch
    d_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    nbytes = _work_bytes(enc, T, B, dev)
    assert nbytes == (2 if L > 1 else 1) * T * B * 2 * H * 4

    def run(names):
        bufs = {'y': _guarded(T * B * H * 4, dev) if 'y' in names else None,
                'hn': _guarded(2 * L * B * H * 4, dev) if 'hn' in names else None, 'work': _guarded(nbytes, dev)}
        ptr = lambda k: bufs[k][1] if bufs[k] else None
        nat.check(_raw(enc, x, T, B, d_len.data_ptr(), ptr('y'), ptr('hn'), ptr('work'), nbytes))
        return {k: v[2](f'{k} of {names}').copy() for k, v in bufs.items() if v}

    full = run(('y', 'hn'))
    assert np.isfinite(full['y'].view(np.float32)).all() and np.isfinite(full['hn'].view(np.float32)).all()
    assert np.array_equal(run(('y',))['y'], full['y'])
    assert np.array_equal(run(('hn',))['hn'], full['hn'])


def test_argument_errors_return_einval_and_a_message():
    import torch
    from features import _native as nat
    dev = _dev()
    enc = _enc((13, 20, 3), 3, dev)
    B, T = 16, 9
    x = _x(T, B, 13, 4, dev)
    y = torch.empty(T, B, 20, device=dev)
    nbytes = _work_bytes(enc, T, B, dev)
    work = torch.empty(nbytes // 4, device=dev)
    lib = nat.load()
    handle = enc._native_handle(dev)
    yp, wp = y.data_ptr(), work.data_ptr()
    n = nat.c_i64(0)
    calls = ((lambda: _raw(enc, x, 0, B, None, yp, None, wp, nbytes), b'T 0'),
             (lambda: _raw(enc, x, T, 0, None, yp, None, wp, nbytes), b'B 0'),
             (lambda: _raw(enc, x, T, B, None, None, None, wp, nbytes), b'nothing to write'),
             (lambda: _raw(enc, x, T, B, None, yp, None, wp, nbytes - 4), b'workspace'),
             (lambda: _raw(enc, x, T, B, None, yp, None, None, nbytes), b'workspace'),
             (lambda: lib.dsp_bigru_forward(None, x.data_ptr(), T, B, None, yp, None, wp, nbytes, None), b'NULL'),
             (lambda: lib.dsp_bigru_forward(handle, None, T, B, None, yp, None, wp, nbytes, None), b'NULL'),
             (lambda: lib.dsp_bigru_workspace_bytes(None, T, B, C.byref(n)), b'NULL'),
             (lambda: lib.dsp_bigru_workspace_bytes(handle, 0, B, C.byref(n)), b'T 0'))
    for call, what in calls:
        rc = call()
        assert rc == nat.EINVAL and what in lib.dsp_last_error(), (rc, what, lib.dsp_last_error())
    with pytest.raises(nat.DspError):
        nat.check(rc)
    for sizes, what in (((0, 20, 1), b'input_size'), ((513, 20, 1), b'input_size'), ((13, 22, 1), b'hidden'), ((13, 260, 1), b'hidden'),
                        ((13, 0, 1), b'hidden'), ((13, 20, 0), b'n_layers'), ((13, 20, 5), b'n_layers')):
        d = nat.BigruDesc(*sizes, 0)
        for i in range(32):
            d.d_params[i] = x.data_ptr()
        h = nat.c_vp(0)
        assert lib.dsp_bigru_create(C.byref(d), C.byref(h)) == nat.EINVAL and not h.value and what in lib.dsp_last_error(), sizes
    d = nat.BigruDesc(13, 20, 1, 0)                                            # a NULL parameter
    h = nat.c_vp(0)
    assert lib.dsp_bigru_create(C.byref(d), C.byref(h)) == nat.EINVAL and b'NULL parameter' in lib.dsp_last_error()
    assert lib.dsp_bigru_create(None, C.byref(h)) == nat.EINVAL
    assert nat.check(_raw(enc, x, T, B, None, yp, None, wp, nbytes)) is None   # ... and the valid call still runs
    with torch.no_grad():
        assert torch.equal(y, enc.run(x, np.full(B, T), native=True)[0])


def test_handle_follows_the_parameters():
    """The packed copy is rebuilt when a parameter is written in place (its _version moves)."""
    import torch
    dev = _dev()
    enc = _enc((13, 20, 2), 5, dev, dropout=0.2)
    B, T = 5, 9
    x = _x(T, B, 13, 6, dev)
    lens = np.array([3, 9, 1, 5, 9])
    with torch.no_grad():
        y1 = enc(x, lens, native=True)
        h1 = enc._handle
        assert torch.equal(enc(x, lens, native=True), y1) and enc._handle == h1     # unchanged parameters: the same handle
        twin = copy.deepcopy(enc)
        assert twin._handle is None
        assert torch.equal(twin(x, lens, native=True), y1) and twin._handle not in (None, h1)
        enc.gru.weight_hh_l1_reverse.mul_(-1.0)
        y2 = enc(x, lens, native=True)
        ref = enc(x, lens, native=False)
        assert torch.equal(twin(x, lens, native=True), y1)                          # the copy kept its own parameters
    assert not torch.equal(y1, y2)
    assert float((y2 - ref).abs().max()) <= bc.ROCM_BAR
    # native=None follows _DynEnc.native_default where the native path can run; a required gradient takes nn.GRU
    calls, run_native = [], enc._run_native
    enc._run_native = lambda *a: calls.append(1) or run_native(*a)
    with torch.no_grad():
        got = enc(x, lens)
    del enc._run_native
    assert len(calls) == int(enc.native_default)
    assert torch.equal(got, y2) if enc.native_default else float((got - ref).abs().max()) <= bc.ROCM_BAR
    assert enc(x, lens).requires_grad
    with pytest.raises(RuntimeError, match='gradient'):
        enc(x, lens, native=True)
    # inter-layer dropout in training mode is the nn.GRU path's business
    enc.train()
    with torch.no_grad():
        assert 'dropout' in enc.native_supported(x)
        with pytest.raises(RuntimeError, match='dropout'):
            enc(x, lens, native=True)
        assert enc(x, lens).shape == y1.shape
    enc.eval()
    with torch.no_grad():
        assert torch.equal(enc(x, lens, native=True), y2)


def test_a_copy_owns_its_handle():
    """copy.deepcopy leaves the native handle behind: the copy builds its own on first use, and deleting the copy destroys
    that one alone -- the original keeps its handle and its results."""
    import gc
    import torch
    from features.classifier import _DynEnc, fill_parameters
    dev = _dev()
    torch.manual_seed(0)
    enc = _DynEnc(5, 4, 2).eval()
    fill_parameters(enc, 11)
    enc = enc.to(dev)
    x, lens = _x(3, 3, 5, 12, dev), np.array([3, 1, 2])
    with torch.no_grad():
        y1, hn1 = enc.run(x, lens, native=True)
        h1 = enc._handle
        assert h1 is not None
        twin = copy.deepcopy(enc)
        assert twin._handle is None
        y2, hn2 = twin.run(x, lens, native=True)
        assert twin._handle not in (None, h1)
        assert _np(y2).tobytes() == _np(y1).tobytes() and _np(hn2).tobytes() == _np(hn1).tobytes()
        del twin
        gc.collect()
        y3, hn3 = enc.run(x, lens, native=True)
    assert enc._handle == h1
    assert _np(y3).tobytes() == _np(y1).tobytes() and _np(hn3).tobytes() == _np(hn1).tobytes()


def test_graph_capture_and_replay_equals_the_eager_call(g):
    import torch
    from features import _native as nat
    dev = _dev()
    I, H, L = (int(v) for v in g['c_shape'])
    enc = bc.encoder(g, 'c').to(dev)
    B, T = 16, 40
    x = _x(T, B, I, 21, dev)
    lens = _lens(B, T, 'ragged', 22)
    lens[3] = T
    d_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    with torch.no_grad():
        y_e, hn_e = enc.run(x, lens, native=True)                              # (also builds the handle outside the capture)
    nbytes = _work_bytes(enc, T, B, dev)
    work = torch.zeros(nbytes // 4, device=dev)
    y = torch.zeros(T, B, H, device=dev)
    hn = torch.zeros(2 * L, B, H, device=dev)
    handle, lib = enc._native_handle(dev), nat.load()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            nat.check(lib.dsp_bigru_forward(handle, x.data_ptr(), T, B, d_len.data_ptr(), y.data_ptr(), hn.data_ptr(),
                                            work.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream))
    y.zero_(); hn.zero_(); work.zero_()
    torch.cuda.synchronize(dev)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(y, y_e) and torch.equal(hn, hn_e)


# ---- the heads on the native encoder -------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def rg():
    return np.load(os.path.join(bc.HERE, 'golden', 'rnn_golden.npz'))


def test_rnn_head_on_the_native_encoder_reproduces_the_reference_logits(rg):
    import torch
    from features.classifier import RNNHead, fill_parameters
    dev = _dev()
    torch.manual_seed(0)
    head = RNNHead().eval()
    assert fill_parameters(head, int(rg['seed'])) == [str(n) for n in rg['names']]
    head = head.to(dev)
    with torch.no_grad():
        got = _np(head(torch.from_numpy(rg['inp']).to(dev), rg['len0'], native_enc=True))
    d = record('bigru_rnn_head_logits_vs_reference', np.max(np.abs(got - rg['logits'])) / hc.scale(rg['logits']))
    assert d <= 1e-4


@pytest.mark.parametrize('kind', ['hrnn', 'hrnn_att', 'transformer'])
def test_hierarchical_and_transformer_heads_on_the_native_encoder(kind, rg):
    import torch
    from features import classifier as clf
    dev = _dev()
    cg = np.load(os.path.join(bc.HERE, 'golden', 'clf_golden.npz'))
    cls, k = {'hrnn': (clf.HRNNHead, 0), 'hrnn_att': (clf.HRNNAttHead, 1), 'transformer': (clf.TransformerHead, 2)}[kind]
    torch.manual_seed(0)
    head = cls().eval()
    assert clf.fill_parameters(head, int(cg['seed']) + k) == [str(n) for n in cg[kind + '_names']]
    head = head.to(dev)
    with torch.no_grad():
        res = head(torch.from_numpy(rg['inp']).to(dev), rg['len0'], dropout=False, native_enc=True)
    for got, name in ((res[1], '_feat_nodrop'), (res[0], '_logits_nodrop')):
        want = cg[kind + name]
        d = record('bigru_heads_vs_reference', np.max(np.abs(_np(got) - want)) / hc.scale(want))
        assert d <= 2e-4, (kind, name, d)


def test_hmrnn_head_on_the_native_encoder(rg):
    import torch
    from features.classifier import HMRNNHead, fill_parameters
    dev = _dev()
    hg = hc.load_golden()
    torch.manual_seed(0)
    head = HMRNNHead().eval()
    assert fill_parameters(head, int(hg['head_seed'])) == [str(n) for n in hg['head_names']]
    head = head.to(dev)
    inp = torch.from_numpy(rg['inp']).to(dev)
    with torch.no_grad():
        enc = head.enc1(inp, rg['len0'], native=True)
        r = head.enc2.run(enc, None, lens=rg['len0'], native=True)
        lo, feat = head(inp, rg['len0'], dropout=False, native=True, native_enc=True)
    zh_ref = hg['head_z_hat']
    cut = hc.cuts(zh_ref)
    ok = rg['len0'] <= cut
    assert ok.all()
    assert np.array_equal(_np(r.z_hat)[:, :, ok] > 0.5, zh_ref[:, :, ok] > 0.5)
    want = hg['head_feat_nodrop']
    d_feat = record('bigru_hmrnn_head_feat_vs_reference', np.max(np.abs(_np(feat)[ok] - want[ok])) / hc.scale(want))
    wl = hg['head_logits_nodrop']
    d_lo = record('bigru_hmrnn_head_logits_vs_reference', np.max(np.abs(_np(lo)[ok] - wl[ok])) / hc.scale(wl))
    assert d_feat <= bc.ROCM_BAR and d_lo <= bc.ROCM_BAR


def test_model_features_feed_the_rnn_head_on_the_native_encoder():
    """End to end: ModelFeatureBatch's [200, B, 39] device tensor into RNNHead; only len0 crosses to the host."""
    import torch
    from features.model_glue import ModelFeatureBatch
    from features.classifier import RNNHead, fill_parameters
    from golden_cases import make_signal
    dev = _dev()
    rate, B = 44100, 6
    clips = [make_signal(('vad', 120 + i, int((20000 + 3000 * i) * rate / 16000), rate, 0.6)) for i in range(B)]
    so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
    inp, len0, _ = ModelFeatureBatch(rate=rate).run(torch.from_numpy(np.concatenate(clips)).to(dev), so)
    assert torch.is_tensor(inp) and inp.is_cuda and tuple(inp.shape) == (200, B, 39)
    torch.manual_seed(0)
    head = RNNHead().eval()
    fill_parameters(head, 3)
    head = head.to(dev)
    len0_h = _np(len0) if torch.is_tensor(len0) else np.asarray(len0)
    with torch.no_grad():
        lo = head(inp, len0_h, native_enc=True)
        lo_gru = head(inp, len0_h, native_enc=False)
    assert lo.is_cuda and tuple(lo.shape) == (B, 20) and torch.isfinite(lo).all()
    assert float((lo - lo_gru).abs().max()) <= bc.ROCM_BAR * hc.scale(_np(lo_gru))
