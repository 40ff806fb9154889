"""The training entry points of the heads on the device (csrc/kernels_head.h, csrc/kernels_attn*.h, csrc/dsp_rnn.hip,
csrc/dsp_attn.hip) against the restatements of tests/head_train_cases.py, which tests/test_head_train_host.py pins to torch
fp64 autograd:

  * ``dsp_head_pool_train_batch``: the bits of ``dsp_head_pool_batch`` and the row of every maximum, exactly;
  * ``dsp_head_pool_backward_batch``: every element written, exact zeros at t >= len, the fp64 restatement within BAR and the
    fp32 restatement's bits where the arithmetic is exact; col_avg < 0, a strided ld_g, the scalar route, a misaligned d_gy;
  * the ``dsp_selfattn_pool_rows_*`` pair: the bits of the plain pair on the contiguous ``y[:rows]``, zeros behind;
  * ``dsp_*_refresh``: after the parameters were written in place the handle is kept and gives the bits of a fresh one, eager
    and inside a replayed HIP graph; wrong sizes and NULLs are DSP_EINVAL.

The shapes are those of tests/head_pool_cases.py (the smallest at which the pooling can go wrong); T, B = 9, 5 for the refresh."""
import copy

import numpy as np
import pytest

import head_pool_cases as hp
import head_train_cases as ht
from conftest import record

pytestmark = pytest.mark.gpu

BAR = 2e-5                 # the BAR of tests/test_gpu_head_pool.py: error <= BAR * max(1, max |ref|)
SENT = np.float32(-12345.5)
ISENT = -777


def _dev():
    import torch
    return torch.device('cuda', 0)


def _st(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def _err(got, ref):
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got.astype(np.float64)[ok] - ref[ok]))) / max(1.0, float(np.max(np.abs(ref[ok]))))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pool_train(yd, lens_d, rows_d, H, ld, col_avg, col_max, train=True):
    """One call on a sentinel-filled [B, ld] tensor -> (feat, arg or None) as NumPy."""
    import torch
    from features import _native as nat
    T, B, _ = yd.shape
    dev = yd.device
    feat = torch.full((B, ld), float(SENT), dtype=torch.float32, device=dev)
    rows_p = None if rows_d is None else rows_d.data_ptr()
    if not train:
        nat.check(nat.load().dsp_head_pool_batch(yd.data_ptr(), T, B, H, lens_d.data_ptr(), rows_p, feat.data_ptr(), ld, col_avg, col_max,
                                                 _st(dev)))
        return feat.cpu().numpy(), None
    arg = torch.full((B, H), ISENT, dtype=torch.int32, device=dev)
    nat.check(nat.load().dsp_head_pool_train_batch(yd.data_ptr(), T, B, H, lens_d.data_ptr(), rows_p, feat.data_ptr(), ld, col_avg, col_max,
                                                   arg.data_ptr(), _st(dev)))
    return feat.cpu().numpy(), arg.cpu().numpy()


def _variants(T, B, H):
    out = [('plain', v) for v in hp.pool_variants(T, B, H)] + [('exact', v) for v in hp.pool_variants(T, B, H, exact=True)]
    if T >= 9:
        out += [('ties', v) for v in ht.tie_variants(T, B, H)]
    return out


@pytest.mark.parametrize('shape', hp.POOL_SHAPES)
def test_pool_train_gives_the_forwards_bits_and_the_row_of_every_maximum(shape):
    import torch
    T, B, H = shape
    dev = _dev()
    ld, ca, cm = 2 * H + 7, 2, H + 5
    seen, ties = set(), 0
    for kind, v in _variants(T, B, H):
        rows, lens = v['rows'], v['lens']
        yd = torch.from_numpy(v['y']).to(dev)
        lens_d = torch.from_numpy(lens).to(dev)
        rows_d = torch.tensor([rows], dtype=torch.int32, device=dev)
        want_arg = ht.pool_train_ref(v['y'], lens, rows)[2]
        for col_avg in (ca, -1):
            feat, arg = _pool_train(yd, lens_d, rows_d, H, ld, col_avg, cm)
            plain, _ = _pool_train(yd, lens_d, rows_d, H, ld, col_avg, cm, train=False)
            assert np.array_equal(_bits(feat), _bits(plain)), (shape, kind, col_avg)      # sentinels included: the same columns written
            assert np.array_equal(arg, want_arg), (shape, kind, col_avg)
        for b in v['neg_lt']:
            assert (arg[b] == -1).all()
            seen.add('lt')
        for b in v['neg_eq']:
            assert ((arg[b] >= 0) & (arg[b] < lens[b])).all()
            seen.add('eq')
        if v['nan_at'] is not None:
            t, b, h = v['nan_at']
            assert arg[b, h] == t
            seen.add('nan')
        for b, h, first in v.get('ties', []):
            assert arg[b, h] == first
            ties += 1
        # d_rows NULL: rows = T
        _, arg_full = _pool_train(yd, lens_d, None, H, ld, ca, cm)
        assert np.array_equal(arg_full, ht.pool_train_ref(v['y'], lens, None)[2])
    assert seen == ({'eq', 'lt', 'nan'} if T >= 3 else {'nan'})
    assert ties >= 3 or T < 9


def test_pool_train_first_nan_zero_tie_and_the_scalar_route_on_a_misaligned_view():
    """Two NaNs in a column: the first one's row.  An active 0.0 against the padding: the active row.  The same on a y that is
    4 bytes off a 16-byte boundary (H a multiple of 4, scalar loads)."""
    import torch
    dev = _dev()
    T, B, H = 9, 2, 4
    y = -np.ones((T, B, H), dtype=np.float32)
    lens = np.array([6, 5], dtype=np.int32)
    y[2, 0, 1] = y[4, 0, 1] = np.nan
    y[3, 1, 2] = 0.0
    for b in range(B):
        y[lens[b]:, b] = np.nan
    want = ht.pool_train_ref(y, lens, T)[2]
    assert want[0, 1] == 2 and want[1, 2] == 3 and (np.delete(want.reshape(-1), [1, 6]) == -1).all()
    lens_d = torch.from_numpy(lens).to(dev)
    base = torch.zeros(T * B * H + 1, dtype=torch.float32, device=dev)
    off = base[1:].view(T, B, H)
    off.copy_(torch.from_numpy(y))
    assert off.data_ptr() % 16 == 4
    a_feat, a_arg = _pool_train(torch.from_numpy(y).to(dev), lens_d, None, H, 2 * H, 0, H)
    s_feat, s_arg = _pool_train(off, lens_d, None, H, 2 * H, 0, H)
    assert np.array_equal(a_arg, want) and np.array_equal(s_arg, want)
    assert np.array_equal(_bits(a_feat), _bits(s_feat))


def _backward(g_d, ld_g, col_avg, col_max, lens_d, arg_d, T, B, H, gy=None):
    import torch
    from features import _native as nat
    dev = g_d.device
    if gy is None:
        gy = torch.full((T, B, H), float(SENT), dtype=torch.float32, device=dev)
    nat.check(nat.load().dsp_head_pool_backward_batch(g_d.data_ptr(), ld_g, col_avg, col_max, lens_d.data_ptr(), arg_d.data_ptr(), T, B, H,
                                                      gy.data_ptr(), _st(dev)))
    return gy


@pytest.mark.parametrize('shape', hp.POOL_SHAPES)
def test_pool_backward_against_the_restatements(shape):
    """g lies in a [B, ld_g] matrix (ld_g > 2 H: a strided gradient) whose every other column is NaN; d_gy is prefilled with
    a sentinel.  (33, 2, 3) is the scalar route."""
    import torch
    T, B, H = shape
    dev = _dev()
    ld, ca, cm = 2 * H + 7, 2, H + 5
    cases = [('plain', v, False) for v in hp.pool_variants(T, B, H)] + [('pow2', v, True) for v in ht.pow2_variants(T, B, H)]
    if T >= 9:
        cases += [('ties', v, False) for v in ht.tie_variants(T, B, H)]
    for kind, v, exact in cases:
        rows, lens = v['rows'], v['lens']
        g_avg, g_max = ht.grad_case(B, H, exact=exact)
        g = np.full((B, ld), np.nan, dtype=np.float32)
        g[:, ca:ca + H], g[:, cm:cm + H] = g_avg, g_max
        g_d = torch.from_numpy(g).to(dev)
        lens_d = torch.from_numpy(lens).to(dev)
        arg = ht.pool_train_ref(v['y'], lens, rows)[2].astype(np.int32)
        arg_d = torch.from_numpy(arg).to(dev)
        active = np.arange(T)[:, None] < lens[None, :]
        for col_avg in (ca, -1):
            gy_d = _backward(g_d, ld, col_avg, cm, lens_d, arg_d, T, B, H)
            gy = gy_d.cpu().numpy()
            assert not (gy == SENT).any() and np.isfinite(gy).all(), (shape, kind)       # every element written, no NaN column read
            assert (_bits(gy[~active]) == 0).all(), (shape, kind)                        # t >= len: +0.0f
            ga = g_avg if col_avg >= 0 else None
            ref = ht.pool_backward_ref(ga, g_max, lens, arg, T, np.float64)
            e = record('head_pool_backward_vs_fp64', _err(gy[active], ref[active]))
            assert e <= BAR, (shape, kind, e)
            if exact:
                ref32 = ht.pool_backward_ref(ga, g_max, lens, arg, T, np.float32)
                assert np.array_equal(_bits(gy[active]), _bits(ref32[active])), (shape, kind)
            # a dense gradient (ld_g = the columns read) and a second run: the same bits
            dense = np.concatenate([g_avg, g_max], 1) if col_avg >= 0 else g_max
            d_d = torch.from_numpy(np.ascontiguousarray(dense)).to(dev)
            again = _backward(d_d, dense.shape[1], 0 if col_avg >= 0 else -1, H if col_avg >= 0 else 0, lens_d, arg_d, T, B, H)
            assert torch.equal(again.view(torch.int32), gy_d.view(torch.int32))
            # d_gy 4 bytes off a 16-byte boundary (the scalar stores): the same bits
            base = torch.full((T * B * H + 1,), float(SENT), dtype=torch.float32, device=dev)
            off = base[1:].view(T, B, H)
            assert off.data_ptr() % 16 == 4
            _backward(g_d, ld, col_avg, cm, lens_d, arg_d, T, B, H, gy=off)
            assert torch.equal(off.view(torch.int32), gy_d.view(torch.int32)) and float(base[0]) == float(SENT)


def test_pool_autograd_function_equals_the_restatement():
    """``_pool_native`` on a y that requires a gradient: the values of the forward-only call, the restatement's gradient."""
    import torch
    from features.classifier import _pool_native
    dev = _dev()
    T, B, H = 40, 17, 200
    v = hp.pool_variants(T, B, H)[0]
    rows, lens = v['rows'], v['lens']
    g_avg, g_max = ht.grad_case(B, H)
    lens_d = torch.from_numpy(lens).to(dev)
    rows_d = torch.tensor([rows], dtype=torch.int32, device=dev)
    arg = ht.pool_train_ref(v['y'], lens, rows)[2]
    active = np.arange(T)[:, None] < lens[None, :]
    for avg in (True, False):
        y = torch.from_numpy(v['clean']).to(dev).requires_grad_(True)
        feat = _pool_native(y, lens_d, rows_d, avg=avg, grad=True)
        assert _pool_native(y, lens_d, rows_d, avg=avg).grad_fn is None      # without the flag: detached, as before
        with torch.no_grad():
            plain = _pool_native(y, lens_d, rows_d, avg=avg)
        assert type(feat.grad_fn).__name__.startswith('_PoolTrain') and torch.equal(feat.detach(), plain)
        g = np.concatenate([g_avg, g_max], 1) if avg else g_max
        feat.backward(torch.from_numpy(np.ascontiguousarray(g)).to(dev))
        ref = ht.pool_backward_ref(g_avg if avg else None, g_max, lens, arg, T)
        got = y.grad.cpu().numpy()
        assert (got[~active] == 0).all() and _err(got[active], ref[active]) <= BAR


@pytest.mark.parametrize('shape', hp.ATTN_SHAPES)
def test_selfattn_rows_pair_equals_the_plain_pair_on_the_first_rows(shape):
    import torch
    from features import _native as nat
    T, B, H = shape
    dev = _dev()
    lib = nat.load()
    y, W, bW, v, c = hp.attn_case(T, B, H)
    g_out = np.random.default_rng(5 + T).standard_normal((B, H)).astype(np.float32)
    yd, Wd, bd, vd, cd, gd = (torch.from_numpy(a).to(dev) for a in (y, W, bW, v, c, g_out))
    par = (Wd.data_ptr(), bd.data_ptr(), vd.data_ptr())
    f32 = dict(dtype=torch.float32, device=dev)
    st = _st(dev)
    for rows in hp.ATTN_ROWS(T):
        head = yd[:rows].contiguous()
        want = dict(out=torch.empty(B, H, **f32), w=torch.empty(rows, B, **f32), g_y=torch.empty(rows, B, H, **f32),
                    g_pre=torch.empty(rows, B, H, **f32), g_e=torch.empty(rows, B, **f32), gv=torch.empty(B, H, **f32))
        nat.check(lib.dsp_selfattn_pool_train_batch(head.data_ptr(), rows, B, H, *par, cd.data_ptr(), want['out'].data_ptr(),
                                                    want['w'].data_ptr(), st))
        nat.check(lib.dsp_selfattn_pool_backward_batch(head.data_ptr(), rows, B, H, *par, want['w'].data_ptr(), gd.data_ptr(),
                                                       want['g_y'].data_ptr(), want['g_pre'].data_ptr(), want['g_e'].data_ptr(),
                                                       want['gv'].data_ptr(), st))
        poisoned = yd.clone()
        poisoned[rows:] = float('nan')                           # rows behind the count are not part of the result
        rows_d = torch.tensor([rows], dtype=torch.int32, device=dev)
        got = dict(out=torch.full((B, H), float(SENT), **f32), w=torch.full((T, B), float(SENT), **f32),
                   g_y=torch.full((T, B, H), float(SENT), **f32), g_pre=torch.full((T, B, H), float(SENT), **f32),
                   g_e=torch.full((T, B), float(SENT), **f32), gv=torch.full((B, H), float(SENT), **f32))
        nat.check(lib.dsp_selfattn_pool_rows_train_batch(poisoned.data_ptr(), T, B, H, *par, cd.data_ptr(), got['out'].data_ptr(),
                                                         got['w'].data_ptr(), rows_d.data_ptr(), st))
        nat.check(lib.dsp_selfattn_pool_rows_backward_batch(poisoned.data_ptr(), T, B, H, *par, got['w'].data_ptr(), gd.data_ptr(),
                                                            got['g_y'].data_ptr(), got['g_pre'].data_ptr(), got['g_e'].data_ptr(),
                                                            got['gv'].data_ptr(), rows_d.data_ptr(), st))
        ref = ht.selfattn_rows_train_ref(y, rows, W, bW, v, c, g_out)
        for key in ('out', 'gv'):
            assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), (shape, rows, key)
        for key in ('w', 'g_y', 'g_pre', 'g_e'):
            assert torch.equal(got[key][:rows].view(torch.int32), want[key].view(torch.int32)), (shape, rows, key)
            assert (got[key][rows:].view(torch.int32) == 0).all(), (shape, rows, key)     # every element behind: +0.0f
        for key, name in (('out', 'out'), ('w', 'w'), ('g_y', 'g_y'), ('g_pre', 'g_pre'), ('g_e', 'g_e'), ('gv', 'gv_part')):
            e = record(f'selfattn_rows_train_{key}_vs_fp64', _err(got[key].cpu().numpy(), ref[name]))
            assert e <= BAR, (shape, rows, key, e)
        # without d_gy: the other three are the same
        three = [torch.full_like(got[k], float(SENT)) for k in ('g_pre', 'g_e', 'gv')]
        nat.check(lib.dsp_selfattn_pool_rows_backward_batch(poisoned.data_ptr(), T, B, H, *par, got['w'].data_ptr(), gd.data_ptr(), None,
                                                            *[t.data_ptr() for t in three], rows_d.data_ptr(), st))
        for t, k in zip(three, ('g_pre', 'g_e', 'gv')):
            assert torch.equal(t.view(torch.int32), got[k].view(torch.int32))


def test_selfattn_module_gradients_with_the_rows_on_the_device():
    """``_SelfAttn(y, d_rows=..., device_grad=True)``: the gradients of the native training path on ``y[:rows]``."""
    import torch
    from features.classifier import _SelfAttn
    dev = _dev()
    T, B, H = 40, 3, 200
    y, W, bW, v, c = hp.attn_case(T, B, H)
    mod = _SelfAttn(H)
    with torch.no_grad():
        for p, a in zip((mod.attn.weight, mod.attn.bias, mod.v.weight, mod.v.bias), (W, bW, v, c)):
            p.copy_(torch.from_numpy(a))
    mod = mod.to(dev)
    g_out = torch.from_numpy(np.random.default_rng(9).standard_normal((B, H)).astype(np.float32)).to(dev)
    rows = 17
    res = []
    for route in ('rows', 'plain'):
        yd = torch.from_numpy(y).to(dev).requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        if route == 'rows':
            out = mod(yd, native=True, d_rows=torch.tensor([rows], dtype=torch.int32, device=dev), device_grad=True)
            assert type(out.grad_fn).__name__.startswith('_SelfAttnRowsTrain')
        else:
            out = mod(yd[:rows], native=True)
        out.backward(g_out)
        res.append([out.detach(), yd.grad] + [p.grad for p in mod.parameters()])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and (res[0][1][rows:] == 0).all()
    for a, b in zip(res[0][2:], res[1][2:]):                     # sums over T rows (zeros behind) against sums over `rows` rows
        e = record('selfattn_rows_module_param_grads_vs_plain', _err(a.cpu().numpy(), b.cpu().numpy().astype(np.float64)))
        assert e <= BAR


# ---- refresh ----------------------------------------------------------------------------------------------------------------

RT, RB = 9, 5
LENS = np.array([9, 1, 5, 4, 8], dtype=np.int32)


def _refresh_module(kind, dev):
    import torch
    from features import classifier as C
    torch.manual_seed(0)
    m, width = {'bigru': (lambda: C._DynEnc(12, 20, 2), 12), 'hmlstm': (lambda: C.HMLSTM(1.0, 20, [28, 24]), 20),
                'attn': (lambda: C._TransformerEncoder(39, 200, 1, 100, 100), 39)}[kind]
    m = m().train()
    C.fill_parameters(m, 21)
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((RT, RB, width))).astype(np.float32)
    for b in range(RB):
        x[LENS[b]:, b] = 0.0
    return m.to(dev), torch.from_numpy(x).to(dev)


def _refresh_run(kind, m, x, d_len, grad=True):
    """Forward (+ backward into x and the parameters) on the refreshing route -> a list of tensors: outputs, then gradients."""
    import torch
    if not grad:
        with torch.no_grad():
            if kind == 'bigru':
                return list(m.run(x, d_len, device_len=True, device_grad=True))
            if kind == 'hmlstm':
                return [m.run(x, None, lens=d_len, device_len=True, device_grad=True).last_h2]
            return [m.run(x, native=True, refresh=True)]
    xg = x.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    if kind == 'bigru':
        outs = list(m.run(xg, d_len, device_len=True, device_grad=True))
    elif kind == 'hmlstm':
        outs = [m.run(xg, None, lens=d_len, device_len=True, device_grad=True).last_h2]
    else:
        outs = [m.run(xg, native=True, refresh=True)]
    gen = torch.Generator(device='cpu').manual_seed(3)
    loss = sum((o * torch.randn(o.shape, generator=gen).to(o.device)).sum() for o in outs)
    loss.backward()
    grads = [xg.grad] + [p.grad for p in m.parameters()]
    assert all(g is not None for g in grads)
    return [o.detach().clone() for o in outs] + [g.clone() for g in grads]


def _perturb(m, seed):
    import torch
    gen = torch.Generator(device='cpu').manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_((0.01 * torch.randn(p.shape, generator=gen)).to(p.device))


@pytest.mark.parametrize('kind', ['bigru', 'hmlstm', 'attn'])
def test_refresh_keeps_the_handle_and_gives_a_fresh_handles_bits(kind):
    import torch
    dev = _dev()
    m, x = _refresh_module(kind, dev)
    d_len = torch.from_numpy(LENS).to(dev)
    first = _refresh_run(kind, m, x, d_len)
    handle = m._handle
    assert handle is not None
    _perturb(m, 1)
    assert m._param_key(dev.index) != m._handle_key                          # the versions moved, the tensors did not
    second = _refresh_run(kind, m, x, d_len)
    assert m._handle == handle and m._param_key(dev.index) == m._handle_key  # kept, repacked in place
    fresh = copy.deepcopy(m)
    assert fresh._handle is None
    want = _refresh_run(kind, fresh, x, d_len)                               # builds a new handle through create
    assert fresh._handle is not None and fresh._handle != handle
    assert len(second) == len(want)
    for k, (a, b) in enumerate(zip(second, want)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (kind, k)
    n_out = 2 if kind == 'bigru' else 1
    assert not torch.equal(second[0], first[0]) and not torch.equal(second[n_out], first[n_out])
    # (... and it is not the first run's answer: the first output and the gradient of x both moved)
    # without refresh a written parameter still rebuilds, as it always did
    _perturb(m, 2)
    m._native_handle(dev)
    assert m._param_key(dev.index) == m._handle_key
    # refresh plus forward recorded in a HIP graph: the replay repacks what was written since
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _refresh_run(kind, m, x, d_len, grad=False)                          # warm-up: the handle exists, the key is current
    side.synchronize()
    kept = m._handle
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        m._native_handle(dev, refresh='always')
        out_g = _refresh_run(kind, m, x, d_len, grad=False)
    assert m._handle == kept
    _perturb(m, 3)
    torch.cuda.synchronize(dev)
    graph.replay()
    torch.cuda.synchronize(dev)
    want = _refresh_run(kind, copy.deepcopy(m), x, d_len, grad=False)
    for a, b in zip(out_g, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), kind


def test_refresh_refuses_other_sizes_and_null_parameters():
    import ctypes as C
    import torch
    from features import _native as nat
    from features import classifier as cl
    dev = _dev()
    lib = nat.load()
    st = _st(dev)

    def einval(rc, what):
        assert rc == nat.EINVAL and what in lib.dsp_last_error().decode(), (rc, lib.dsp_last_error())
    pairs = {'bigru': (cl._DynEnc(12, 20, 2), cl._DynEnc(12, 24, 2), 'dsp_bigru_refresh'),
             'hmlstm': (cl.HMLSTM(1.0, 20, [28, 24]), cl.HMLSTM(1.0, 20, [28, 28]), 'dsp_hmlstm_refresh'),
             'attn': (cl._TransformerEncoder(39, 200, 1, 100, 100), cl._TransformerEncoder(39, 200, 1, 100, 96), 'dsp_attn_refresh')}
    for kind, (a, b, fn) in pairs.items():
        a, b = a.to(dev), b.to(dev)
        with torch.cuda.device(dev):
            h = a._native_handle(dev)
            einval(getattr(lib, fn)(h, C.byref(b._descriptor(nat)), st), "differ from the handle's")
            d = a._descriptor(nat)
            if kind == 'hmlstm':
                d.d_c2_bias = None
            else:
                d.d_params[1] = None
            einval(getattr(lib, fn)(h, C.byref(d), st), 'NULL parameter tensor')
            einval(getattr(lib, fn)(h, None, st), 'NULL argument')
            einval(getattr(lib, fn)(None, C.byref(a._descriptor(nat)), st), 'NULL argument')
            assert getattr(lib, fn)(h, C.byref(a._descriptor(nat)), st) == nat.OK
    torch.cuda.synchronize(dev)
