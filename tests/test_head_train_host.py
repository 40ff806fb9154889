"""The training entry points of the heads without a device: the restatements of tests/head_train_cases.py -- the yardsticks of
tests/test_gpu_head_train.py -- against torch fp64 autograd on the CPU, on a y with zero rows behind each end
(``torch.cat([y[:rows].sum(0) / n, y[:rows].max(0).values])`` and the ``layers.SelfAttn`` expression on ``y[:rows]``), the
surface of the new entry points, their argument checks, and the refusals of ``device_grad`` that need no GPU."""
import os
import re

import numpy as np
import pytest

import head_pool_cases as hp
import head_train_cases as ht
from conftest import ROOT

NEW = ['dsp_head_pool_train_batch', 'dsp_head_pool_backward_batch', 'dsp_selfattn_pool_rows_train_batch',
       'dsp_selfattn_pool_rows_backward_batch', 'dsp_bigru_refresh', 'dsp_hmlstm_refresh', 'dsp_attn_refresh']


def _torch_pool(clean, lens, rows, g_avg, g_max):
    """torch fp64 autograd of the heads' pooling on the zero-padded y -> (y.grad [T, B, H], the max's indices [B, H])."""
    import torch
    y = torch.from_numpy(clean.astype(np.float64)).requires_grad_(True)
    n = torch.from_numpy(np.asarray(lens, dtype=np.float64))
    mx, idx = y[:rows].max(0)
    feat = torch.cat([y[:rows].sum(0) / n.unsqueeze(1), mx], dim=1)
    g = np.concatenate([g_avg, g_max], axis=1).astype(np.float64)
    feat.backward(torch.from_numpy(g))
    return y.grad.numpy(), idx.numpy()


def _check_against_torch(v, T, B, H, exact):
    rows, lens = v['rows'], v['lens']
    g_avg, g_max = ht.grad_case(B, H, exact=exact)
    _, mx, arg = ht.pool_train_ref(v['y'], lens, rows)
    want, idx = _torch_pool(v['clean'], lens, rows, g_avg, g_max)
    # torch's index: the restatement's row, and the first padding row (t = len) where the padding won
    assert np.array_equal(np.where(arg < 0, lens[:, None], arg), idx)
    active = np.arange(T)[:, None] < lens[None, :]                                # [T, B]
    for dtype, tol in ((np.float64, 1e-13), (np.float32, 2e-6)):                  # one division, one sum per element
        got = ht.pool_backward_ref(g_avg, g_max, lens, arg, T, dtype)
        assert got.dtype == dtype and (got[~active] == 0).all()
        err = np.abs(got.astype(np.float64) - want)[active]
        assert err.max() <= tol * max(1.0, float(np.abs(want).max())), (dtype, err.max())
    return arg, mx


@pytest.mark.parametrize('shape', hp.POOL_SHAPES)
def test_pool_restatements_equal_torch_autograd(shape):
    T, B, H = shape
    seen = set()
    for exact in (False, True):
        for v in hp.pool_variants(T, B, H, exact=exact):
            arg, mx = _check_against_torch(v, T, B, H, exact)
            lens = v['lens']
            assert ((arg >= -1) & (arg < lens[:, None])).all()
            for b in v['neg_eq']:
                assert (arg[b] >= 0).all()                                        # len == rows: there is no padding to win
                seen.add('eq')
            for b in v['neg_lt']:
                assert (arg[b] == -1).all() and (mx[b] == 0).all()                # the padding's 0 won: the gradient is dropped
                seen.add('lt')
            if v['nan_at'] is not None:
                t, b, h = v['nan_at']
                assert arg[b, h] == t
                seen.add('nan')
    assert seen == ({'eq', 'lt', 'nan'} if T >= 3 else {'nan'})


def test_pool_restatement_first_nan_and_zero_tie():
    """Two NaNs in a column: the first one's row.  An active 0.0 against the padding's 0.0: the active row (torch's first
    occurrence on a y with zero rows behind)."""
    T, B, H = 9, 2, 4
    y = -np.ones((T, B, H), dtype=np.float32)
    lens = np.array([6, 5], dtype=np.int32)
    y[2, 0, 1] = y[4, 0, 1] = np.nan
    y[3, 1, 2] = 0.0
    clean = y.copy()
    for b in range(B):
        y[lens[b]:, b] = np.nan
        clean[lens[b]:, b] = 0.0
    _, mx, arg = ht.pool_train_ref(y, lens, T)
    assert arg[0, 1] == 2 and arg[1, 2] == 3 and mx[1, 2] == 0
    keep = np.ones((B, H), dtype=bool)
    keep[0, 1] = keep[1, 2] = False
    assert (arg[keep] == -1).all()
    _, idx = _torch_pool(clean, lens, T, np.zeros((B, H)), np.ones((B, H)))
    assert idx[0, 1] == 2 and idx[1, 2] == 3


TIE_SHAPES = [s for s in hp.POOL_SHAPES if s[0] >= 9]       # a tie needs a column of six active rows; these shapes have some


@pytest.mark.parametrize('shape', TIE_SHAPES)
def test_planted_ties_go_to_the_smallest_row(shape):
    T, B, H = shape
    n = 0
    for v in ht.tie_variants(T, B, H):
        arg, _ = _check_against_torch(v, T, B, H, True)
        for b, h, first in v['ties']:
            assert arg[b, h] == first
            n += 1
    assert n >= 3


@pytest.mark.parametrize('shape', hp.POOL_SHAPES)
def test_pow2_lengths_make_the_backward_exact(shape):
    """The fp32 restatement equals the fp64 one value for value on the power-of-two cases: what lets the GPU test ask for bits."""
    T, B, H = shape
    for v in ht.pow2_variants(T, B, H):
        lens = v['lens']
        assert all(int(n) & (int(n) - 1) == 0 and 1 <= n <= v['rows'] for n in lens)
        g_avg, g_max = ht.grad_case(B, H, exact=True)
        arg = ht.pool_train_ref(v['y'], lens, v['rows'])[2]
        a = ht.pool_backward_ref(g_avg, g_max, lens, arg, T, np.float32)
        b = ht.pool_backward_ref(g_avg, g_max, lens, arg, T, np.float64)
        assert np.array_equal(a.astype(np.float64), b)
        _check_against_torch(v, T, B, H, True)


@pytest.mark.parametrize('shape', hp.ATTN_SHAPES)
def test_selfattn_backward_restatement_equals_torch_autograd(shape):
    """fp64 on both sides, different summation orders: 1e-11 is far above H T eps and far below fp32's eps."""
    import torch
    from features.classifier import _SelfAttn
    T, B, H = shape
    y, W, bW, v, c = hp.attn_case(T, B, H)
    g_out = np.random.default_rng(5 + T).standard_normal((B, H)).astype(np.float32)
    mod = _SelfAttn(H).double()
    params = (mod.attn.weight, mod.attn.bias, mod.v.weight, mod.v.bias)
    with torch.no_grad():
        for p, a in zip(params, (W, bW, v, c)):
            p.copy_(torch.from_numpy(a.astype(np.float64)))
    for rows in hp.ATTN_ROWS(T):
        yt = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
        for p in params:
            p.grad = None
        out = mod._run_torch(yt[:rows])
        out.backward(torch.from_numpy(g_out.astype(np.float64)))
        ref = ht.selfattn_rows_train_ref(y, rows, W, bW, v, c, g_out)
        close = lambda got, want: np.max(np.abs(got - want)) <= 1e-11 * max(1.0, float(np.max(np.abs(want))))
        assert close(ref['out'], out.detach().numpy())
        assert close(ref['g_y'], yt.grad.numpy()) and (ref['g_y'][rows:] == 0).all() and (ref['w'][rows:] == 0).all()
        assert abs(ref['w'].sum(0) - 1).max() <= 1e-12
        for key, p in zip(('gW', 'gbW', 'gv', 'gc'), params):
            assert close(ref[key], p.grad.numpy()), key
        assert close(ref['gv_part'].sum(0, keepdims=True), mod.v.weight.grad.numpy())
        f32 = ht.selfattn_rows_train_ref(y, rows, W, bW, v, c, g_out, np.float32)
        assert all(f32[k].dtype == np.float32 for k in ('out', 'w', 'g_y', 'g_pre', 'g_e', 'gv_part'))
        assert np.max(np.abs(f32['g_y'] - ref['g_y'])) <= 2e-5 * max(1.0, float(np.abs(ref['g_y']).max()))


def _lib():
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return nat, nat.load()


def test_new_entry_points_are_declared_bound_and_exported():
    nat, lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    for name in NEW:
        assert name in nat.SIGNATURES and hasattr(lib, name)
        decl = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        assert len(decl.split(',')) == len(nat.SIGNATURES[name][1]), name              # one ctypes type per C parameter
    assert 'caller orders the refresh after earlier uses of the handle on OTHER streams' in re.sub(r'\s*\n \*\s*', ' ', hdr)


def test_argument_errors_come_before_any_device_call():
    """No GPU here: a call that got past its checks would fail differently (or fault).  Every one is DSP_EINVAL with a message."""
    import ctypes as C
    nat, lib = _lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def einval(rc, what):
        assert rc == nat.EINVAL and what in lib.dsp_last_error().decode(), (rc, lib.dsp_last_error())
    einval(lib.dsp_head_pool_train_batch(p, 2, 1, 4, p, p, p, 8, 0, 4, None, None), 'NULL argument')
    einval(lib.dsp_head_pool_train_batch(None, 2, 1, 4, p, p, p, 8, 0, 4, p, None), 'NULL argument')
    einval(lib.dsp_head_pool_train_batch(p, 0, 1, 4, p, p, p, 8, 0, 4, p, None), 'T 0 must be >= 1')
    einval(lib.dsp_head_pool_train_batch(p, 2, 1, 4, p, p, p, 7, 0, 4, p, None), 'ld_feat 7 is below the 8 columns written')
    for k in (0, 4, 5, 9):                                                      # d_gfeat, d_len, d_arg, d_gy
        args = [p, 8, 0, 4, p, p, 2, 1, 4, p, None]
        args[k] = None
        einval(lib.dsp_head_pool_backward_batch(*args), 'NULL argument')
    einval(lib.dsp_head_pool_backward_batch(p, 8, 0, 4, p, p, 0, 1, 4, p, None), 'T 0 must be >= 1')
    einval(lib.dsp_head_pool_backward_batch(p, 8, 0, 4, p, p, 2, 0, 4, p, None), 'B 0 must be >= 1')
    einval(lib.dsp_head_pool_backward_batch(p, 8, 0, 4, p, p, 2, 1, 0, p, None), 'H 0 must be in')
    einval(lib.dsp_head_pool_backward_batch(p, 8, 0, -1, p, p, 2, 1, 4, p, None), 'col_max -1 is negative')
    einval(lib.dsp_head_pool_backward_batch(p, 8, 1, 4, p, p, 2, 1, 4, p, None), 'overlap')
    einval(lib.dsp_head_pool_backward_batch(p, 7, 0, 4, p, p, 2, 1, 4, p, None), 'ld_g 7 is below the 8 columns read')
    einval(lib.dsp_head_pool_backward_batch(p, 3, -1, 0, p, p, 2, 1, 4, p, None), 'ld_g 3 is below the 4 columns read')
    einval(lib.dsp_selfattn_pool_rows_train_batch(p, 1, 1, 4, p, p, p, p, p, p, None, None), 'NULL argument')
    einval(lib.dsp_selfattn_pool_rows_train_batch(p, 1, 1, 4, p, p, p, p, p, None, p, None), 'NULL argument')
    einval(lib.dsp_selfattn_pool_rows_train_batch(p, 0, 1, 4, p, p, p, p, p, p, p, None), 'T 0 must be in [1, 1024]')
    einval(lib.dsp_selfattn_pool_rows_train_batch(p, 1, 1, 6, p, p, p, p, p, p, p, None), 'H 6 must be a multiple of 4')
    einval(lib.dsp_selfattn_pool_rows_backward_batch(p, 1, 1, 4, p, p, p, p, p, p, p, p, p, None, None), 'NULL argument')
    einval(lib.dsp_selfattn_pool_rows_backward_batch(p, 1, 1, 4, p, p, p, None, p, p, p, p, p, p, None), 'NULL argument')
    einval(lib.dsp_selfattn_pool_rows_backward_batch(p, 1025, 1, 4, p, p, p, p, p, p, p, p, p, p, None), 'T 1025 must be in [1, 1024]')
    einval(lib.dsp_bigru_refresh(None, C.byref(nat.BigruDesc()), None), 'NULL argument')
    einval(lib.dsp_hmlstm_refresh(None, C.byref(nat.HmlstmDesc()), None), 'NULL argument')
    einval(lib.dsp_attn_refresh(None, C.byref(nat.AttnDesc()), None), 'NULL argument')
    einval(lib.dsp_bigru_refresh(p, None, None), 'NULL argument')
    einval(lib.dsp_hmlstm_refresh(p, None, None), 'NULL argument')
    einval(lib.dsp_attn_refresh(p, None, None), 'NULL argument')


def test_device_grad_needs_device_len_and_a_gpu():
    """``device_grad=True`` alone is a ValueError on every head and block, before anything else is looked at; with
    ``device_len=True`` on host tensors it is the RuntimeError that names the reason, never a fallback."""
    import torch
    from features import classifier as C
    inp = torch.zeros(6, 2, 39)
    len0 = torch.tensor([6, 3], dtype=torch.int32)
    for cls in (C.RNNHead, C.HRNNHead, C.HRNNAttHead, C.TransformerHead, C.HMRNNHead):
        head = cls().train()
        with pytest.raises(ValueError, match='device_grad=True needs device_len=True'):
            head(inp, len0, device_grad=True)
        with pytest.raises(RuntimeError, match='not on a GPU'):
            head(inp, len0, device_len=True, device_grad=True)
    with pytest.raises(ValueError, match='device_grad=True needs device_len=True'):
        C._DynEnc(12, 20, 2).run(torch.zeros(6, 2, 12), len0, device_grad=True)
    with pytest.raises(ValueError, match='device_grad=True needs device_len=True'):
        C.HMLSTM(1.0, 20, [28, 24]).run(torch.zeros(6, 2, 20), None, lens=len0, device_grad=True)
    with pytest.raises(ValueError, match='device_grad=True needs d_rows'):
        C._SelfAttn(12)(torch.zeros(6, 2, 12), device_grad=True)


def test_train_batch_is_exported_and_enqueue_takes_a_jitter():
    import inspect
    import features
    from features.model_glue import ModelFeatureBatch
    from features.train import TrainBatch
    assert features.TrainBatch is TrainBatch
    assert inspect.signature(ModelFeatureBatch.enqueue).parameters['d_jitter'].default is None
    for name in ('run', 'capture'):
        assert list(inspect.signature(getattr(TrainBatch, name)).parameters)[:5] == ['self', 'waves', 'sample_offsets', 'labels', 'jitter']
