"""The head entry points without a device: the fp64 restatement of tests/head_pool_cases.py against the heads' own torch
expressions (features/classifier.py: ``y[:rows].sum(0) / n``, ``y[:rows].max(0).values``, ``(len + hir - 1) // hir``,
``_SelfAttn._run_torch(y[:rows])``) on the cases the GPU tests run, the surface of the three new entry points, and the
refusals of ``device_len=True`` that need no GPU."""
import os
import re

import numpy as np
import pytest

import head_pool_cases as hp
from conftest import ROOT

NEW = ['dsp_head_lengths_batch', 'dsp_head_pool_batch', 'dsp_selfattn_pool_rows_batch']


@pytest.mark.parametrize('shape', hp.POOL_SHAPES)
def test_pool_restatement_equals_the_heads_expressions(shape):
    """fp64 values on a 1/64 grid: every sum is exact in any order, so the restatement (which reads rows t < len only) and
    the heads' expressions over the zero-padded y[:rows] must be EQUAL."""
    import torch
    T, B, H = shape
    seen = set()
    for v in hp.pool_variants(T, B, H, exact=True):
        rows, lens = v['rows'], v['lens']
        avg, mx = hp.pool_ref(v['y'], lens, rows)                                   # NaNs behind every end: never read
        y = torch.from_numpy(v['clean'].astype(np.float64))[:rows]                  # what the encoders leave: exact zeros
        n = torch.from_numpy(lens.astype(np.float64))
        want_avg, want_mx = (y.sum(0) / n.unsqueeze(1)).numpy(), y.max(0).values.numpy()
        assert np.array_equal(avg, want_avg, equal_nan=True) and np.array_equal(mx, want_mx, equal_nan=True)
        for b in v['neg_eq']:
            assert lens[b] == rows < T and (mx[b] < 0).all()
            seen.add('eq')
        for b in v['neg_lt']:
            assert lens[b] < rows and (mx[b] == 0).all()
            seen.add('lt')
        seen |= {'one'} if (lens == 1).any() else set()
        seen |= {'full'} if (lens == T).any() else set()
        if v['nan_at'] is not None:
            t, b, h = v['nan_at']
            assert t < lens[b]
            bad = np.zeros((B, H), dtype=bool)
            bad[b, h] = True
            assert np.array_equal(np.isnan(avg), bad) and np.array_equal(np.isnan(mx), bad)      # exactly that column
            seen.add('nan')
        else:
            assert np.isfinite(avg).all() and np.isfinite(mx).all()
    assert seen == ({'eq', 'lt', 'one', 'full', 'nan'} if T >= 3 else {'one', 'full', 'nan'})


def test_lengths_restatement_equals_the_heads_expression():
    T = hp.LENGTH_T
    for B in hp.LENGTH_B:
        len0, n_bad = hp.length_case(B)
        for hir in hp.LENGTH_HIR:
            c, len1, info = hp.lengths_ref(len0, T, hir)
            assert ((1 <= c) & (c <= T)).all() and info[2] == n_bad == np.sum((len0 < 1) | (len0 > T))
            assert np.array_equal(len1, (c + hir - 1) // hir)                       # rnn_clf.py:52 on the clamped lengths
            assert info[0] == c.max() and info[1] == len1.max() and info[3] == 0
            ok = (len0 >= 1) & (len0 <= T)
            assert np.array_equal(c[ok], len0[ok])


@pytest.mark.parametrize('shape', hp.ATTN_SHAPES)
def test_selfattn_restatement_equals_the_torch_chain(shape):
    """Both sides in fp64; they sum in different orders, so equal means to fp64 rounding: 1e-12 is four orders above
    H eps = 200 x 2.2e-16 and seven below fp32's eps."""
    import torch
    from features.classifier import _SelfAttn
    T, B, H = shape
    y, W, bW, v, c = hp.attn_case(T, B, H)
    mod = _SelfAttn(H).double()
    with torch.no_grad():
        for p, a in zip((mod.attn.weight, mod.attn.bias, mod.v.weight, mod.v.bias), (W, bW, v, c)):
            p.copy_(torch.from_numpy(a.astype(np.float64)))
        for rows in hp.ATTN_ROWS(T):
            want = mod._run_torch(torch.from_numpy(y.astype(np.float64))[:rows]).numpy()
            got = hp.selfattn_rows_ref(y, rows, W, bW, v, c)
            assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, float(np.max(np.abs(want))))


def test_new_entry_points_are_declared_bound_and_exported():
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    lib = nat.load()
    for name in NEW:
        assert name in nat.SIGNATURES and hasattr(lib, name)
        decl = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        assert len(decl.split(',')) == len(nat.SIGNATURES[name][1]), name              # one ctypes type per C parameter


def test_argument_errors_come_before_any_device_call():
    """No GPU here: a call that got past its checks would fail differently (or fault).  Every one is DSP_EINVAL with a message."""
    import ctypes as C
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    def einval(rc, what):
        assert rc == nat.EINVAL and what in lib.dsp_last_error().decode(), (rc, lib.dsp_last_error())
    einval(lib.dsp_head_lengths_batch(None, 4, 200, 5, p, p, p, None), 'NULL argument')
    einval(lib.dsp_head_lengths_batch(p, 0, 200, 5, p, p, p, None), 'B 0 must be in [1, 65535]')
    einval(lib.dsp_head_lengths_batch(p, 65536, 200, 5, p, p, p, None), 'B 65536 must be in [1, 65535]')
    einval(lib.dsp_head_lengths_batch(p, 4, 0, 5, p, p, p, None), 'T 0 must be >= 1')
    einval(lib.dsp_head_lengths_batch(p, 4, 200, 0, p, p, p, None), 'hir 0 must be >= 1')
    einval(lib.dsp_head_pool_batch(None, 2, 1, 4, p, p, p, 8, 0, 4, None), 'NULL argument')
    einval(lib.dsp_head_pool_batch(p, 2, 1, 4, None, p, p, 8, 0, 4, None), 'NULL argument')
    einval(lib.dsp_head_pool_batch(p, 0, 1, 4, p, p, p, 8, 0, 4, None), 'T 0 must be >= 1')
    einval(lib.dsp_head_pool_batch(p, 2, 0, 4, p, p, p, 8, 0, 4, None), 'B 0 must be >= 1')
    einval(lib.dsp_head_pool_batch(p, 2, 1, 0, p, p, p, 8, 0, 4, None), 'H 0 must be in')
    einval(lib.dsp_head_pool_batch(p, 2, 1, 4, p, p, p, 8, 0, -1, None), 'col_max -1 is negative')
    einval(lib.dsp_head_pool_batch(p, 2, 1, 4, p, p, p, 8, 1, 4, None), 'overlap')
    einval(lib.dsp_head_pool_batch(p, 2, 1, 4, p, p, p, 7, 0, 4, None), 'ld_feat 7 is below the 8 columns written')
    einval(lib.dsp_selfattn_pool_rows_batch(p, 1, 1, 4, p, p, p, p, p, None, None), 'NULL argument')
    einval(lib.dsp_selfattn_pool_rows_batch(p, 0, 1, 4, p, p, p, p, p, p, None), 'T 0 must be in [1, 1024]')
    einval(lib.dsp_selfattn_pool_rows_batch(p, 1, 1, 6, p, p, p, p, p, p, None), 'H 6 must be a multiple of 4')


def test_device_len_refuses_what_it_cannot_serve_on_the_cpu():
    """``device_len=True`` never falls back: host tensors raise the RuntimeError that names the reason, and the default
    (``device_len=False``) still takes a tensor of lengths through the host as before."""
    import torch
    from features import classifier as C
    inp = torch.zeros(6, 2, 39)
    len0 = torch.tensor([6, 3], dtype=torch.int32)
    for cls in (C.RNNHead, C.HRNNHead, C.HRNNAttHead, C.TransformerHead, C.HMRNNHead):
        head = cls().eval()
        with torch.no_grad():
            with pytest.raises(RuntimeError, match='not on a GPU'):
                head(inp, len0, device_len=True)
            out = head(inp, len0, device_len=False)
            assert (out[0] if isinstance(out, tuple) else out).shape == (2, 20)
    with pytest.raises(TypeError, match='int32 device tensor'):
        C.head_length_info(len0, 6, 5)
