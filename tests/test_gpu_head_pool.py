"""The three head entry points on the device (csrc/kernels_head.h, csrc/dsp_attn.hip): ``dsp_head_pool_batch`` and
``dsp_head_lengths_batch`` against the fp64 restatement of tests/head_pool_cases.py (which tests/test_head_pool_host.py pins to
the heads' own torch expressions), ``dsp_selfattn_pool_rows_batch`` against ``dsp_selfattn_pool_batch`` on ``y[:rows]``.

The shapes are the smallest at which the pooling can go wrong: one row, fewer rows than the four waves a column's time axis
is split over, H below one float4 group's 256 columns and not a multiple of 4 (the scalar route), more rows than one pass of
the waves, H = 200 (the heads').  NaNs fill every row t >= len of the input: a kernel that read one would show it."""
import numpy as np
import pytest

import head_pool_cases as hp
from conftest import record

pytestmark = pytest.mark.gpu

BAR = 2e-5                 # the BAR of tests/test_gpu_attn.py: error <= BAR * max(1, max |ref|)
SENT = np.float32(-12345.5)


def _dev():
    import torch
    return torch.device('cuda', 0)


def _err(got, ref):
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got.astype(np.float64)[ok] - ref[ok]))) / max(1.0, float(np.max(np.abs(ref[ok]))))


def _pool(yd, lens_d, rows_d, H, ld, col_avg, col_max, feat=None, stream=None):
    """One call on a [B, ld] tensor prefilled with a sentinel -> that tensor."""
    import torch
    from features import _native as nat
    T, B, _ = yd.shape
    dev = yd.device
    if feat is None:
        feat = torch.full((B, ld), float(SENT), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev) if stream is None else stream
    nat.check(nat.load().dsp_head_pool_batch(yd.data_ptr(), T, B, H, lens_d.data_ptr(), None if rows_d is None else rows_d.data_ptr(),
                                             feat.data_ptr(), ld, col_avg, col_max, st.cuda_stream))
    return feat


@pytest.mark.parametrize('shape', hp.POOL_SHAPES)
def test_pool_kernel_against_the_restatement(shape):
    import torch
    T, B, H = shape
    dev = _dev()
    ld, ca, cm = 2 * H + 7, 2, H + 5            # ld_feat > 2 H: sentinels in front of, between and behind the written columns
    seen = set()
    for k, v in enumerate(hp.pool_variants(T, B, H)):
        rows, lens = v['rows'], v['lens']
        want_avg, want_mx = hp.pool_ref(v['y'], lens, rows)
        yd = torch.from_numpy(v['y']).to(dev)
        lens_d = torch.from_numpy(lens).to(dev)
        rows_d = torch.tensor([rows], dtype=torch.int32, device=dev)
        feat = _pool(yd, lens_d, rows_d, H, ld, ca, cm)
        got = feat.cpu().numpy()
        avg, mx = got[:, ca:ca + H], got[:, cm:cm + H]
        # the max half: the same values, NaNs in the same places
        assert np.array_equal(mx.astype(np.float64), want_mx, equal_nan=True), (shape, k)
        assert np.array_equal(np.isnan(avg), np.isnan(want_avg)), (shape, k)
        e = record('head_pool_avg_vs_fp64', _err(avg, want_avg))
        print(f'pool {shape} variant {k} rows {rows}: avg err {e:.3g}')
        assert e <= BAR
        for b in v['neg_eq']:
            assert lens[b] == rows < T and (mx[b] < 0).all()
            seen.add('eq')
        for b in v['neg_lt']:
            assert lens[b] < rows and (mx[b] == 0).all()
            seen.add('lt')
        seen |= ({'one'} if (lens == 1).any() else set()) | ({'full'} if (lens == T).any() else set())
        if v['nan_at'] is not None:
            bad = np.zeros((B, H), dtype=bool)
            bad[v['nan_at'][1], v['nan_at'][2]] = True
            assert np.array_equal(np.isnan(avg), bad) and np.array_equal(np.isnan(mx), bad)      # exactly that column
            seen.add('nan')
        else:                                                    # the NaNs behind every end did not reach the output
            assert np.isfinite(avg).all() and np.isfinite(mx).all()
        keep = np.ones(ld, dtype=bool)
        keep[ca:ca + H] = keep[cm:cm + H] = False
        assert (got[:, keep] == SENT).all()                      # only feat[b, col .. col + H) is written
        # col_avg = -1: the average's columns stay untouched, the max half is the same
        only = _pool(yd, lens_d, rows_d, H, ld, -1, cm).cpu().numpy()
        keep[ca:ca + H] = True
        assert (only[:, keep] == SENT).all() and np.array_equal(only[:, cm:cm + H], mx, equal_nan=True)
        # d_rows NULL: rows = T
        full = _pool(yd, lens_d, None, H, ld, ca, cm).cpu().numpy()
        assert np.array_equal(full[:, cm:cm + H].astype(np.float64), hp.pool_ref(v['y'], lens, None)[1], equal_nan=True)
        # the same bytes twice and on a side stream
        again = _pool(yd, lens_d, rows_d, H, ld, ca, cm)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            other = _pool(yd, lens_d, rows_d, H, ld, ca, cm, stream=side)
        side.synchronize()
        for t in (again, other):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), got.view(np.uint32))
    assert seen == ({'eq', 'lt', 'one', 'full', 'nan'} if T >= 3 else {'one', 'full', 'nan'})


def test_pool_kernel_scalar_route_on_a_misaligned_view_and_clamped_lengths():
    """H a multiple of 4 but y 4 bytes off a 16-byte boundary takes the scalar loads; lengths outside [1, T] are clamped."""
    import torch
    dev = _dev()
    T, B, H = 9, 5, 12
    rng = np.random.default_rng(4)
    y = rng.standard_normal((T, B, H)).astype(np.float32)
    lens = np.array([0, -4, T + 3, 5, T], dtype=np.int32)
    base = torch.zeros(T * B * H + 1, dtype=torch.float32, device=dev)
    yd = base[1:].view(T, B, H)
    yd.copy_(torch.from_numpy(y))
    assert yd.data_ptr() % 16 == 4
    lens_d = torch.from_numpy(lens).to(dev)
    got = _pool(yd, lens_d, None, H, 2 * H, 0, H).cpu().numpy()
    aligned = _pool(torch.from_numpy(y).to(dev), lens_d, None, H, 2 * H, 0, H).cpu().numpy()
    want_avg, want_mx = hp.pool_ref(y, lens, None)
    assert np.array_equal(got[:, H:].astype(np.float64), want_mx) and _err(got[:, :H], want_avg) <= BAR
    assert np.array_equal(got.view(np.uint32), aligned.view(np.uint32))          # both routes sum in the same order


def test_lengths_kernel_exact():
    import torch
    from features.classifier import head_length_info
    dev = _dev()
    T = hp.LENGTH_T
    for B in hp.LENGTH_B:
        len0, n_bad = hp.length_case(B)
        d = torch.from_numpy(len0).to(dev)
        for hir in hp.LENGTH_HIR:
            c, len1, info = (t.cpu().numpy() for t in head_length_info(d, T, hir))
            wc, w1, wi = hp.lengths_ref(len0, T, hir)
            assert c.dtype == len1.dtype == info.dtype == np.int32
            assert np.array_equal(c, wc) and np.array_equal(len1, w1) and np.array_equal(info, wi), (B, hir)
            assert info[2] == n_bad == min(3, B)
        assert np.array_equal(d.cpu().numpy(), len0)             # the input is left as it was


@pytest.mark.parametrize('shape', hp.ATTN_SHAPES)
def test_selfattn_rows_equals_the_entry_point_on_the_first_rows(shape):
    import torch
    from features import _native as nat
    T, B, H = shape
    dev = _dev()
    lib = nat.load()
    y, W, bW, v, c = hp.attn_case(T, B, H)
    yd, Wd, bd, vd, cd = (torch.from_numpy(a).to(dev) for a in (y, W, bW, v, c))
    st = torch.cuda.current_stream(dev).cuda_stream
    for rows in hp.ATTN_ROWS(T):
        want = torch.empty(B, H, dtype=torch.float32, device=dev)
        head = yd[:rows].contiguous()
        nat.check(lib.dsp_selfattn_pool_batch(head.data_ptr(), rows, B, H, Wd.data_ptr(), bd.data_ptr(), vd.data_ptr(), cd.data_ptr(),
                                              want.data_ptr(), st))
        poisoned = yd.clone()
        poisoned[rows:] = float('nan')                           # rows behind the count are not part of the result
        got = torch.full((B, H), float(SENT), dtype=torch.float32, device=dev)
        rows_d = torch.tensor([rows], dtype=torch.int32, device=dev)
        nat.check(lib.dsp_selfattn_pool_rows_batch(poisoned.data_ptr(), T, B, H, Wd.data_ptr(), bd.data_ptr(), vd.data_ptr(), cd.data_ptr(),
                                                   got.data_ptr(), rows_d.data_ptr(), st))
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), (shape, rows)
        ref = hp.selfattn_rows_ref(y, rows, W, bW, v, c)
        assert record('selfattn_rows_vs_fp64', _err(got.cpu().numpy(), ref)) <= BAR
