"""The row-bounded column sums on the GPU, alone (include/dsp_frontend.h: dsp_rows_colsum; csrc/kernels_reduce.h), against the
fp64 sum.  The smallest shapes at which the two kernels can go wrong: one element; fewer columns than a narrow block and more
(7, 39); a partial 64-column block behind full ones on a strided slice (600 of 800); one and several chunks of 8 time steps
with a partial last one; T = 1; a [T, B] view of scalars whose rows run over several wave-sized row sets; chunks of more than
256 rows, where a thread of the narrow kernel owns several rows, and batch sizes that do not divide the kernels' row strides.

  * bar: 2e-5 of the largest magnitude of the fp64 result, per tensor (the project's bar between fp32 and fp64); the one- and
    seven-column cases are drawn from uniform(0.5, 1.5), so their sums are far from cancellation;
  * the bound: R in {1, 8, 9, T} -- below, at and behind a chunk edge -- clamped to T; rows >= R of the whole buffer are NaN;
    the result is finite and EQUAL under == to the call without a bound on a dense copy of the first R rows;
  * every result equals the NumPy restatement (tools/rows_sum_emul.py) bit for bit;
  * the output and the scratch sit between guard words that stay untouched; two calls give equal bits; a view whose pointer
    is only 4-byte aligned gives the aligned call's bits;
  * ``features.wgrad.rows_colsum`` -- the call the heads make -- gives the same bits through tensor strides."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, record

pytestmark = pytest.mark.gpu

BAR = 2e-5
GUARD, SENTINEL = 64, 1234.5            # floats on either side of the output and the scratch (256 bytes: alignment is kept)

_spec = importlib.util.spec_from_file_location('rows_sum_emul', os.path.join(ROOT, 'tools', 'rows_sum_emul.py'))
emul = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(emul)

# name -> (T, B, cols, shape of the buffer, how the [T, B, cols] view is cut from it, uniform data?)
CASES = {
    'one':      (1, 1, 1, (1, 1, 1), lambda t: t, True),
    'seven':    (3, 5, 7, (3, 5, 7), lambda t: t, True),
    'narrow39': (20, 3, 39, (20, 3, 39), lambda t: t, False),
    'da_slice': (17, 5, 600, (17, 5, 2, 800), lambda t: t[:, :, 1, :600], False),
    'wide200':  (9, 64, 200, (9, 64, 200), lambda t: t, False),
    'bias400':  (1, 17, 400, (1, 17, 400), lambda t: t, False),
    'scalars':  (200, 32, 1, (200, 32), lambda t: t.unsqueeze(2), True),
    # more than 256 rows per chunk: every thread of the narrow kernel walks its rows tid, tid + 256, .. (2400 and 800 rows a chunk)
    'rows300':  (9, 300, 7, (9, 300, 7), lambda t: t, True),
    'rows100':  (16, 100, 1, (16, 100), lambda t: t.unsqueeze(2), True),
    # ... and more than 16 rows per row group with B no divisor of 16: the wide kernel's (t, b) carry
    'wide_b5':  (9, 5, 70, (9, 5, 70), lambda t: t, False),
}
BOUNDS = (1, 8, 9, None)                # None: T


def _dev():
    import torch
    from features import _native as nat
    nat.require_device()
    return torch.device('cuda', 0)


def _guarded(numel, dev):
    import torch
    whole = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = whole[GUARD:GUARD + numel]
    view.fill_(float('nan'))
    return whole, view


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def colsum(a, x, rows, dev):
    """``dsp_rows_colsum`` through the C ABI on the device views ``a`` / ``x`` ([T, B, cols]; x or None) with the bound ``rows``
    (None: NULL) -> the [cols] result as a NumPy array.  Output and scratch are NaN-filled and guarded; the scratch is exactly
    the bytes the library asks for."""
    import torch
    from features import _native as nat
    lib = nat.load()
    T, B, cols = a.shape
    nbytes = nat.c_i64(0)
    nat.check(lib.dsp_rows_colsum_scratch_bytes(T, B, cols, C.byref(nbytes)))
    assert nbytes.value == emul.scratch_bytes(T, B, cols)
    out_whole, out = _guarded(cols, dev)
    scr_whole, scr = _guarded(nbytes.value // 4, dev)
    d_rows = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=dev)
    op = lambda t: nat.RowsOperand(t.data_ptr(), t.stride(0), t.stride(1), cols, 0)
    oa, ox = op(a), None if x is None else op(x)
    nat.check(lib.dsp_rows_colsum(C.byref(oa), None if ox is None else C.byref(ox), T, B, None if d_rows is None else d_rows.data_ptr(),
                                  out.data_ptr(), scr.data_ptr(), nbytes.value, torch.cuda.current_stream(dev).cuda_stream))
    got = out.cpu().numpy()
    assert _guards_intact(out_whole) and _guards_intact(scr_whole), 'a guard word around the output or the scratch was written'
    return got


def _buffers(name, dev):
    """The case's two buffers on the host (fp32) and the device."""
    import torch
    T, B, cols, shape, cut, uniform = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    draw = (lambda: rng.uniform(0.5, 1.5, shape)) if uniform else (lambda: rng.standard_normal(shape))
    host = [torch.from_numpy(draw().astype(np.float32)) for _ in range(2)]
    return host, [h.to(dev) for h in host], cut


def _misaligned(buf, cut, dev):
    """The same values 4 bytes behind a 16-byte boundary, cut the same way."""
    import torch
    base = torch.empty(buf.numel() + 1, dtype=torch.float32, device=dev)
    base[1:].copy_(buf.reshape(-1))
    v = cut(base[1:].view(buf.shape))
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize('with_x', [False, True], ids=['plain', 'times_x'])
@pytest.mark.parametrize('name', list(CASES))
def test_colsum_against_fp64_bounds_bits_and_guards(name, with_x):
    import torch
    from features.wgrad import rows_colsum
    dev = _dev()
    T, B, cols = CASES[name][:3]
    host, bufs, cut = _buffers(name, dev)
    ha, hx = cut(host[0]).numpy(), cut(host[1]).numpy() if with_x else None
    worst = 0.0
    for bound in BOUNDS:
        R = T if bound is None else min(bound, T)
        ref = (ha[:R].astype(np.float64) * (hx[:R].astype(np.float64) if with_x else 1.0)).sum((0, 1))
        # rows behind R of the WHOLE buffers are NaN: nothing there may be read
        nan = [b.clone() for b in bufs]
        for b in nan:
            b[R:] = float('nan')
        a, x = cut(nan[0]), cut(nan[1]) if with_x else None
        got = colsum(a, x, bound, dev)
        assert got.shape == (cols,) and np.isfinite(got).all(), (name, bound)
        err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
        worst = max(worst, err)
        print(f'{name} with_x={with_x} R={R}: error {err:.3e} of max |ref| {np.max(np.abs(ref)):.4g}')
        assert err <= BAR, (name, with_x, bound, err)
        # the same bits: again; without a bound on a dense copy of the first R rows; from a 4-byte-aligned view; through the
        # tensor strides; and from the NumPy restatement
        assert np.array_equal(got, colsum(a, x, bound, dev)), (name, bound, 'second run')
        dense = colsum(a[:R].contiguous(), None if x is None else x[:R].contiguous(), None, dev)
        assert np.array_equal(got, dense), (name, bound, 'bounded call differs from the call on R rows')
        mis = colsum(_misaligned(nan[0], cut, dev), _misaligned(nan[1], cut, dev) if with_x else None, bound, dev)
        assert np.array_equal(got, mis), (name, bound, 'a 4-byte-aligned view gives other bits')
        d_rows = None if bound is None else torch.tensor([bound], dtype=torch.int32, device=dev)
        assert np.array_equal(got, rows_colsum(a, x, d_rows).cpu().numpy()), (name, bound, 'features.wgrad.rows_colsum')
        assert np.array_equal(got, emul.colsum(ha, hx, R)), (name, bound, 'the NumPy restatement gives other bits')
    record('rows_colsum_vs_fp64', worst)


def test_bound_word_is_clamped():
    """0 and negative act as 1, anything above T as T, and T as no bound at all."""
    import torch
    dev = _dev()
    host, bufs, cut = _buffers('wide200', dev)
    a = cut(bufs[0])
    T = a.shape[0]
    at = {r: colsum(a, None, r, dev) for r in (0, -3, 1, T, T + 5)}
    assert np.array_equal(at[0], at[1]) and np.array_equal(at[-3], at[1])
    assert np.array_equal(at[T + 5], at[T]) and np.array_equal(at[T], colsum(a, None, None, dev))
    assert not np.array_equal(at[1], at[T])


def test_wrapper_refusals():
    import torch
    from features.wgrad import rows_colsum
    dev = _dev()
    a = torch.zeros(4, 3, 8, device=dev)
    with pytest.raises(TypeError, match='float32 device tensor'):
        rows_colsum(a.double())
    with pytest.raises(TypeError, match='float32 device tensor'):
        rows_colsum(a[0])
    a.copy_(torch.arange(96, device=dev).view(4, 3, 8))
    assert torch.equal(rows_colsum(a.transpose(1, 2)), a.sum((0, 2)))     # no unit column stride: copied first (exact integers)
    with pytest.raises(ValueError, match='does not match'):
        rows_colsum(a, a[:2])
    with pytest.raises(TypeError, match='one-element int32'):
        rows_colsum(a, d_rows=torch.zeros(1, device=dev))
    with pytest.raises(ValueError, match='cols 4096'):
        rows_colsum(torch.zeros(1, 1, 4096, device=dev))
