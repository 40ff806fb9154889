"""The row-bounded products on the GPU, alone (include/dsp_frontend.h: dsp_rows_wgrad, dsp_rows_product; csrc/kernels_wgrad.h),
against the NumPy fp64 interpreter of tests/wgrad_cases.py.  The smallest shapes that can go wrong: every edge of the 16-wide
MFMA tiles and of the 128-wide workgroup tile's bounds checks, one and several chunks of 8 time steps with a partial last one,
the three shifts with and without an initial row, [B, T, H] strides, column-offset views whose row stride exceeds their columns,
the scale and the column sums on and off.

  * bar: 2e-5 max(1, max |ref|) per tensor, the project's bar between fp32 and fp64 (tests/test_gpu_device_train.py);
  * the bound: d_rows in {NULL, 0 (acts as 1), 1, a chunk edge, one inside a chunk, T, T + 5 (acts as T)}; rows >= R of every
    operand are NaN; the result is finite and EQUAL under == to the NULL call on dense buffers truncated to R rows;
  * the row product writes every element of a NaN-filled Y, exact +0.0 at rows >= R;
  * outputs and scratch sit between guard words that stay untouched; two calls give equal bits; a view whose pointers are
    only 4-byte aligned gives the aligned call's bits;
  * one case at the heads' own width (T = 200, B = 32, m = 600, n = 400, R = 131), its error recorded beside torch's fp32
    ``a.t() @ x`` on the same operands."""
import ctypes as C

import numpy as np
import pytest

import wgrad_cases as wc
from conftest import record

pytestmark = pytest.mark.gpu

BAR = 2e-5
GUARD, SENTINEL = 64, 1234.5            # floats on either side of every output (256 bytes: 16-byte alignment is kept)


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


def _word(v, dev):
    import torch
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=dev)


def launch(plan, rows, dev, misalign=False):
    """Every product of ``plan`` (CPU fp32 buffers) through the C ABI with the bound ``rows`` (None: NULL) -> name -> CPU tensor.
    Outputs and scratch are NaN-filled and guarded.  ``misalign``: every buffer and output starts 4 bytes behind a 16-byte
    boundary."""
    import torch
    from features import _native as nat
    lib = nat.load()
    T, B = plan.T, plan.B
    bufs = {}
    for k, v in plan.buffers.items():
        if misalign:
            base = torch.empty(v.numel() + 1, dtype=torch.float32, device=dev)
            base[1:].copy_(v.reshape(-1))
            bufs[k] = base[1:]
            assert bufs[k].data_ptr() % 16 == 4
        else:
            bufs[k] = v.to(dev).contiguous()
            assert bufs[k].data_ptr() % 16 == 0
    d_rows = _word(rows, dev)
    rp = None if d_rows is None else d_rows.data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    operand = lambda op: nat.RowsOperand(bufs[op['buf']].data_ptr() + 4 * op['offset'], op['stride_t'], op['stride_b'], op['cols'], 0)
    addr = lambda ref: None if ref is None else bufs[ref['buf']].data_ptr() + 4 * ref['offset']
    outs, wholes = {}, []
    off = 1 if misalign else 0

    def out(numel):
        whole, view = _guarded(numel + off, dev)
        wholes.append(whole)
        return view[off:]
    for p in plan.products:
        if p['kind'] == 'wgrad':
            m, n = p['a']['cols'], p['x']['cols']
            nbytes = nat.c_i64(0)
            nat.check(lib.dsp_rows_wgrad_scratch_bytes(T, B, m, n, C.byref(nbytes)))
            whole, scratch = _guarded(nbytes.value // 4, dev)
            wholes.append(whole)
            c = out(m * n)
            cs = out(m) if p['colsum'] is not None else None
            a, x = operand(p['a']), operand(p['x'])
            nat.check(lib.dsp_rows_wgrad(C.byref(a), C.byref(x), p['shift'], addr(p['init']), p['init']['stride_b'] if p['init'] else 0,
                                         addr(p['scale']), T, B, rp, c.data_ptr(), None if cs is None else cs.data_ptr(),
                                         scratch.data_ptr(), nbytes.value, st))
            outs[p['out']] = c.view(m, n)
            if cs is not None:
                outs[p['colsum']] = cs
        else:
            ops = [operand(a) for a, _ in p['terms']]
            ws = [addr(w) for _, w in p['terms']]
            y = out(T * B * p['n'])
            nat.check(lib.dsp_rows_product(C.byref(ops[0]), ws[0], C.byref(ops[1]) if len(ops) > 1 else None, ws[1] if len(ops) > 1 else None,
                                           p['n'], T, B, rp, y.data_ptr(), st))
            outs[p['out']] = y.view(T, B, p['n'])
    torch.cuda.synchronize(dev)
    assert all(_guards_intact(w) for w in wholes), 'a guard word was written'
    return {k: v.cpu() for k, v in outs.items()}


def _check(tag, got, ref):
    worst = 0.0
    for k, r in ref.items():
        g = got[k].numpy().astype(np.float64)
        assert g.shape == r.shape and np.isfinite(g).all(), (tag, k)
        e = float(np.max(np.abs(g - r))) / max(1.0, float(np.max(np.abs(r))))
        worst = max(worst, e)
        assert e <= BAR, (tag, k, e)
    return worst


def _bounds(T, steps=8):
    """NULL, 0, 1, a chunk edge, one inside a chunk, T, T + 5 -- those that differ for this T."""
    inside = [v for v in (steps, steps + 3, 2 * steps + 1) if 1 < v < T]
    return [None, 0, 1] + inside + [T, T + 5]


# (m, n, T, B, shift, init, scale, colsum, layout of a, layout of x)
REDUCTIONS = [
    (1, 1, 1, 1, 0, False, False, True, 'tb', 'tb'),
    (15, 39, 2, 3, -1, True, True, True, 'tb', 'tb'),
    (16, 64, 9, 5, 0, False, False, False, 'tb', 'tb'),
    (17, 81, 23, 16, 1, False, True, True, 'off', 'tb'),
    (75, 39, 23, 33, -1, False, False, True, 'tb', 'bt'),
    (75, 81, 9, 3, -1, True, True, False, 'off', 'bt'),
    (17, 1, 23, 1, 1, False, False, True, 'tb', 'off'),
    (1, 64, 2, 33, 0, False, True, False, 'bt', 'bt'),
    (16, 81, 23, 5, -1, True, False, True, 'off', 'off'),
    (15, 64, 9, 16, 1, False, True, True, 'off', 'off'),
    (75, 1, 1, 5, -1, True, False, False, 'tb', 'tb'),
    (39, 17, 23, 3, 0, False, True, True, 'bt', 'off'),
]


@pytest.mark.parametrize('case', REDUCTIONS, ids=lambda c: 'm{}n{}T{}B{}s{}{}{}{}{}{}'.format(*[int(v) if isinstance(v, bool) else v for v in c]))
def test_row_reduction_against_fp64_under_every_bound(case):
    m, n, T, B, shift, init, scale, colsum, la, lx = case
    dev = _dev()
    plan = wc.wgrad_case(100 + REDUCTIONS.index(case), m, n, T, B, shift, init, scale, colsum, la, lx)
    worst = 0.0
    for rows in _bounds(T):
        R = wc.bound(rows, T)
        got = launch(wc.poisoned(plan, R), rows, dev)
        worst = max(worst, _check((case, rows), got, wc.interpret(plan, rows=rows)))
        cut = launch(wc.truncated(plan, R), None, dev)
        for k in got:
            assert np.array_equal(got[k].numpy(), cut[k].numpy()), (case, rows, k)
    record('wgrad_reduction_vs_fp64', worst)


# (ks, n, T, B, layouts)
PRODUCTS = [
    ((1,), 1, 1, 1, ('tb',)),
    ((15,), 39, 2, 3, ('off',)),
    ((16, 17), 64, 9, 5, ('tb', 'off')),
    ((75,), 81, 23, 16, ('bt',)),
    ((17, 75), 39, 23, 33, ('off', 'off')),
    ((39, 1), 17, 23, 1, ('bt', 'tb')),
    ((16,), 15, 9, 33, ('tb',)),
]


@pytest.mark.parametrize('case', PRODUCTS, ids=lambda c: 'k{}n{}T{}B{}'.format('_'.join(map(str, c[0])), *c[1:4]))
def test_row_product_writes_every_element_and_zeros_behind_the_bound(case):
    ks, n, T, B, layouts = case
    dev = _dev()
    plan = wc.product_case(200 + PRODUCTS.index(case), ks, n, T, B, layouts)
    worst = 0.0
    for rows in _bounds(T):
        R = wc.bound(rows, T)
        got = launch(wc.poisoned(plan, R), rows, dev)                 # Y was NaN-filled: every element must have been written
        worst = max(worst, _check((case, rows), got, wc.interpret(plan, rows=rows)))
        y = got['y'].numpy()
        assert not y[R:].any() and not np.signbit(y[R:]).any(), (case, rows)          # exact +0.0
        cut = launch(wc.truncated(plan, R), None, dev)
        assert np.array_equal(y[:R], cut['y'].numpy()), (case, rows)
    record('wgrad_product_vs_fp64', worst)


@pytest.mark.parametrize('rows', [None, 11])
def test_same_bits_twice_and_from_a_4_byte_aligned_view(rows):
    dev = _dev()
    for plan in (wc.wgrad_case(7, 75, 81, 23, 5, -1, True, True, True, 'off', 'bt'), wc.wgrad_case(8, 16, 64, 23, 16, 1, False, False, True),
                 wc.product_case(9, (16, 75), 64, 23, 5, ('tb', 'off')), wc.product_case(10, (64,), 16, 23, 16)):
        a, b, c = launch(plan, rows, dev), launch(plan, rows, dev), launch(plan, rows, dev, misalign=True)
        for k in a:
            assert np.array_equal(a[k].numpy().view(np.int32), b[k].numpy().view(np.int32)), k
            assert np.array_equal(a[k].numpy().view(np.int32), c[k].numpy().view(np.int32)), k


def test_run_plan_is_the_same_launches():
    """features.wgrad.run_plan on device buffers: the outputs of the direct calls above, bit for bit."""
    import copy
    import torch
    from features.wgrad import run_plan
    dev = _dev()
    plan = wc.wgrad_case(3, 39, 17, 23, 3, -1, True, True, True, 'bt', 'off')
    extra = wc.product_case(4, (39,), 17, 23, 3)
    plan.products += extra.products
    plan.buffers.update(extra.buffers)
    plan.outputs.update(extra.outputs)
    want = launch(plan, 11, dev)
    on = copy.copy(plan)
    on.buffers = {k: v.to(dev) for k, v in plan.buffers.items()}
    got = run_plan(on, _word(11, dev), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert set(got) == set(want) == {'c', 'cs', 'y'}
    for k in want:
        assert torch.equal(got[k].cpu().reshape(-1), want[k].reshape(-1)), k
    with pytest.raises(TypeError, match='one-element int32'):
        run_plan(on, torch.tensor([1, 2], dtype=torch.int32, device=dev), torch.cuda.current_stream(dev).cuda_stream)


def test_the_heads_own_width():
    """T = 200, B = 32, m = 600, n = 400, R = 131: every workgroup tile, 17 of 25 chunks.  The error against fp64 is recorded
    beside that of torch's fp32 ``a.t() @ x`` over the same 131 rows."""
    import torch
    dev = _dev()
    T, B, m, n, R = 200, 32, 600, 400, 131
    plan = wc.wgrad_case(12, m, n, T, B, 0, False, False, True, 'off', 'tb')
    ref = wc.interpret(plan, rows=R)
    got = launch(wc.poisoned(plan, R), R, dev)
    e = _check('heads_width', got, ref)
    a = torch.from_numpy(wc.gather(plan.buffers['a'].reshape(-1).numpy(), plan.products[0]['a'], range(R), B)).to(dev).reshape(R * B, m)
    x = plan.buffers['x'][:R].to(dev).reshape(R * B, n)
    t = (a.t() @ x).cpu().numpy().astype(np.float64)
    et = float(np.max(np.abs(t - ref['c']))) / max(1.0, float(np.max(np.abs(ref['c']))))
    record('wgrad_heads_width_vs_fp64', e)
    record('wgrad_heads_width_torch_fp32_vs_fp64', et)
    print(f'T 200, B 32, m 600, n 400, R 131: native {e:.3g}, torch fp32 {et:.3g} of max |ref| against fp64')
    cut = launch(wc.truncated(plan, R), None, dev)
    for k in got:
        assert np.array_equal(got[k].numpy(), cut[k].numpy()), k
