"""The attention blocks' backward without a device: the NumPy restatement of csrc/kernels_attn_bwd.h (tools/attn_bwd_emul.py)
against fp64 autograd of the torch chains, on every case the device test runs (tests/attn_train_cases.py).

In fp64 the two agree to 1e-10 per tensor: the derivation, both LayerNorm skips (T = 1, B = 1), the exact zeros of w_qs / w_ks at
B = 1 and of the pooling's v.bias.  In fp32 the restatement -- the kernels' order of operations: scores recomputed from x and q',
weights from the saved statistics, D, g_S = A (g_A - D), the two reductions -- stays under the project's bar for the gradients of a
native fp32 kernel (hmrnn_cases.BAR, 2e-5); the per-case value is printed."""
import numpy as np
import pytest

import attn_train_cases as cases
import attn_bwd_emul as em

BLOCK = list(cases.block_cases())
POOL = list(cases.pool_cases())


def _params(mod):
    return [p.detach().numpy() for p in mod.parameters()]


@pytest.mark.parametrize('case', BLOCK, ids=[c[0] for c in BLOCK])
def test_block_emulation_fp64_is_autograd_and_fp32_is_under_the_bar(case):
    name, enc, x, gw = case
    ref = cases.reference(name, enc, x, gw)
    T, B, _ = x.shape
    assert len(ref) == 14 and ref[0].shape == x.shape
    assert (ref[4] is None) == (T == 1) and (ref[12] is None) == (B == 1)          # a skipped LayerNorm has no gradient
    if B == 1:
        assert not ref[1].any() and not ref[2].any()                                 # A == 1: the scores carry no gradient
    e64 = em.errors(em.block_gradients(_params(enc), x, gw, np.float64), ref)
    e32 = em.errors(em.block_gradients(_params(enc), x, gw, np.float32), ref)
    print(f'block {name}: fp64 emulation {max(e64):.3g}, fp32 emulation {max(e32):.3g} ({cases.BLOCK_NAMES[int(np.argmax(e32))]})')
    for n, v in zip(cases.BLOCK_NAMES, e64):
        assert v <= 1e-10, (n, v)
    for n, v in zip(cases.BLOCK_NAMES, e32):
        assert v <= cases.BAR, (n, v)


def test_the_overflow_case_has_scores_beyond_88():
    dims, T, B, fill, k = cases.OVERFLOW
    _, enc, x, _ = cases.block_case(dims, T, B, fill, k)
    assert cases.max_score(enc, x) > 88


def test_forward_of_the_emulation_is_the_torch_chain():
    import torch
    name, enc, x, gw = cases.block_case('small', 17, 2, 'wide')
    _, y = em.block_forward_tape(_params(enc), x, np.float64)
    import copy
    with torch.no_grad():
        want = copy.deepcopy(enc).double()(torch.from_numpy(x).double()).numpy()
    assert np.max(np.abs(y - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))


@pytest.mark.parametrize('case', POOL, ids=[c[0] for c in POOL])
def test_pooling_emulation_fp64_is_autograd_and_fp32_is_under_the_bar(case):
    name, pool, y, gw = case
    ref = cases.reference(name, pool, y, gw)
    assert len(ref) == 5
    e64 = em.errors(em.pool_gradients(_params(pool), y, gw, np.float64), ref)
    e32 = em.errors(em.pool_gradients(_params(pool), y, gw, np.float32), ref)
    print(f'pooling {name}: fp64 emulation {max(e64):.3g}, fp32 emulation {max(e32):.3g} ({cases.POOL_NAMES[int(np.argmax(e32))]})')
    for n, v in zip(cases.POOL_NAMES, e64):
        assert v <= 1e-10, (n, v)
    for n, v in zip(cases.POOL_NAMES, e32):
        assert v <= cases.BAR, (n, v)


def test_need_leaves_out_what_is_not_wanted():
    name, enc, x, gw = cases.block_case('small', 17, 2, 'wide')
    full = em.block_gradients(_params(enc), x, gw, np.float64)
    assert em.block_gradients(_params(enc), x, gw, np.float64, need=[False] * 13)[1:] == [None] * 13
    for k in (0, 1, 3, 5, 9, 11, 12):
        need = [i == k for i in range(13)]
        got = em.block_gradients(_params(enc), x, gw, np.float64, need=need)[1:]
        assert [g is not None for g in got] == need and np.array_equal(got[k], full[1 + k])


def test_the_wide_batch_route_of_the_parameter_gemms():
    """B >= 64: attn_param_grads runs its row GEMMs per time step; the same gradients."""
    import torch
    from features.classifier import _TransformerEncoder
    from test_gpu_attn import DIMS, _fill, _input
    d, di, dk, dv = DIMS['small']
    enc = _fill(_TransformerEncoder(d, di, 1, dk, dv).eval(), 11, 'wide')
    x = _input(3, 64, d, 1)
    gw = np.random.default_rng(2).standard_normal(x.shape).astype(np.float32)
    ref = em.autograd_reference(enc, x, gw)
    for n, v in zip(cases.BLOCK_NAMES, em.errors(em.block_gradients(_params(enc), x, gw, np.float64), ref)):
        assert v <= 1e-10, (n, v)
