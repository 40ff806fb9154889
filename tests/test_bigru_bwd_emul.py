"""CPU: the math of the native bidirectional GRU backward pass (csrc/kernels_bigru_bwd.h, features/classifier.py::gru_param_grads)
as tools/bigru_bwd_emul.py restates it -- the kernel's step order and masking, both directions -- against autograd over
``_DynEnc._run_torch`` in fp64 (tests/test_bigru_golden.py pins that route to the real layers.DynamicEncoder); and the argument
checks of the training entry points that need no device."""
import ctypes as C
import importlib.util
import os

import pytest

from conftest import ROOT

BAR = 1e-12           # fp64 against fp64: rounding only (the HM-LSTM's equivalent reached 6e-16)
CASES = [(13, 20, 3, 5, 9), (36, 132, 1, 3, 4)]          # (input, hidden, layers, B, T)


@pytest.fixture(scope='module')
def emul():
    spec = importlib.util.spec_from_file_location('_bigru_bwd_emul', os.path.join(ROOT, 'tools', 'bigru_bwd_emul.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _names(L):
    return ['x'] + [f'{n}_l{l}{sfx}' for l in range(L) for sfx in ('', '_reverse') for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


@pytest.mark.parametrize('which', ['g_y', 'g_hn', 'both'])
@pytest.mark.parametrize('I,H,L,B,T,with_drop', [c + (d,) for c in CASES for d in (False, True) if c[2] > 1 or not d])   # one layer has no inter-layer dropout
def test_emulated_backward_equals_fp64_autograd(emul, I, H, L, B, T, with_drop, which):
    import torch
    params, x, lens, g_y, g_hn, drop = emul.random_case(20260930 + B, I, H, L, B, T)
    assert int(lens.min()) == 1 and int(lens.max()) == T            # ragged, with a column of one step and a full one
    gy, gh = (g_y if which != 'g_hn' else None), (g_hn if which != 'g_y' else None)
    d = drop if with_drop else None
    got = emul.gradients(params, x, lens, gy, gh, d)
    ref = emul.autograd_reference(params, x, lens, gy, gh, d)
    worst = 0.0
    for name, a, b in zip(_names(L), got, ref):
        err = float((a - b).abs().max() / b.abs().max())
        worst = max(worst, err)
        assert err <= BAR, (name, err)
    print(f'{I} -> {H} x {L} B {B} T {T} {which} drop {with_drop}: worst relative deviation from autograd {worst:.3g}')
    # the forward the emulation keeps its tape from is the route's own
    _, y, hn = emul.forward_tape(params, x, lens, d)
    y_ref, hn_ref, _ = emul.reference_forward(params, x, lens, d)
    assert float((y - y_ref).abs().max()) <= BAR and float((hn - hn_ref).abs().max()) <= BAR
    # a row behind a column's end holds exact zeros, and so does its gradient
    tapes, _, _ = emul.forward_tape(params, x, lens, d)
    da = emul.backward_layer(params[8 * (L - 1):], lens, tapes[-1], gy, None if gh is None else gh[2 * (L - 1):], top=True)
    for b in range(B):
        assert not da[int(lens[b]):, b].any() and not tapes[-1]['out'][int(lens[b]):, b].any()
    assert torch.isfinite(da).all()


def test_need_list_leaves_out_what_is_not_wanted(emul):
    from features.classifier import gru_param_grads
    params, x, lens, g_y, g_hn, _ = emul.random_case(3, 13, 20, 1, 4, 5)
    tapes, _, _ = emul.forward_tape(params, x, lens)
    da = emul.backward_layer(params, lens, tapes[0], g_y, g_hn, top=True)
    full = gru_param_grads(params, x, tapes[0]['out'], da)
    need = [False, True, False, False, True, False, True, False, False]
    part = gru_param_grads(params, x, tapes[0]['out'], da, need=need)
    for k, (p, f) in enumerate(zip(part, full)):
        assert (p is None) == (not need[k]) and (p is None or (p == f).all())


def test_training_entry_points_reject_bad_arguments_without_a_device():
    """DSP_EINVAL before any device call: sizes, NULL / misaligned / short tape, no gradient, missing output, no handle."""
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load()
    p = 4096                                 # a non-NULL, aligned value where a pointer is only checked, never followed
    big = 1 << 40
    n = nat.c_i64(0)
    assert lib.dsp_bigru_tape_bytes(None, 4, 4, C.byref(n)) == nat.EINVAL and b'NULL' in lib.dsp_last_error()
    assert lib.dsp_bigru_tape_bytes(p, 4, 4, None) == nat.EINVAL
    assert lib.dsp_bigru_tape_rows(None, 0, 4, 4, C.byref(n)) == nat.EINVAL and b'NULL' in lib.dsp_last_error()

    def fwd(T=4, B=4, x=p, drop=None, tape=p, nbytes=big, handle=None):
        return lib.dsp_bigru_forward_train(handle, x, T, B, None, drop, p, p, tape, nbytes, None)

    def bwd(T=4, B=4, tape=p, nbytes=big, g=p, g_hn=p, da=p, handle=None):
        return lib.dsp_bigru_backward(handle, 0, T, B, None, tape, nbytes, g, g_hn, da, None)

    cases = [(lambda: fwd(T=0), b'T 0'), (lambda: fwd(B=0), b'B 0'), (lambda: fwd(tape=None), b'NULL tape'),
             (lambda: fwd(tape=p + 4), b'aligned'), (lambda: fwd(nbytes=100), b'short'), (lambda: fwd(x=None), b'NULL input'),
             (lambda: fwd(), b'NULL handle'),
             (lambda: bwd(T=0), b'T 0'), (lambda: bwd(B=-1), b'B -1'), (lambda: bwd(tape=None), b'NULL tape'),
             (lambda: bwd(tape=p + 8), b'aligned'), (lambda: bwd(nbytes=0), b'short'), (lambda: bwd(g=None, g_hn=None), b'no gradient'),
             (lambda: bwd(da=None), b'NULL output'), (lambda: bwd(g=p + 2), b'aligned'), (lambda: bwd(da=p + 1), b'aligned'),
             (lambda: bwd(), b'NULL handle')]
    for call, what in cases:
        rc = call()
        assert rc == nat.EINVAL and what in lib.dsp_last_error(), (rc, what, lib.dsp_last_error())
    assert lib.dsp_abi_version() == 2
