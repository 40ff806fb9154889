"""CPU: the math of the native HM-LSTM backward pass (csrc/kernels_hmlstm_bwd.h, features/classifier.py::hm_param_grads) as
tools/hmlstm_bwd_emul.py restates it, against autograd of the fp64 step loop; and the argument checks of the training entry
points that need no device."""
import ctypes as C
import importlib.util
import os

import pytest

from conftest import ROOT

BAR = 1e-10           # fp64 against fp64: two orders of summation of at most a few thousand terms


@pytest.fixture(scope='module')
def emul():
    spec = importlib.util.spec_from_file_location('_hmlstm_bwd_emul', os.path.join(ROOT, 'tools', 'hmlstm_bwd_emul.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('ragged,with_state', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('I,sizes,B,T', [(24, (20, 28), 5, 9), (36, (256, 132), 3, 4)])
def test_emulated_backward_equals_fp64_autograd(emul, I, sizes, B, T, ragged, with_state):
    params, x, lens, state, gs = emul.random_case(20260900 + B, I, sizes, B, T, ragged=ragged, with_state=with_state)
    tape = emul.forward_tape(params, 1.0, x, state)
    for c in ('c1', 'c2'):                  # the case exercises what it is meant to: both boundary values, both sides of the clamp
        assert 0 < float(tape['z' + c[1]].mean()) < 1 or T * B < 20, c
    got = emul.gradients(params, 1.0, x, lens, state, *gs)
    ref = emul.autograd_reference(params, 1.0, x, lens, state, *gs)
    for name, a, b in zip(('x', 'c1.U_11', 'c1.U_21', 'c1.W_01', 'c1.bias', 'c2.U_11', 'c2.W_01', 'c2.bias'), got, ref):
        err = float((a - b).abs().max() / b.abs().max())
        assert err <= BAR, (name, err)


@pytest.mark.parametrize('which', [0, 1, 2])
def test_each_loss_gradient_alone(emul, which):
    """g_h1, g_h2 and g_last one at a time (the others None): the parts add up to the combined call (linearity)."""
    params, x, lens, state, gs = emul.random_case(20260901, 24, (20, 28), 4, 6)
    only = [g if k == which else None for k, g in enumerate(gs)]
    got = emul.gradients(params, 1.0, x, lens, state, *only)
    ref = emul.autograd_reference(params, 1.0, x, lens, state, *only)
    assert emul.worst_relative(got, ref) <= BAR


def test_slope_other_than_one(emul):
    params, x, lens, state, gs = emul.random_case(20260902, 24, (20, 28), 4, 6)
    assert emul.worst_relative(emul.gradients(params, 2.5, x, lens, state, *gs),
                               emul.autograd_reference(params, 2.5, x, lens, state, *gs)) <= BAR


def test_training_entry_points_reject_bad_arguments_without_a_device():
    """DSP_EINVAL before any device call: sizes, NULL / misaligned / short tape, no gradient, missing outputs, no handle."""
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load()
    p = 4096                                 # a non-NULL, aligned value where a pointer is only checked, never followed
    big = 1 << 40
    n = nat.c_i64(0)
    assert lib.dsp_hmlstm_tape_bytes(None, 4, 4, C.byref(n)) == nat.EINVAL
    assert lib.dsp_hmlstm_tape_bytes(p, 4, 4, None) == nat.EINVAL

    def fwd(T=4, B=4, a=1.0, x=p, h1=p, h2=p, z1=p, z2=p, tape=p, nbytes=big, handle=None):
        return lib.dsp_hmlstm_forward_train(handle, x, T, B, a, None, None, None, h1, h2, z1, z2, None, None, tape, nbytes, None)

    def bwd(T=4, B=4, a=1.0, tape=p, nbytes=big, h1=p, g=(p, p, p), dfs=(p, p), handle=None):
        return lib.dsp_hmlstm_backward(handle, T, B, a, None, None, tape, nbytes, h1, p, p, p, *g, *dfs, None)

    cases = [(lambda: fwd(T=0), b'T 0'), (lambda: fwd(B=0), b'B 0'), (lambda: fwd(tape=None), b'NULL tape'),
             (lambda: fwd(tape=p + 4), b'aligned'), (lambda: fwd(nbytes=100), b'short'), (lambda: fwd(h1=None), b'mandatory'),
             (lambda: fwd(z2=None), b'mandatory'), (lambda: fwd(x=None), b'NULL'), (lambda: fwd(), b'NULL handle'),
             (lambda: bwd(T=0), b'T 0'), (lambda: bwd(B=-1), b'B -1'), (lambda: bwd(tape=None), b'NULL tape'),
             (lambda: bwd(nbytes=0), b'short'), (lambda: bwd(g=(None, None, None)), b'no gradient'),
             (lambda: bwd(dfs=(p, None)), b'NULL output'), (lambda: bwd(h1=None), b'NULL forward output'),
             (lambda: bwd(a=float('inf')), b'not finite'), (lambda: bwd(), b'NULL handle')]
    for call, what in cases:
        rc = call()
        assert rc == nat.EINVAL and what in lib.dsp_last_error(), (rc, what, lib.dsp_last_error())
    assert lib.dsp_abi_version() == 2
