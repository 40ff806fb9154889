"""The device-resident Adam without a device: the fp64 restatement of tests/adam_cases.py -- the yardstick of
tests/test_gpu_adam.py -- against ``torch.optim.Adam`` (fp64, CPU, ``foreach=False``), the chunk-table builder (every element of
every tensor in exactly one chunk), the surface of the ``dsp_adam_*`` entry points, their argument checks (every one returns
before a device call) and the refusals of ``features.optim.DeviceAdam`` that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adam_cases as ac
from conftest import ROOT

NEW = ['dsp_adam_chunk_elems', 'dsp_adam_chunk_table', 'dsp_adam_create', 'dsp_adam_destroy', 'dsp_adam_bind_grads',
       'dsp_adam_set_hyper', 'dsp_adam_set_step', 'dsp_adam_get_state', 'dsp_adam_step']


def _lib():
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return nat, nat.load()


def test_restatement_equals_torch_adam_in_fp64():
    """1e-14 relative over 6 steps: both sides are fp64 (eps 1.1e-16) and differ in the order of a few roundings per step
    (torch forms m by lerp and p by addcdiv)."""
    import torch
    lens = ac.lengths(1024)
    p0, grads = ac.make_case(lens)
    params = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in p0]
    opt = torch.optim.Adam(params, lr=ac.LR, betas=ac.BETAS, eps=ac.EPS, foreach=False)
    for row in grads:
        for p, g in zip(params, row):
            p.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
    p, m, v = ac.adam_ref(p0, grads)
    for i in range(len(lens)):
        st = opt.state[params[i]]
        assert float(st['step']) == ac.K_STEPS
        for got, want in ((p[i], params[i].detach().numpy()), (m[i], st['exp_avg'].numpy()), (v[i], st['exp_avg_sq'].numpy())):
            assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want)), i
    # ... and from a checkpoint at step 10 000 with one lr per step (what set_lr does between steps)
    m0, v0 = ac.make_moments(lens)
    lrs = [1e-3, 0.8e-3]
    params = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in p0]
    opt = torch.optim.Adam(params, lr=lrs[0], betas=ac.BETAS, eps=ac.EPS, foreach=False)
    for q, a, b in zip(params, m0, v0):
        opt.state[q] = {'step': torch.tensor(10000.0), 'exp_avg': torch.from_numpy(a.astype(np.float64)),
                        'exp_avg_sq': torch.from_numpy(b.astype(np.float64))}
    for lr, row in zip(lrs, grads):
        opt.param_groups[0]['lr'] = lr
        for q, g in zip(params, row):
            q.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
    p, m, v = ac.adam_ref(p0, grads[:2], lr=lrs, step0=10000, m0=m0, v0=v0)
    for i in range(len(lens)):
        assert np.max(np.abs(p[i] - params[i].detach().numpy())) <= 1e-14 * np.max(np.abs(p[i])), i


def _check_cover(nat, numel):
    chunk = nat.load().dsp_adam_chunk_elems()
    tensor, offset = ac.chunk_table(nat, numel)
    assert len(tensor) == sum((n + chunk - 1) // chunk for n in numel)
    assert (np.diff(tensor) >= 0).all() and (offset % chunk == 0).all()              # tensors in order, chunks aligned in their tensor
    for t, n in enumerate(numel):
        seen = np.zeros(n, dtype=np.int32)
        for off in offset[tensor == t]:
            assert 0 <= off < n
            seen[off:min(off + chunk, n)] += 1
        assert (seen == 1).all(), t
    assert set(tensor.tolist()) == set(range(len(numel)))


def test_chunk_table_covers_every_element_once():
    nat, lib = _lib()
    chunk = lib.dsp_adam_chunk_elems()
    assert chunk >= 4 and chunk % 4 == 0                      # a chunk of an aligned tensor starts 16-byte aligned
    _check_cover(nat, ac.lengths(chunk))
    _check_cover(nat, ac.lengths(chunk)[::-1])


@pytest.mark.parametrize('kind', ac.HEADS)
def test_chunk_table_of_the_heads_parameter_lists(kind):
    nat, _ = _lib()
    numel = ac.head_numels(kind)
    assert len(numel) >= 8 and min(numel) <= 20
    _check_cover(nat, numel)


def test_entry_points_are_declared_bound_and_exported():
    nat, lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    for name in NEW:
        assert name in nat.SIGNATURES and hasattr(lib, name)
        decl = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        n_args = 0 if decl.strip() == 'void' else len(decl.split(','))
        assert n_args == len(nat.SIGNATURES[name][1]), name                            # one ctypes type per C parameter
    mk = open(os.path.join(ROOT, 'dsp-speech-recognition_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bdsp_optim\.hip\b', mk, re.M) and 'asan-optim' in mk
    import features
    from features.optim import DeviceAdam
    assert features.DeviceAdam is DeviceAdam


def test_argument_errors_come_before_any_device_call():
    """No GPU here: a call that got past its checks would fail differently (or fault).  Every one is DSP_EINVAL with a message."""
    nat, lib = _lib()
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    numel = (C.c_int64 * 2)(5, 3)

    def ptrs(*offs):
        return (C.c_void_p * len(offs))(*[None if o is None else base + 4 * o for o in offs])

    def einval(rc, what):
        assert rc == nat.EINVAL and what in lib.dsp_last_error().decode(), (rc, lib.dsp_last_error())
    h = C.c_void_p(0)
    P, M, V = ptrs(0, 8), ptrs(16, 24), ptrs(32, 40)
    good = [2, numel, P, M, V, 1e-3, 0.9, 0.999, 1e-8, C.byref(h)]

    def create(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.dsp_adam_create(*a)
    for k in (1, 2, 3, 4, 9):
        einval(create(**{f'a{k}': None}), 'NULL argument')
    einval(create(a0=0), 'n 0 must be >= 1')
    einval(create(a0=-2), 'n -2 must be >= 1')
    einval(create(a1=(C.c_int64 * 2)(5, 0)), 'numel[1] 0 must be in')
    einval(create(a1=(C.c_int64 * 2)(-1, 3)), 'numel[0] -1 must be in')
    einval(create(a5=float('nan')), 'lr is not finite')
    einval(create(a5=float('inf')), 'lr is not finite')
    for bad in (-0.1, 1.0, 1.5, float('nan')):
        einval(create(a6=bad), 'beta1')
        einval(create(a7=bad), 'beta2')
    einval(create(a8=-1e-8), 'eps')
    einval(create(a8=float('nan')), 'eps')
    einval(create(a2=ptrs(0, None)), 'NULL pointer p[1]')
    einval(create(a3=ptrs(None, 24)), 'NULL pointer m[0]')
    einval(create(a4=ptrs(32, None)), 'NULL pointer v[1]')
    einval(create(a2=ptrs(0, 4)), 'p[0] and p[1] overlap')                             # 5 elements at 0 reach into 4
    einval(create(a3=ptrs(16, 2)), 'overlap')                                          # m[1] inside p[0]
    einval(create(a4=ptrs(20, 40)), 'm[0] and v[0] overlap')
    einval(create(a4=ptrs(32, 8)), 'overlap')                                          # v[1] is p[1]
    odd = (C.c_void_p * 2)(base + 2, base + 32)
    einval(create(a2=odd), 'p[0] is not 4-byte aligned')
    assert h.value is None
    # the other calls: NULL handles and values, then -- on a dry-run handle -- everything that passed its checks is refused
    einval(lib.dsp_adam_bind_grads(None, P, None), 'NULL argument')
    einval(lib.dsp_adam_set_hyper(None, 1e-3, 0.9, 0.999, 1e-8, None), 'NULL argument')
    einval(lib.dsp_adam_set_step(None, 0, None), 'NULL argument')
    einval(lib.dsp_adam_get_state(None, None, None, None), 'NULL argument')
    einval(lib.dsp_adam_step(None, 0, None), 'NULL argument')
    assert lib.dsp_adam_destroy(None) == nat.OK
    nc = C.c_int64(0)
    einval(lib.dsp_adam_chunk_table(2, None, 0, None, None, C.byref(nc)), 'NULL argument')
    einval(lib.dsp_adam_chunk_table(2, numel, 0, None, None, None), 'NULL argument')
    einval(lib.dsp_adam_chunk_table(0, numel, 0, None, None, C.byref(nc)), 'n 0 must be >= 1')
    einval(lib.dsp_adam_chunk_table(2, (C.c_int64 * 2)(4, -4), 0, None, None, C.byref(nc)), 'numel[1] -4 must be in')
    one = (C.c_int64 * 1)()
    einval(lib.dsp_adam_chunk_table(2, numel, 2, one, None, C.byref(nc)), 'NULL argument')
    einval(lib.dsp_adam_chunk_table(2, numel, 1, one, one, C.byref(nc)), 'capacity 1 is below the 2 chunks')
    assert lib.dsp_debug_host_dry_run(1) == nat.OK
    try:
        assert lib.dsp_adam_create(*good) == nat.OK and h.value
        refused = 'dsp_debug_host_dry_run: launches are refused'
        einval(lib.dsp_adam_step(h, 0, None), 'no gradients are bound')
        einval(lib.dsp_adam_bind_grads(h, None, None), 'NULL argument')
        einval(lib.dsp_adam_bind_grads(h, ptrs(48, None), None), 'NULL pointer g[1]')
        einval(lib.dsp_adam_bind_grads(h, ptrs(48, 50), None), 'g[0] and g[1] overlap')
        einval(lib.dsp_adam_bind_grads(h, ptrs(48, 42), None), 'overlap')              # g[1] reaches into v[1]
        einval(lib.dsp_adam_bind_grads(h, ptrs(48, 56), None), refused)
        einval(lib.dsp_adam_set_hyper(h, float('nan'), 0.9, 0.999, 1e-8, None), 'lr is not finite')
        einval(lib.dsp_adam_set_hyper(h, 1e-3, 1.0, 0.999, 1e-8, None), 'beta1')
        einval(lib.dsp_adam_set_hyper(h, 1e-3, 0.9, -0.5, 1e-8, None), 'beta2')
        einval(lib.dsp_adam_set_hyper(h, 1e-3, 0.9, 0.999, -1.0, None), 'eps')
        einval(lib.dsp_adam_set_hyper(h, 1e-3, 0.9, 0.999, 1e-8, None), refused)
        einval(lib.dsp_adam_set_step(h, -1, None), 'step -1 must be >= 0')
        einval(lib.dsp_adam_set_step(h, 7, None), refused)
        step, hyper = C.c_int64(0), (C.c_double * 4)()
        einval(lib.dsp_adam_get_state(h, None, hyper, None), 'NULL argument')
        einval(lib.dsp_adam_get_state(h, C.byref(step), hyper, None), refused)
        assert lib.dsp_adam_destroy(h) == nat.OK
    finally:
        lib.dsp_debug_host_dry_run(0)


def test_device_adam_refuses_what_it_does_not_serve():
    """Before anything touches a device: parameters that are not contiguous fp32 CUDA tensors, an empty list."""
    import torch
    from features.optim import DeviceAdam
    with pytest.raises(ValueError, match='no parameters'):
        DeviceAdam([])
    with pytest.raises(ValueError, match='contiguous float32 CUDA tensor'):
        DeviceAdam([torch.zeros(4)])
    with pytest.raises(ValueError, match='contiguous float32 CUDA tensor'):
        DeviceAdam([torch.zeros(4, dtype=torch.float64)])
    with pytest.raises(TypeError, match='not a tensor'):
        DeviceAdam([np.zeros(4, dtype=np.float32)])
    from features.train import TrainBatch
    import inspect
    assert inspect.signature(TrainBatch.capture).parameters['optimizer'].default is None
