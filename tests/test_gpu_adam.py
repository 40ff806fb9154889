"""The device-resident Adam on the device (csrc/kernels_optim.h, csrc/dsp_optim.hip, features/optim.py) against the fp64
restatement of tests/adam_cases.py (which tests/test_adam_host.py holds against ``torch.optim.Adam`` in fp64):

  * K = 6 steps at lr = 1e-3 over the lengths of ``adam_cases.lengths`` (1 .. 3 C + 7 elements, every numel % 4, both sides of
    the chunk size C): m, v within 2e-5 max|ref|, p within K (2^-24 max|p0| + 2e-5 lr); torch's own fp32 Adam on the device is
    recorded beside it;
  * layouts, through the C ABI: all four arrays as views 1, 2, 3 floats off a 16-byte boundary, and only g off it -- the bits of
    the aligned run; sentinel words round every buffer intact; two runs equal; ``zero_grads`` leaves +0.0 and the same p, m, v;
  * the step count: a checkpoint at step 0 and at step 10 000, then one step (the bias corrections are not single precision);
  * a checkpoint into ``torch.optim.Adam`` and back; ``set_lr`` / ``device_state``; refusals;
  * the parameters' version counters: a head's next native forward repacks and equals a fresh handle's bits.
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import adam_cases as ac
from conftest import record

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PAD = 8                          # sentinel floats in front of and behind every view (32 bytes: the view at offset 0 is 16-byte aligned)
SENTINEL = 12345.0


def _dev():
    import torch
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def case():
    """The lengths, the inputs and the fp64 answer, computed once and left unchanged."""
    import types
    from features import _native as nat
    nat.require_device()
    chunk = nat.load().dsp_adam_chunk_elems()
    lens = ac.lengths(chunk)
    p0, grads = ac.make_case(lens)
    p, m, v = ac.adam_ref(p0, grads)
    return types.SimpleNamespace(lens=lens, p0=p0, grads=grads, p=p, m=m, v=v, chunk=chunk)


def _to_dev(arrays, dev):
    import torch
    return [torch.from_numpy(np.array(a, dtype=np.float32)).to(dev) for a in arrays]


def _host(tensors):
    return [t.detach().cpu().numpy() for t in tensors]


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _device_adam_run(case, dev, zero_grads=False):
    from features.optim import DeviceAdam
    params = _to_dev(case.p0, dev)
    opt = DeviceAdam(params, lr=ac.LR, betas=ac.BETAS, eps=ac.EPS)
    for row in case.grads:
        grads = _to_dev(row, dev)
        for p, g in zip(params, grads):
            p.grad = g
        opt.step(zero_grads=zero_grads)
    return opt, params, grads


class _Raw:
    """The C ABI on views into sentinel-filled buffers: ``offs`` = the offsets in floats of (p, g, m, v) from a 16-byte boundary."""

    def __init__(self, case, dev, offs):
        import torch
        from features import _native as nat
        self.nat, self.lib, self.case, self.dev = nat, nat.load(), case, dev
        self.bufs, self.views = [], {k: [] for k in 'pgmv'}
        for k, off in zip('pgmv', offs):
            for n in case.lens:
                buf = torch.full((n + 2 * PAD + 4,), SENTINEL, dtype=torch.float32, device=dev)
                assert buf.data_ptr() % 16 == 0
                view = buf[PAD + off:PAD + off + n]
                assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
                self.bufs.append((buf, PAD + off, n))
                self.views[k].append(view)
        for view, a in zip(self.views['p'], case.p0):
            view.copy_(torch.from_numpy(a))
        for k in 'mv':
            for view in self.views[k]:
                view.zero_()
        torch.cuda.synchronize(dev)
        n = len(case.lens)
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        h = C.c_void_p(0)
        nat.check(self.lib.dsp_adam_create(n, (C.c_int64 * n)(*case.lens), arr(self.views['p']), arr(self.views['m']), arr(self.views['v']),
                                           ac.LR, ac.BETAS[0], ac.BETAS[1], ac.EPS, C.byref(h)))
        self.h = h
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        nat.check(self.lib.dsp_adam_bind_grads(h, arr(self.views['g']), self.stream))

    def run(self, zero):
        import torch
        for row in self.case.grads:
            for view, g in zip(self.views['g'], row):
                view.copy_(torch.from_numpy(g))
            self.nat.check(self.lib.dsp_adam_step(self.h, 1 if zero else 0, self.stream))
        torch.cuda.synchronize(self.dev)
        step, hyper = C.c_int64(0), (C.c_double * 4)()
        self.nat.check(self.lib.dsp_adam_get_state(self.h, C.byref(step), hyper, self.stream))
        assert step.value == len(self.case.grads) and tuple(hyper) == (ac.LR,) + ac.BETAS + (ac.EPS,)
        for buf, lo, n in self.bufs:
            outside = torch.cat([buf[:lo], buf[lo + n:]])
            assert bool((outside == SENTINEL).all()), 'a sentinel word was written'
        out = {k: _host(self.views[k]) for k in 'pgmv'}
        self.nat.check(self.lib.dsp_adam_destroy(self.h))
        return out


def test_kernel_against_the_fp64_restatement(case):
    import torch
    dev = _dev()
    opt, params, _ = _device_adam_run(case, dev)
    torch.cuda.synchronize(dev)
    assert opt.device_state() == (ac.K_STEPS, ac.LR) + ac.BETAS + (ac.EPS,)
    bound = ac.p_bound(case.p0, ac.K_STEPS)
    # torch's own fp32 Adam on the device, on the same fp32 inputs: recorded, the bars are the project's
    t_params = [p.requires_grad_(True) for p in _to_dev(case.p0, dev)]
    t_opt = torch.optim.Adam(t_params, lr=ac.LR, betas=ac.BETAS, eps=ac.EPS)
    for row in case.grads:
        for p, g in zip(t_params, _to_dev(row, dev)):
            p.grad = g
        t_opt.step()
    torch.cuda.synchronize(dev)
    tm = [t_opt.state[p]['exp_avg'] for p in t_params]
    tv = [t_opt.state[p]['exp_avg_sq'] for p in t_params]
    figures = {
        'adam_native_m': ac.moment_err(_host(opt.exp_avg), case.m), 'adam_native_v': ac.moment_err(_host(opt.exp_avg_sq), case.v),
        'adam_native_p_over_bound': ac.p_err(_host(params), case.p) / bound,
        'adam_torch_fp32_m': ac.moment_err(_host(tm), case.m), 'adam_torch_fp32_v': ac.moment_err(_host(tv), case.v),
        'adam_torch_fp32_p_over_bound': ac.p_err(_host(t_params), case.p) / bound,
    }
    for k, val in figures.items():
        record(k, val)
    print(f'K = {ac.K_STEPS}, bound on p {bound:.3g}: ' + ', '.join(f'{k}={v:.3g}' for k, v in figures.items()))
    assert figures['adam_native_m'] <= ac.BAR and figures['adam_native_v'] <= ac.BAR
    assert figures['adam_native_p_over_bound'] <= 1.0
    # every tensor on its own as well: a wrong tail of a one-element tensor must not hide behind the largest one
    m_max, v_max = np.max(np.abs(ac.flat(case.m))), np.max(np.abs(ac.flat(case.v)))
    for i, n in enumerate(case.lens):
        assert ac.p_err([params[i].cpu().numpy()], [case.p[i]]) <= bound, n
        assert np.max(np.abs(opt.exp_avg[i].cpu().numpy() - case.m[i])) <= ac.BAR * m_max, n
        assert np.max(np.abs(opt.exp_avg_sq[i].cpu().numpy() - case.v[i])) <= ac.BAR * v_max, n


@pytest.fixture(scope='module')
def aligned(case):
    """The aligned run through the C ABI: what every other layout has to equal bit for bit."""
    return _Raw(case, _dev(), (0, 0, 0, 0)).run(False)


def test_aligned_run_twice_and_through_the_module_gives_the_same_bits(case, aligned):
    import torch
    again = _Raw(case, _dev(), (0, 0, 0, 0)).run(False)
    for k in 'pmv':
        assert _bits_equal(again[k], aligned[k]), k
    opt, params, _ = _device_adam_run(case, _dev())
    torch.cuda.synchronize(_dev())
    assert _bits_equal(_host(params), aligned['p']) and _bits_equal(_host(opt.exp_avg), aligned['m'])
    assert _bits_equal(_host(opt.exp_avg_sq), aligned['v'])
    assert _bits_equal(aligned['g'], case.grads[-1])                                   # without zero_grads the gradients stay


@pytest.mark.parametrize('offs', [(1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 1, 0, 0), (3, 0, 2, 1)], ids=str)
def test_misaligned_views_give_the_aligned_bits(case, aligned, offs):
    got = _Raw(case, _dev(), offs).run(False)
    for k in 'pmv':
        assert _bits_equal(got[k], aligned[k]), (k, offs)


@pytest.mark.parametrize('offs', [(0, 0, 0, 0), (1, 1, 1, 1), (0, 3, 0, 0)], ids=str)
def test_zero_grads_leaves_plus_zero_and_the_same_update(case, aligned, offs):
    got = _Raw(case, _dev(), offs).run(True)
    for k in 'pmv':
        assert _bits_equal(got[k], aligned[k]), (k, offs)
    for g in got['g']:
        assert (g.view(np.int32) == 0).all()                                           # +0.0, every element


def test_zero_grads_through_the_module(case):
    import torch
    dev = _dev()
    opt, params, grads = _device_adam_run(case, dev, zero_grads=True)
    plain, plain_params, plain_grads = _device_adam_run(case, dev)
    torch.cuda.synchronize(dev)
    assert all(p.grad is g for p, g in zip(params, grads))
    assert all((g.cpu().numpy().view(np.int32) == 0).all() for g in grads)
    assert _bits_equal(_host(plain_grads), case.grads[-1])
    assert _bits_equal(_host(params), _host(plain_params)) and _bits_equal(_host(opt.exp_avg), _host(plain.exp_avg))
    opt.zero_grad()
    assert all(p.grad is None for p in params)


@pytest.mark.parametrize('step0', [0, 10000])
def test_one_step_from_a_loaded_step_count(case, step0):
    """sqrt(1 - 0.999^t) and 1 - 0.9^t formed in fp32 are off by up to 6e-5 relative at t = 1 (1 - 0.999f): above the bar."""
    import torch
    from features.optim import DeviceAdam
    dev = _dev()
    m0, v0 = ac.make_moments(case.lens)
    params = _to_dev(case.p0, dev)
    opt = DeviceAdam(params, lr=ac.LR, betas=ac.BETAS, eps=ac.EPS)
    group = torch.optim.Adam([torch.zeros(1)], lr=ac.LR, betas=ac.BETAS, eps=ac.EPS).state_dict()['param_groups'][0]
    group['params'] = list(range(len(params)))
    state = {i: {'step': torch.tensor(float(step0)), 'exp_avg': torch.from_numpy(a), 'exp_avg_sq': torch.from_numpy(b)}
             for i, (a, b) in enumerate(zip(m0, v0))}
    opt.load_state_dict({'state': state, 'param_groups': [group]})
    assert opt.device_state()[0] == step0
    for p, g in zip(params, _to_dev(case.grads[0], dev)):
        p.grad = g
    opt.step()
    torch.cuda.synchronize(dev)
    assert opt.device_state()[0] == step0 + 1
    p, m, v = ac.adam_ref(case.p0, case.grads[:1], step0=step0, m0=m0, v0=v0)
    bound = ac.p_bound(case.p0, 1)
    em, ev, ep = ac.moment_err(_host(opt.exp_avg), m), ac.moment_err(_host(opt.exp_avg_sq), v), ac.p_err(_host(params), p)
    record(f'adam_step{step0}_p_over_bound', ep / bound)
    print(f'step0 = {step0}: m {em:.3g}, v {ev:.3g}, p {ep:.3g} of {bound:.3g}')
    assert em <= ac.BAR and ev <= ac.BAR and ep <= bound
    for i in range(len(case.lens)):
        assert ac.p_err([params[i].cpu().numpy()], [p[i]]) <= bound, case.lens[i]


def test_checkpoints_move_between_the_two_optimisers(case):
    """Three steps with one optimiser, the fourth with both from the checkpoint, on equal gradients: the parameters agree within
    twice the one-step bound (each side is one fp32 step away from the same fp64 step)."""
    import torch
    from features.optim import DeviceAdam
    dev = _dev()
    bound = 2 * ac.p_bound(case.p0, 1)
    for direction in ('native_to_torch', 'torch_to_native'):
        first = [p.requires_grad_(True) for p in _to_dev(case.p0, dev)]
        a = DeviceAdam(first, lr=ac.LR) if direction == 'native_to_torch' else torch.optim.Adam(first, lr=ac.LR)
        for row in case.grads[:3]:
            for p, g in zip(first, _to_dev(row, dev)):
                p.grad = g
            a.step()
        second = [p.detach().clone().requires_grad_(True) for p in first]
        b = torch.optim.Adam(second, lr=0.5) if direction == 'native_to_torch' else DeviceAdam(second, lr=0.5)
        sd = a.state_dict()
        assert sorted(sd['state'][0]) == ['exp_avg', 'exp_avg_sq', 'step'] and float(sd['state'][0]['step']) == 3.0
        b.load_state_dict(sd)
        for params, opt in ((first, a), (second, b)):
            for p, g in zip(params, _to_dev(case.grads[3], dev)):
                p.grad = g
            opt.step()
        torch.cuda.synchronize(dev)
        native = a if direction == 'native_to_torch' else b
        assert native.device_state()[:2] == (4, ac.LR)                                 # the lr came with the checkpoint
        err = ac.p_err(_host(first), [x.astype(np.float64) for x in _host(second)])
        record(f'adam_checkpoint_{direction}_over_bound', err / bound)
        assert err <= bound, (direction, err, bound)
        assert not _bits_equal(_host(first), case.p0)


def test_set_lr_and_refusals(case):
    import torch
    from features.optim import DeviceAdam
    dev = _dev()
    params = _to_dev(case.p0[:3], dev)
    opt = DeviceAdam(params)
    assert opt.device_state() == (0, 1e-3, 0.9, 0.999, 1e-8)
    assert opt.state_dict()['state'] == {}                                             # torch's Adam before its first step
    opt.set_lr(0.8e-3)
    assert opt.lr == 0.8e-3 and opt.device_state()[1] == 0.8e-3
    with pytest.raises(ValueError, match='lr is not finite'):
        opt.set_lr(float('nan'))
    assert opt.lr == 0.8e-3
    with pytest.raises(RuntimeError, match='has no gradient'):
        opt.step()
    for p in params:
        p.grad = torch.zeros_like(p)
    params[1].grad = torch.zeros(3, 2, device=dev)[:, 0]
    with pytest.raises(ValueError, match='gradient of parameter 1'):
        opt.step()
    assert opt.device_state()[0] == 0
    with pytest.raises(ValueError, match='contiguous float32 CUDA tensor'):
        DeviceAdam([torch.zeros(4, 4, device=dev)[:, 1]])
    with pytest.raises(ValueError, match='appears twice'):
        DeviceAdam([params[0], params[0]])
    with pytest.raises(ValueError, match='steps differ'):
        sd = {'state': {i: {'step': torch.tensor(float(i)), 'exp_avg': torch.zeros_like(p), 'exp_avg_sq': torch.zeros_like(p)}
                        for i, p in enumerate(params)},
              'param_groups': [{'lr': 1e-3, 'betas': (0.9, 0.999), 'eps': 1e-8, 'params': [0, 1, 2]}]}
        opt.load_state_dict(sd)


def test_step_bumps_the_version_counters_a_heads_handles_watch():
    """After ``DeviceAdam.step()`` the head's next native forward repacks its handles in place (they are kept) and gives the bits
    of a copy of the head that builds fresh handles from the written parameters."""
    import torch
    from features import classifier as cl
    from features.optim import DeviceAdam
    dev = _dev()
    rg = np.load(os.path.join(HERE, 'golden', 'rnn_golden.npz'))
    inp = torch.from_numpy(rg['inp']).to(dev)
    len_d = torch.from_numpy(np.asarray(rg['len0']).astype(np.int32)).to(dev)
    torch.manual_seed(0)
    head = cl.HMRNNHead().train()
    cl.fill_parameters(head, 3)
    head = head.to(dev)
    run = lambda h: h(inp, len_d, device_len=True, device_grad=True, dropout=False)[0]
    params = list(head.parameters())
    opt = DeviceAdam(params, lr=1e-2)
    before = run(head)
    before.square().sum().backward()
    handles = [(m, m._handle) for m in head.modules() if isinstance(m, cl._NativeHandle)]
    assert handles and all(h is not None for _, h in handles)
    versions = [p._version for p in params]
    opt.step()
    assert all(p._version > v for p, v in zip(params, versions))
    assert all(m._param_key(dev.index) != m._handle_key for m, _ in handles)
    with torch.no_grad():
        after = run(head)
    assert all(m._handle == h and m._param_key(dev.index) == m._handle_key for m, h in handles)     # kept, repacked
    fresh = copy.deepcopy(head)
    assert all(m._handle is None for m in fresh.modules() if isinstance(m, cl._NativeHandle))
    with torch.no_grad():
        want = run(fresh)
    torch.cuda.synchronize(dev)
    assert torch.equal(after.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(after, before.detach())
