"""The attention blocks' training entry points without a device (include/dsp_frontend.h: dsp_attn_tape_bytes,
dsp_attn_forward_train, dsp_attn_backward_bytes, dsp_attn_backward, dsp_selfattn_pool_train_batch,
dsp_selfattn_pool_backward_batch; features/classifier.py: _AttnTrain, _SelfAttnTrain, attn_param_grads): declared / exported /
bound, no byte count holds a B T T term, every argument check is DSP_EINVAL before any device call under dsp_debug_host_dry_run,
``native=True`` with a gradient required names both reasons on a CPU tensor, and the default route under grad is torch's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_attn_host import _einval, _host_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dsp_attn_tape_bytes', 'dsp_attn_forward_train', 'dsp_attn_backward_bytes', 'dsp_attn_backward',
       'dsp_selfattn_pool_train_batch', 'dsp_selfattn_pool_backward_batch']


@pytest.fixture(scope='module')
def nat():
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.fail(f'{nat.LIB_PATH} is not built')
    return nat


@pytest.fixture()
def dry(nat):
    """(lib, a dry-run handle of the shipped head's block); the handle is destroyed and dry run left afterwards."""
    lib = nat.load()
    nat.check(lib.dsp_debug_host_dry_run(1))
    h = nat.c_vp(0)
    try:
        desc, keep = _host_block(nat)
        nat.check(lib.dsp_attn_create(C.byref(desc), C.byref(h)))
        yield lib, h
    finally:
        if h.value:
            assert lib.dsp_attn_destroy(h) == nat.OK
        nat.check(lib.dsp_debug_host_dry_run(0))


def test_entry_points_declared_exported_and_bound(nat):
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    lib = nat.load()
    for name in NEW:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
        assert name in nat.SIGNATURES and hasattr(lib, name)
        decl = re.search(name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        assert len(decl.split(',')) == len(nat.SIGNATURES[name][1]), name              # one ctypes type per C parameter
    new_part = hdr[hdr.index('Training the encoder layer'):]
    for cite in ('transformer.py:41,56', 'transformer.py:112-121,134-139', 'layers.py:136-142', 'layers.py:139', 'layers.py:88-94'):
        assert cite in new_part, cite


def _sizes(nat, lib, h, T, B):
    tape, work, da = nat.c_i64(0), nat.c_i64(0), nat.c_i64(0)
    nat.check(lib.dsp_attn_tape_bytes(h, T, B, C.byref(tape)))
    nat.check(lib.dsp_attn_backward_bytes(h, T, B, C.byref(work), C.byref(da)))
    return tape.value, work.value, da.value


def test_tape_work_and_da_have_no_btt_term(nat, dry):
    lib, h = dry
    TP, DP, d, di, dk, dv = 208, 48, 39, 200, 100, 100
    small, big = _sizes(nat, lib, h, 200, 8), _sizes(nat, lib, h, 200, 512)
    # a B T'-linear term plus a T'^2 constant: f(B) = B row + const, exactly
    for (s, b), rows, const in zip(zip(small, big), (3 * TP * DP, 2 * TP * DP, 200 * (4 * d + di + dv + dk)), (2 * TP * TP, TP * TP, 0)):
        assert s == 4 * (8 * rows + const) and b == 4 * (512 * rows + const), (s, b, rows, const)
        assert b - s == 4 * (512 - 8) * rows
    one_btt = 4 * 512 * 200 * 200
    assert big[0] < one_btt and big[1] < one_btt              # tape and workspace: each below ONE [B, T, T] fp32 tensor
    assert big[2] == 4 * 200 * 512 * (4 * d + di + dv + dk)   # da: the rows of the parameter-gradient GEMMs, nothing else
    # linear in B beside the constant
    a, b, c = (_sizes(nat, lib, h, 200, B) for B in (512, 1024, 1536))
    assert all(z - y == y - x for x, y, z in zip(a, b, c))


def test_block_checks_return_before_any_launch(nat, dry):
    lib, h = dry
    nb, wb, db = nat.c_i64(0), nat.c_i64(0), nat.c_i64(0)
    tb = lambda T, B, handle=h, out=C.byref(nb): lib.dsp_attn_tape_bytes(handle, T, B, out)
    bb = lambda T, B, handle=h, w=C.byref(wb), a=C.byref(db): lib.dsp_attn_backward_bytes(handle, T, B, w, a)
    for f in (tb, bb):
        _einval(nat, f(5, 3, handle=None), 'NULL argument')
        _einval(nat, f(0, 3), 'T 0 must be in [1, 1024]')
        _einval(nat, f(1025, 3), 'T 1025 must be in [1, 1024]')
        _einval(nat, f(5, 0), 'B 0 must be >= 1')
        _einval(nat, f(1024, 2 ** 31 - 1), 'more than one launch holds')
    _einval(nat, tb(5, 3, out=None), 'NULL argument')
    _einval(nat, bb(5, 3, w=None), 'NULL argument')
    _einval(nat, bb(5, 3, a=None), 'NULL argument')
    nat.check(tb(5, 3))
    nat.check(bb(5, 3))
    # host memory stands in for the device buffers: no call below gets as far as a launch
    x, y, g, gx = (np.zeros((5, 3, 39), np.float32) for _ in range(4))
    al = lambda a: (a.ctypes.data + 15) & ~15
    tape, work, da = np.zeros(nb.value // 4 + 8, np.float32), np.zeros(wb.value // 4 + 8, np.float32), np.zeros(db.value // 4, np.float32)
    fwd = lambda hh=h, xx=x.ctypes.data, T=5, B=3, yy=y.ctypes.data, t=al(tape), n=nb.value: lib.dsp_attn_forward_train(hh, xx, T, B, yy, t, n, None)
    for k in ('hh', 'xx', 'yy'):
        _einval(nat, fwd(**{k: None}), 'NULL handle / input / output')
    _einval(nat, fwd(T=0), 'T 0 must be in [1, 1024]')
    _einval(nat, fwd(B=0), 'B 0 must be >= 1')
    _einval(nat, fwd(t=None), 'd_tape holds 0 bytes')
    _einval(nat, fwd(n=nb.value - 1), f'd_tape holds {nb.value - 1} bytes, {nb.value} are needed')
    _einval(nat, fwd(t=al(tape) + 4), 'd_tape must be 16-byte aligned')
    _einval(nat, fwd(), 'dry_run: launches are refused')
    bwd = lambda hh=h, T=5, B=3, t=al(tape), tn=nb.value, gg=g.ctypes.data, dx=gx.ctypes.data, a=da.ctypes.data, an=db.value, w=al(work), wn=wb.value: \
        lib.dsp_attn_backward(hh, T, B, t, tn, gg, dx, a, an, w, wn, None)
    _einval(nat, bwd(hh=None), 'NULL handle / gradient')
    _einval(nat, bwd(gg=None), 'NULL handle / gradient')
    _einval(nat, bwd(T=1025), 'T 1025 must be in [1, 1024]')
    _einval(nat, bwd(B=-1), 'B -1 must be >= 1')
    _einval(nat, bwd(t=None), 'd_tape holds 0 bytes')
    _einval(nat, bwd(tn=nb.value - 4), f'd_tape holds {nb.value - 4} bytes, {nb.value} are needed')
    _einval(nat, bwd(t=al(tape) + 8), 'd_tape must be 16-byte aligned')
    _einval(nat, bwd(w=None), 'd_work holds 0 bytes')
    _einval(nat, bwd(wn=wb.value - 1), f'd_work holds {wb.value - 1} bytes, {wb.value} are needed')
    _einval(nat, bwd(w=al(work) + 4), 'd_work must be 16-byte aligned')
    _einval(nat, bwd(a=None), 'd_da holds 0 bytes')
    _einval(nat, bwd(an=db.value - 1), f'd_da holds {db.value - 1} bytes, {db.value} are needed')
    _einval(nat, bwd(), 'dry_run: launches are refused')
    _einval(nat, bwd(dx=None), 'dry_run: launches are refused')                        # d_gx is optional
    # a tape of another (T, B) is too short for this one
    _einval(nat, bwd(T=6, B=30), 'are needed')


def test_d_model_one_is_refused_for_training(nat):
    lib = nat.load()
    nat.check(lib.dsp_debug_host_dry_run(1))
    h = nat.c_vp(0)
    try:
        desc, keep = _host_block(nat, 1, 4, 4, 4)
        nat.check(lib.dsp_attn_create(C.byref(desc), C.byref(h)))
        n = nat.c_i64(0)
        nat.check(lib.dsp_attn_workspace_bytes(h, 5, 3, C.byref(n)))                    # the forward still serves it
        what = 'd_model 1 must be in [2, 64] for training'
        _einval(nat, lib.dsp_attn_tape_bytes(h, 5, 3, C.byref(n)), what)
        _einval(nat, lib.dsp_attn_backward_bytes(h, 5, 3, C.byref(n), C.byref(n)), what)
        buf = np.zeros(64, np.float32)
        p = (buf.ctypes.data + 15) & ~15
        _einval(nat, lib.dsp_attn_forward_train(h, p, 5, 3, p, p, 1 << 20, None), what)
        _einval(nat, lib.dsp_attn_backward(h, 5, 3, p, 1 << 20, p, p, p, 1 << 20, p, 1 << 20, None), what)
    finally:
        if h.value:
            assert lib.dsp_attn_destroy(h) == nat.OK
        nat.check(lib.dsp_debug_host_dry_run(0))


def test_pooling_checks_return_before_any_launch(nat):
    lib = nat.load()
    nat.check(lib.dsp_debug_host_dry_run(1))
    try:
        H = 8
        al = lambda a: (a.ctypes.data + 15) & ~15
        y, W, go = np.zeros(4 * 2 * H + 8, np.float32), np.zeros(H * H + 8, np.float32), np.zeros(2 * H + 8, np.float32)
        vec = np.zeros(4 * 2 * H, np.float32)
        vp = vec.ctypes.data
        tr = lambda yy=al(y), T=4, B=2, HH=H, WW=al(W), bW=vp, v=vp, c=vp, o=vp, w=vp: \
            lib.dsp_selfattn_pool_train_batch(yy, T, B, HH, WW, bW, v, c, o, w, None)
        for k in ('yy', 'WW', 'bW', 'v', 'c', 'o', 'w'):
            _einval(nat, tr(**{k: None}), 'NULL argument')
        _einval(nat, tr(T=0), 'T 0 must be in [1, 1024]')
        _einval(nat, tr(B=0), 'B 0 must be >= 1')
        _einval(nat, tr(HH=6), 'H 6 must be a multiple of 4 in [4, 256]')
        _einval(nat, tr(yy=al(y) + 4), 'must be 16-byte aligned')
        _einval(nat, tr(), 'dry_run: launches are refused')
        bw = lambda yy=al(y), T=4, B=2, HH=H, WW=al(W), bW=vp, v=vp, w=vp, g=al(go), gy=vp, gp=vp, ge=vp, gv=vp: \
            lib.dsp_selfattn_pool_backward_batch(yy, T, B, HH, WW, bW, v, w, g, gy, gp, ge, gv, None)
        for k in ('yy', 'WW', 'bW', 'v', 'w', 'g', 'gp', 'ge', 'gv'):
            _einval(nat, bw(**{k: None}), 'NULL argument')
        _einval(nat, bw(T=0), 'T 0 must be in [1, 1024]')
        _einval(nat, bw(T=1025), 'T 1025 must be in [1, 1024]')
        _einval(nat, bw(B=0), 'B 0 must be >= 1')
        for bad in (0, 6, 260):
            _einval(nat, bw(HH=bad), f'H {bad} must be a multiple of 4 in [4, 256]')
        for k, p in (('yy', al(y) + 4), ('WW', al(W) + 8), ('g', al(go) + 4)):
            _einval(nat, bw(**{k: p}), 'must be 16-byte aligned')
        _einval(nat, bw(), 'dry_run: launches are refused')
        _einval(nat, bw(gy=None), 'dry_run: launches are refused')                      # d_gy is optional
    finally:
        nat.check(lib.dsp_debug_host_dry_run(0))


def test_native_true_with_a_gradient_required_names_both_reasons():
    import torch
    from features.classifier import _SelfAttn, _TransformerEncoder
    for mod, inp in ((_TransformerEncoder(39, 200, 1, 100, 100), torch.zeros(5, 3, 39)), (_SelfAttn(200), torch.zeros(4, 3, 200))):
        for m in (mod.train(), mod.eval()):                  # no mode-dependent behaviour: the same answer in both
            assert m.native_supported(inp, train=True) == 'the input is not on a GPU'
            assert 'a gradient is required' in m.native_supported(inp)                  # train=False: what it always said
            with pytest.raises(RuntimeError) as e:
                m(inp, native=True)
            assert 'a gradient is required' in str(e.value) and 'not on a GPU' in str(e.value)
            assert 'the native training path (a gradient is required) cannot run: ' in str(e.value)
    enc1 = _TransformerEncoder(1, 4, 1, 4, 4)
    assert enc1.native_supported(torch.zeros(5, 3, 1), train=True) is not None


def test_both_train_defaults_are_off_and_the_default_route_under_grad_is_torch(monkeypatch):
    import torch
    from features import classifier as Cl
    assert Cl._TransformerEncoder.native_train_default is False and Cl._SelfAttn.native_train_default is False

    def boom(*a, **k):
        raise AssertionError('the native path was asked for')
    for cls in (Cl._TransformerEncoder, Cl._SelfAttn):
        for name in ('_run_native', '_run_native_train', 'native_supported'):
            monkeypatch.setattr(cls, name, boom)
    rng = np.random.default_rng(0)
    inp = torch.from_numpy(rng.standard_normal((12, 3, 39)).astype(np.float32))
    lens = [12, 7, 3]
    torch.manual_seed(0)
    for head in (Cl.TransformerHead().eval(), Cl.HRNNAttHead().eval()):      # (eval: no GRU dropout between the two calls)
        a = head(inp, lens, dropout=False)
        b = head(inp, lens, dropout=False, native_attn=None)
        assert a[0].requires_grad and torch.equal(a[0], b[0])
        a[0].sum().backward()
        assert all(p.grad is not None for p in head.parameters())
    # an instance-level default asks (and, here, is told by the stub)
    enc = Cl._TransformerEncoder(39, 200, 1, 100, 100)
    enc.native_train_default = True
    with pytest.raises(AssertionError, match='the native path was asked for'):
        enc(inp)


def test_attn_param_grads_with_nothing_needed_returns_nones():
    import torch
    from features.classifier import attn_param_grads, _TransformerEncoder
    enc = _TransformerEncoder(6, 8, 1, 4, 12)
    T, B = 3, 2
    z = lambda n: torch.zeros(T, B, n)
    da = [z(n) for n in enc._da_widths()]
    assert [tuple(v.shape[2:]) for v in da] == [(6,), (8,), (6,), (6,), (12,), (6,), (4,)]
    res = attn_param_grads(enc._params(), z(6), z(6), z(6), da, need=[False] * 13)
    assert res == (None,) * 13
    full = attn_param_grads([p.detach() for p in enc._params()], z(6), z(6), z(6), da)
    assert [tuple(g.shape) for g in full] == [tuple(p.shape) for p in enc._params()]
