"""The attention blocks without a device (include/dsp_frontend.h: dsp_attn_*, dsp_selfattn_pool_batch; features/classifier.py:
_TransformerEncoder, _SelfAttn): the entry points are declared / exported / bound, every size and NULL check is DSP_EINVAL with
its message and every launch is refused under dsp_debug_host_dry_run, the workspace holds no B T T term, ``native_supported``
names its reason, ``native=True`` raises it, and the default call path of both heads is the torch route."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dsp_attn_create', 'dsp_attn_destroy', 'dsp_attn_workspace_bytes', 'dsp_attn_forward', 'dsp_selfattn_pool_batch']
N_PARAMS = 13


@pytest.fixture(scope='module')
def nat():
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.fail(f'{nat.LIB_PATH} is not built')
    return nat


def _einval(nat, rc, what):
    msg = nat.load().dsp_last_error().decode()
    assert rc == nat.EINVAL and what in msg, (rc, msg, what)


def _host_block(nat, d=39, di=200, dk=100, dv=100, n_head=1, eps=1e-3):
    """A descriptor over exact-size HOST arrays (what create reads under dry run) and the arrays that keep them alive."""
    sizes = [d * dk, d * dk, d * dv, d, d, d * dv, d, di * d, di, d * di, d, d, d]
    rng = np.random.default_rng(3)
    arrs = [rng.uniform(-0.08, 0.08, n).astype(np.float32) for n in sizes]
    desc = nat.AttnDesc(d, di, n_head, dk, dv, eps)
    desc.d_params[:N_PARAMS] = [a.ctypes.data for a in arrs]
    return desc, arrs


def test_entry_points_declared_exported_and_bound(nat):
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    lib = nat.load()
    for name in NEW:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
        assert name in nat.SIGNATURES and hasattr(lib, name)
        decl = re.search(name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        assert len(decl.split(',')) == len(nat.SIGNATURES[name][1]), name              # one ctypes type per C parameter
    new_part = hdr[hdr.index('/* ---- the attention blocks'):]
    for cite in ('transformer.py:16-140', 'layers.py:125-143', 'transformer.py:41,56', 'layers.py:136', 'layers.py:78-95'):
        assert cite in new_part, cite
    assert int(re.search(r'#define DSP_ATTN_PARAMS (\d+)', hdr).group(1)) == N_PARAMS


def test_struct_layout_matches_the_header(nat):
    # dsp_attn_desc: 5 int32 | float | 16 pointers
    assert C.sizeof(nat.AttnDesc) == 24 + 16 * 8
    assert [getattr(nat.AttnDesc, f).offset for f, _ in nat.AttnDesc._fields_] == [0, 4, 8, 12, 16, 20, 24]
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    body = re.search(r'typedef struct dsp_attn_desc \{(.*?)\} dsp_attn_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'\b(\w+)\s*(?:\[\d+\])?\s*[,;]', body)
    assert names == [f for f, _ in nat.AttnDesc._fields_], names


def test_descriptor_follows_the_module_parameter_order():
    from features.classifier import _TransformerEncoder
    enc = _TransformerEncoder(39, 200, 1, 100, 100)
    names = [n for n, _ in enc.named_parameters()]
    assert names == ['slf_attn.w_qs', 'slf_attn.w_ks', 'slf_attn.w_vs', 'slf_attn.layer_norm.a_2', 'slf_attn.layer_norm.b_2',
                     'slf_attn.proj.weight', 'slf_attn.proj.bias', 'pos_ffn.w_1.weight', 'pos_ffn.w_1.bias', 'pos_ffn.w_2.weight',
                     'pos_ffn.w_2.bias', 'pos_ffn.layer_norm.a_2', 'pos_ffn.layer_norm.b_2']
    assert len(enc._params()) == N_PARAMS and all(a is b for a, b in zip(enc._params(), enc.parameters()))


def test_create_checks_and_dry_run_handles(nat):
    """No device here: a check that let a call through would come back as a HIP error, not DSP_EINVAL."""
    lib = nat.load()
    nat.check(lib.dsp_debug_host_dry_run(1))
    handles = []
    try:
        def create(desc):
            h = nat.c_vp(0)
            rc = lib.dsp_attn_create(C.byref(desc), C.byref(h))
            if rc == nat.OK:
                handles.append(h.value)
            return rc, h.value

        for dims in ((39, 200, 100, 100), (6, 8, 4, 12), (1, 4, 4, 4), (64, 256, 128, 128)):
            desc, keep = _host_block(nat, *dims)
            rc, h = create(desc)
            assert rc == nat.OK and h, (dims, lib.dsp_last_error())
        for kw, what in ((dict(n_head=2), 'n_head 2 must be 1'), (dict(n_head=0), 'n_head 0 must be 1'),
                         (dict(d=0), 'd_model 0 must be in [1, 64]'), (dict(d=65), 'd_model 65 must be in [1, 64]'),
                         (dict(dk=0), 'multiples of 4 in [4, 128]'), (dict(dk=102), 'multiples of 4 in [4, 128]'),
                         (dict(dk=132), 'multiples of 4 in [4, 128]'), (dict(dv=2), 'multiples of 4 in [4, 128]'),
                         (dict(dv=132), 'multiples of 4 in [4, 128]'), (dict(di=0), 'd_inner 0 must be a multiple of 4 in [4, 256]'),
                         (dict(di=202), 'd_inner 202 must be a multiple of 4 in [4, 256]'),
                         (dict(di=260), 'd_inner 260 must be a multiple of 4 in [4, 256]'),
                         (dict(eps=float('nan')), 'eps must be finite'), (dict(eps=-1.0), 'eps must be finite')):
            desc, keep = _host_block(nat, **{k: (max(v, 1) if k in ('d', 'dk', 'dv', 'di') else v) for k, v in kw.items()})
            for k, v in kw.items():
                setattr(desc, {'d': 'd_model', 'di': 'd_inner', 'dk': 'd_k', 'dv': 'd_v'}.get(k, k), v)
            _einval(nat, create(desc)[0], what)
        for i in range(N_PARAMS):
            desc, keep = _host_block(nat)
            desc.d_params[i] = None
            _einval(nat, create(desc)[0], f'NULL parameter tensor (index {i})')
        desc, keep = _host_block(nat)
        _einval(nat, lib.dsp_attn_create(None, C.byref(nat.c_vp(0))), 'NULL argument')
        _einval(nat, lib.dsp_attn_create(C.byref(desc), None), 'NULL argument')
        assert lib.dsp_attn_destroy(None) == nat.OK
    finally:
        for h in handles:
            assert lib.dsp_attn_destroy(h) == nat.OK
        nat.check(lib.dsp_debug_host_dry_run(0))


def test_forward_and_pooling_checks_return_before_any_launch(nat):
    lib = nat.load()
    nat.check(lib.dsp_debug_host_dry_run(1))
    h = nat.c_vp(0)
    try:
        desc, keep = _host_block(nat)
        nat.check(lib.dsp_attn_create(C.byref(desc), C.byref(h)))
        nb = nat.c_i64(0)
        ws = lambda T, B, handle=h, out=C.byref(nb): lib.dsp_attn_workspace_bytes(handle, T, B, out)
        _einval(nat, ws(5, 3, handle=None), 'NULL argument')
        _einval(nat, ws(5, 3, out=None), 'NULL argument')
        _einval(nat, ws(0, 3), 'T 0 must be in [1, 1024]')
        _einval(nat, ws(1025, 3), 'T 1025 must be in [1, 1024]')
        _einval(nat, ws(5, 0), 'B 0 must be >= 1')
        _einval(nat, ws(1024, 2 ** 31 - 1), 'more than one launch holds')
        nat.check(ws(5, 3))
        # host memory stands in for the device buffers: no call below gets as far as a launch
        x, y = np.zeros((5, 3, 39), np.float32), np.zeros((5, 3, 39), np.float32)
        work = np.zeros(nb.value // 4 + 8, np.float32)
        wp = (work.ctypes.data + 15) & ~15
        fwd = lambda hh=h, xx=x.ctypes.data, T=5, B=3, yy=y.ctypes.data, w=wp, n=nb.value: lib.dsp_attn_forward(hh, xx, T, B, yy, w, n, None)
        _einval(nat, fwd(hh=None), 'NULL handle / input / output')
        _einval(nat, fwd(xx=None), 'NULL handle / input / output')
        _einval(nat, fwd(yy=None), 'NULL handle / input / output')
        _einval(nat, fwd(T=0), 'T 0 must be in [1, 1024]')
        _einval(nat, fwd(T=1025), 'T 1025 must be in [1, 1024]')
        _einval(nat, fwd(B=0), 'B 0 must be >= 1')
        _einval(nat, fwd(w=None), 'the workspace holds 0 bytes')
        _einval(nat, fwd(n=nb.value - 1), f'the workspace holds {nb.value - 1} bytes, {nb.value} are needed')
        _einval(nat, fwd(w=wp + 4), 'd_work must be 16-byte aligned')
        _einval(nat, fwd(), 'dry_run: launches are refused')

        H = 8
        a = np.zeros(4 * 2 * H + 8, np.float32)
        W = np.zeros(H * H + 8, np.float32)
        ap, Wp = (a.ctypes.data + 15) & ~15, (W.ctypes.data + 15) & ~15
        vec = np.zeros(H, np.float32)
        out = np.zeros(2 * H, np.float32)
        vp = vec.ctypes.data
        pool = lambda yy=ap, T=4, B=2, HH=H, WW=Wp, bW=vp, v=vp, c=vp, o=out.ctypes.data: lib.dsp_selfattn_pool_batch(yy, T, B, HH, WW, bW, v, c, o, None)
        for k in ('yy', 'WW', 'bW', 'v', 'c', 'o'):
            _einval(nat, pool(**{k: None}), 'NULL argument')
        _einval(nat, pool(T=0), 'T 0 must be in [1, 1024]')
        _einval(nat, pool(T=1025), 'T 1025 must be in [1, 1024]')
        _einval(nat, pool(B=0), 'B 0 must be >= 1')
        for bad in (0, 6, 260):
            _einval(nat, pool(HH=bad), f'H {bad} must be a multiple of 4 in [4, 256]')
        _einval(nat, pool(yy=ap + 4), 'must be 16-byte aligned')
        _einval(nat, pool(WW=Wp + 8), 'must be 16-byte aligned')
        _einval(nat, pool(), 'dry_run: launches are refused')
    finally:
        if h.value:
            assert lib.dsp_attn_destroy(h) == nat.OK
        nat.check(lib.dsp_debug_host_dry_run(0))


def test_workspace_has_no_btt_term(nat):
    lib = nat.load()
    nat.check(lib.dsp_debug_host_dry_run(1))
    h = nat.c_vp(0)
    try:
        desc, keep = _host_block(nat)
        nat.check(lib.dsp_attn_create(C.byref(desc), C.byref(h)))
        nb = nat.c_i64(0)
        nat.check(lib.dsp_attn_workspace_bytes(h, 200, 512, C.byref(nb)))
        assert 0 < nb.value < 4 * 512 * 200 * 200
        assert nb.value <= 4 * (512 * 208 * (100 + 100) + 2 * 208 * 208)            # O(B T (d_k + d_v)) + O(T T)
        n1, n2 = nat.c_i64(0), nat.c_i64(0)
        nat.check(lib.dsp_attn_workspace_bytes(h, 200, 1024, C.byref(n1)))          # linear in B, beside the [T, T] statistics
        nat.check(lib.dsp_attn_workspace_bytes(h, 200, 1536, C.byref(n2)))
        assert n2.value - n1.value == n1.value - nb.value
    finally:
        if h.value:
            assert lib.dsp_attn_destroy(h) == nat.OK
        nat.check(lib.dsp_debug_host_dry_run(0))


def test_native_supported_names_its_reason_and_native_true_raises_it():
    import torch
    from features.classifier import _SelfAttn, _TransformerEncoder
    x = torch.zeros(5, 3, 39)
    enc = _TransformerEncoder(39, 200, 1, 100, 100).eval()
    pool = _SelfAttn(200).eval()
    y = torch.zeros(4, 3, 200)
    cases = []
    with torch.no_grad():
        cases.append((enc, x, 'the input is not on a GPU'))
        cases.append((pool, y, 'the input is not on a GPU'))
        cases.append((_TransformerEncoder(39, 200, 2, 100, 100).eval(), x, 'n_head is 2'))
        for mod, inp, why in cases:
            assert why in mod.native_supported(inp)
            with pytest.raises(RuntimeError, match='the native path cannot run: .*' + re.escape(why)):
                mod(inp, native=True)
    # a gradient is required: the native path is forward only
    for mod, inp in ((enc, x), (pool, y)):
        assert 'a gradient is required' in mod.native_supported(inp)
        with pytest.raises(RuntimeError, match='a gradient is required'):
            mod(inp, native=True)
        with torch.no_grad():
            assert 'a gradient is required' not in mod.native_supported(inp)
    why = 'input and parameters must be float32 on one device'
    with torch.no_grad():
        for mod, inp in ((enc.double(), x.double()), (pool.double(), y.double()), (enc, x.float())):     # the last: fp64 parameters only
            assert mod.native_supported(inp) == why
            with pytest.raises(RuntimeError, match='the native path cannot run: ' + why):
                mod(inp, native=True)


def test_default_call_path_of_both_heads_is_the_torch_route(monkeypatch):
    import torch
    from features import classifier as Cl
    assert Cl._TransformerEncoder.native_default is False and Cl._SelfAttn.native_default is False

    def boom(*a, **k):
        raise AssertionError('the native path was taken')
    monkeypatch.setattr(Cl._TransformerEncoder, '_run_native', boom)
    monkeypatch.setattr(Cl._SelfAttn, '_run_native', boom)
    monkeypatch.setattr(Cl._TransformerEncoder, 'native_supported', boom)        # the default does not even ask
    monkeypatch.setattr(Cl._SelfAttn, 'native_supported', boom)
    rng = np.random.default_rng(0)
    inp = torch.from_numpy(rng.standard_normal((12, 3, 39)).astype(np.float32))
    lens = [12, 7, 3]
    torch.manual_seed(0)
    th, ah = Cl.TransformerHead().eval(), Cl.HRNNAttHead().eval()
    with torch.no_grad():
        for head in (th, ah):
            a = head(inp, lens, dropout=False)
            b = head(inp, lens, dropout=False, native_attn=None)
            c = head(inp, lens, dropout=False, native_attn=False)
            for u, v, w in zip(a, b, c):
                assert torch.equal(u, v) and torch.equal(u, w)
        # the blocks themselves: the same values as the chains they restate
        enc = th.attn_enc
        assert torch.equal(enc(inp), enc.pos_ffn(enc.slf_attn(inp))) and torch.equal(enc.run(inp, native=False), enc(inp))
        y = torch.from_numpy(rng.standard_normal((4, 3, 200)).astype(np.float32))
        yt = y.transpose(0, 1)
        w = torch.softmax(ah.attn.v(torch.tanh(ah.attn.attn(yt))).squeeze(2), 1)
        assert torch.equal(ah.attn(y), torch.bmm(w.unsqueeze(1), yt).squeeze(1))
