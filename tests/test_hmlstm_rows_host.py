"""The HM-LSTM training pair under a row bound, without a device (include/dsp_frontend.h: dsp_hmlstm_forward_train_rows,
dsp_hmlstm_backward_rows): the header declares both, features/_native.py binds them with one ctypes type per C parameter of
the right kind, the library exports them, their argument checks are the plain pair's and come before any device call, and
the stand-alone sanitized host program (``make asan-rnn``: its own main, no Python, no preloaded runtime) builds and exits
clean."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW = {'dsp_hmlstm_forward_train_rows': 'dsp_hmlstm_forward_train', 'dsp_hmlstm_backward_rows': 'dsp_hmlstm_backward'}
CSRC = os.path.join(ROOT, 'dsp-speech-recognition_amd', 'csrc')


def _lib():
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return nat, nat.load()


def _params(hdr, name):
    """The declaration of ``name`` in the header -> [(C type without the name, parameter name)]."""
    decl = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr)
    assert decl, f'{name} is not declared'
    out = []
    for p in decl.group(1).split(','):
        m = re.fullmatch(r'\s*(.*?)\s*(\w+)\s*', p, re.S)
        out.append((re.sub(r'\s+', ' ', m.group(1)), m.group(2)))
    return out


def _ctype(nat, ctype):
    if '*' in ctype:
        return nat.c_vp
    return {'int32_t': nat.c_i32, 'int64_t': nat.c_i64, 'float': nat.c_f32}[ctype]


def test_header_declares_and_native_binds_both_entry_points():
    nat, lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    for name, plain in NEW.items():
        ps, pp = _params(hdr, name), _params(hdr, plain)
        assert name in nat.SIGNATURES and hasattr(lib, name)
        res, args = nat.SIGNATURES[name]
        assert res is C.c_int and list(args) == [_ctype(nat, t) for t, _ in ps], name
        assert list(nat.SIGNATURES[plain][1]) == [_ctype(nat, t) for t, _ in pp], plain
        # the plain call's parameters with the word behind d_len
        k = [n for _, n in ps].index('d_rows')
        assert ps[k] == ('const int32_t*', 'd_rows') and ps[k - 1][1] == 'd_len'
        assert ps[:k] + ps[k + 1:] == pp, name
    flat = re.sub(r'\s*\n \*\s*', ' ', hdr)
    assert 'd_rows == NULL is the plain call, bit for bit' in flat and 'Both passes must be given the same word' in flat


def test_argument_checks_are_the_plain_pairs_and_need_no_device():
    """No GPU here: a call that got past its checks would fail differently (or fault).  Every one is DSP_EINVAL with a message,
    with d_rows NULL and with d_rows given (the host never follows it)."""
    nat, lib = _lib()
    buf = (C.c_float * 72)()
    p = (C.addressof(buf) + 15) & ~15                           # 16-byte aligned; only checked, never followed
    big = 1 << 40

    def einval(rc, what):
        assert rc == nat.EINVAL and what in lib.dsp_last_error().decode(), (rc, lib.dsp_last_error())
    for rows in (None, p):
        fwd = lambda **kw: lib.dsp_hmlstm_forward_train_rows(*[kw.get(k, v) for k, v in dict(
            h=None, x=p, T=4, B=4, a=1.0, len=None, rows=rows, sin=None, sout=p, h1=p, h2=p, z1=p, z2=p, zhat=p, last=p, tape=p,
            nbytes=big, stream=None).items()])
        bwd = lambda **kw: lib.dsp_hmlstm_backward_rows(*[kw.get(k, v) for k, v in dict(
            h=None, T=4, B=4, a=1.0, len=None, rows=rows, sin=None, tape=p, nbytes=big, h1=p, h2=p, z1=p, z2=p, g1=p, g2=p, gl=p,
            dfs1=p, dfs2=p, stream=None).items()])
        einval(fwd(T=0), 'T 0')
        einval(fwd(B=0), 'B 0')
        einval(fwd(tape=None), 'NULL tape')
        einval(fwd(tape=p + 4), 'aligned')
        einval(fwd(nbytes=100), 'short')
        einval(fwd(z2=None), 'mandatory')
        einval(fwd(x=None), 'NULL input')
        einval(fwd(), 'dsp_hmlstm_forward_train_rows: NULL handle')
        einval(bwd(T=0), 'T 0')
        einval(bwd(B=-1), 'B -1')
        einval(bwd(a=float('inf')), 'not finite')
        einval(bwd(tape=None), 'NULL tape')
        einval(bwd(nbytes=0), 'short')
        einval(bwd(z1=None), 'NULL forward output')
        einval(bwd(g1=None, g2=None, gl=None), 'no gradient')
        einval(bwd(dfs1=None), 'NULL output')
        einval(bwd(), 'dsp_hmlstm_backward_rows: NULL handle')


def test_asan_rnn_builds_and_exits_clean():
    """The stand-alone program behind ``make asan-rnn`` (tools/asan_rnn_args.cpp) holds the two NULL checks of each new entry
    point; it is built against the sanitized library and run as a program of its own."""
    src = open(os.path.join(ROOT, 'tools', 'asan_rnn_args.cpp')).read()
    for name in NEW:
        assert len(re.findall(r'EXPECT\(' + name + r'\(', src)) >= 2, name
    jobs = str(max(1, min(8, os.cpu_count() or 1)))
    r = subprocess.run(['make', '-C', CSRC, '-j', jobs, 'asan-rnn'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'asan_rnn_args: ok' in r.stdout, r.stdout[-4000:]
