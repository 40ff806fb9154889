"""The device-side fit of the pitch model without a device (features/svmfit.py; include/dsp_frontend.h:
dsp_robust_scale_fit_batch, dsp_var_all, dsp_svm_fit_workspace_bytes, dsp_svm_fit_batch):

  (a) the NumPy restatement of the kernels' rules (tools/svm_fit_emul.py) against scikit-learn's stored results
      (tests/golden/svmfit_golden.npz) on every case of tests/svmfit_cases.py: scale_ / center_ equal under ``==``, decisions
      within the stored ``d_ref``, feasibility and the KKT gap of a fresh gradient, rho by libsvm's rule, the counts;
  (b) the header declares the entry points, features/_native.py binds them, every refusal returns before a launch, the
      package imports nothing of scikit-learn, and the stand-alone sanitized program (``make asan-svmfit``: its own main, no
      Python, no preloaded runtime) builds and exits clean.

The conditions and their drift term: tests/svmfit_ref.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))

import svm_fit_emul as emul  # noqa: E402
from svmfit_cases import CASES, MAX_ITER, TOLS, case, key  # noqa: E402
from svmfit_ref import check_conditions  # noqa: E402

CSRC = os.path.join(ROOT, 'dsp-speech-recognition_amd', 'csrc')
NEW = ('dsp_robust_scale_fit_batch', 'dsp_var_all', 'dsp_svm_fit_workspace_bytes', 'dsp_svm_fit_batch')


@pytest.fixture(scope='module')
def sgold():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'svmfit_golden.npz')) as z:
        return {k: z[k] for k in z.files}


# ---- (a) the restatement against scikit-learn's stored numbers ---------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_restatement_reproduces_sklearn(sgold, name):
    X, y, Q, a = case(name)
    classes = sgold[f'{name}/classes']
    center, scale, st = emul.robust_scale_fit(X, None, a['with_centering'], a['quantile_range'])
    assert st == 0
    assert np.array_equal(scale, sgold[f'{name}/scale']), np.max(np.abs(scale - sgold[f'{name}/scale']))
    assert scale.tobytes() == sgold[f'{name}/scale'].tobytes()                     # expected in every bit
    if a['with_centering']:
        assert np.array_equal(center, sgold[f'{name}/center']) and center.tobytes() == sgold[f'{name}/center'].tobytes()
    Xs, Qs = emul.transform(X, scale, center), emul.transform(Q, scale, center)
    yrow = np.where(y == classes[1], 1, -1)
    for tol in TOLS:
        k = key(name, tol)
        gamma = float(sgold[f'{k}/gamma'])
        if a['gamma'] == 'scale':
            assert abs(1.0 / (X.shape[1] * Xs.var()) - gamma) <= 1e-12 * gamma
        elif a['gamma'] == 'auto':
            assert gamma == 1.0 / X.shape[1]
        r = emul.svm_fit(Xs, yrow, a['C'], gamma, tol=tol, max_iter=MAX_ITER)
        assert r['status'] == 0
        dec = emul.decision(Xs, r['coef'], r['rho'], gamma, Qs)
        d = float(np.max(np.abs(dec - sgold[f'{k}/decision'])))
        print(k, 'n_iter', r['n_iter'], 'n_sv', r['n_sv'], 'max |restatement - sklearn|', d, 'd_ref', float(sgold[f'{k}/d_ref']))
        assert d <= float(sgold[f'{k}/d_ref']) * (1 + 1e-9) + 1e-300
        near = np.abs(sgold[f'{k}/decision']) < 4 * tol
        assert (classes[(dec > 0).astype(int)] == sgold[f'{k}/predict'])[~near].all()
        check_conditions(Xs, yrow, r['coef'], r['rho'], r['n_iter'], r['n_sv'], r['n_bounded'], a['C'], gamma, tol)


def test_restatement_status_paths_and_masked_problem():
    X, y, _, a = case('pair01_c1')
    _, scale, _ = emul.robust_scale_fit(X)
    Xs = emul.transform(X, scale)
    yrow = np.where(y == 1, 1, -1)
    r3 = emul.svm_fit(Xs, yrow, 1.0, 0.15, max_iter=3)
    assert (r3['status'], r3['n_iter']) == (emul.MAX_ITER, 3)
    check_conditions(Xs, yrow, r3['coef'], r3['rho'], 3, r3['n_sv'], r3['n_bounded'], 1.0, 0.15, 1e-3, check_gap=False)
    assert emul.svm_fit(Xs, np.abs(yrow), 1.0, 0.15)['status'] == emul.ONE_CLASS
    bad = Xs.copy()
    bad[7, 2] = np.nan
    assert emul.svm_fit(bad, yrow, 1.0, 0.15)['status'] == emul.NONFINITE
    masked = yrow.copy()
    masked[::3] = 0
    masked[7] = 0
    rm = emul.svm_fit(bad, masked, 1.0, 0.15)                                     # the NaN row is outside the problem
    rc = emul.svm_fit(bad[masked != 0], masked[masked != 0], 1.0, 0.15)
    assert rm['status'] == 0 and rm['coef'][masked != 0].tobytes() == rc['coef'].tobytes() and rm['rho'] == rc['rho']
    assert emul.robust_scale_fit(bad)[2] == emul.NONFINITE and emul.robust_scale_fit(bad, np.arange(len(bad)) != 7)[2] == 0
    assert emul.robust_scale_fit(X, np.zeros(len(X)))[2] == 1


# ---- (b) the C surface --------------------------------------------------------------------------------------------------------
def _lib():
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return nat, nat.load()


def test_header_declares_and_native_binds_the_entry_points():
    nat, lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    kinds = {'int32_t': nat.c_i32, 'int64_t': nat.c_i64, 'double': nat.c_f64}
    for name in NEW:
        decl = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr)
        assert decl, name
        want = []
        for p in decl.group(1).split(','):
            ctype = re.sub(r'\s+', ' ', re.fullmatch(r'\s*(.*?)\s*(\w+)\s*', p, re.S).group(1))
            if name.endswith('_bytes') and ctype == 'int64_t*':
                want.append(C.POINTER(nat.c_i64))
            else:
                want.append(nat.c_vp if '*' in ctype else kinds[ctype])
        res, args = nat.SIGNATURES[name]
        assert res is C.c_int and list(args) == want and hasattr(lib, name), name
        assert decl.group(1).rstrip().endswith('void* stream') or name.endswith('_bytes')
    assert 'pitch_model.py:48' in hdr and 'pitch_model.py:49-50' in hdr
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bdsp_svmfit\.hip\b', mk, re.M) and 'asan-svmfit' in mk
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert f'{len(nat.SIGNATURES)} entry points' in readme


def test_every_refusal_returns_before_a_launch():
    """No GPU here: a call that got past its checks would fail differently (or fault).  Every one is DSP_EINVAL with a message."""
    nat, lib = _lib()
    buf = (C.c_double * 8192)()
    p = (C.addressof(buf) + 15) & ~15                           # 16-byte aligned; only checked, never followed
    at = lambda k: p + 8 * k

    def einval(rc, what):
        assert rc == nat.EINVAL and what in lib.dsp_last_error().decode(), (rc, lib.dsp_last_error())

    def scaler(**kw):
        d = dict(X=at(0), ld=5, n=100, F=5, valid=None, ld_valid=0, q_lo=25.0, q_hi=75.0, centering=0, scale=at(1000), center=None,
                 info=at(1100), stream=None)
        d.update(kw)
        return lib.dsp_robust_scale_fit_batch(*d.values())
    einval(scaler(X=None), 'NULL matrix d_X')
    einval(scaler(X=at(0) + 4), '8-byte aligned')
    einval(scaler(F=0), 'F 0')
    einval(scaler(F=17, ld=17), 'F 17')
    einval(scaler(n=0), 'n 0')
    einval(scaler(n=8193), 'n 8193')
    einval(scaler(ld=4), 'ld 4')
    einval(scaler(valid=at(2000), ld_valid=0), 'ld_valid 0')
    einval(scaler(q_lo=80.0), 'quantile pair')
    einval(scaler(q_hi=101.0), 'quantile pair')
    einval(scaler(q_lo=float('nan')), 'quantile pair')
    einval(scaler(scale=None), 'NULL output')
    einval(scaler(info=None), 'NULL output')
    einval(scaler(centering=1), 'NULL output d_center')
    einval(scaler(scale=at(10)), 'd_scale overlaps d_X')
    einval(scaler(valid=at(2000), ld_valid=9, info=at(2100)), 'd_info overlaps d_valid')
    einval(scaler(centering=1, center=at(1002)), 'd_scale overlaps d_center')

    def var(**kw):
        d = dict(X=at(0), ld=5, n=100, F=5, center=None, scale=None, mask=None, out=at(1000), stream=None)
        d.update(kw)
        return lib.dsp_var_all(*d.values())
    einval(var(X=None), 'NULL matrix d_X')
    einval(var(out=None), 'NULL output d_out')
    einval(var(n=0), 'n 0')
    einval(var(F=17, ld=17), 'F 17')
    einval(var(out=at(499)), 'd_out overlaps d_X')
    einval(var(scale=at(1001)), 'd_out overlaps d_scale')
    einval(var(mask=at(1001)), 'd_out overlaps d_mask')

    n = nat.c_i64(0)
    assert lib.dsp_svm_fit_workspace_bytes(100, 5, 3, C.byref(n)) == 0 and n.value == 4096 + 3 * 100 * 4
    need = n.value
    einval(lib.dsp_svm_fit_workspace_bytes(100, 5, 3, None), 'NULL argument')
    einval(lib.dsp_svm_fit_workspace_bytes(1, 5, 3, C.byref(n)), 'n 1')
    einval(lib.dsp_svm_fit_workspace_bytes(8193, 5, 3, C.byref(n)), 'n 8193')
    einval(lib.dsp_svm_fit_workspace_bytes(100, 0, 3, C.byref(n)), 'F 0')
    einval(lib.dsp_svm_fit_workspace_bytes(100, 5, 0, C.byref(n)), 'P 0')
    einval(lib.dsp_svm_fit_workspace_bytes(100, 5, 65536, C.byref(n)), 'P 65536')

    def fit(**kw):
        d = dict(X=at(0), ld=5, n=100, F=5, center=at(600), scale=at(620), Y=at(700), ld_y=100, P=3, C=at(800), gamma=at(810), tol=1e-3,
                 max_iter=1000, coef=at(1000), ld_coef=100, rho=at(1400), info=at(1500), work=at(2000), work_bytes=need, stream=None)
        d.update(kw)
        return lib.dsp_svm_fit_batch(*d.values())
    einval(fit(n=1), 'n 1')
    einval(fit(F=17, ld=17), 'F 17')
    einval(fit(P=0), 'P 0')
    einval(fit(X=None), 'NULL matrix d_X')
    einval(fit(ld=3), 'ld 3')
    einval(fit(Y=None), 'NULL labels')
    einval(fit(C=None), 'NULL labels')
    einval(fit(gamma=None), 'NULL labels')
    einval(fit(ld_y=99), 'ld_y 99')
    einval(fit(tol=0.0), 'tol must be finite and positive')
    einval(fit(tol=float('inf')), 'tol must be finite and positive')
    einval(fit(max_iter=0), 'max_iter 0')
    einval(fit(max_iter=10000001), 'max_iter 10000001')
    einval(fit(coef=None), 'NULL output')
    einval(fit(rho=None), 'NULL output')
    einval(fit(info=None), 'NULL output')
    einval(fit(ld_coef=99), 'ld_coef 99')
    einval(fit(work=None), 'NULL workspace')
    einval(fit(work=at(2001)), '16-byte aligned')
    einval(fit(C=at(800) + 4), 'aligned to its element size')
    einval(fit(work_bytes=need - 1), 'is short of')
    einval(fit(coef=at(400)), 'd_coef overlaps d_X')
    einval(fit(rho=at(801)), 'd_rho overlaps d_C')
    einval(fit(rho=at(811)), 'd_rho overlaps d_gamma')
    einval(fit(info=at(710)), 'd_info overlaps d_Y')
    einval(fit(rho=at(601)), 'd_rho overlaps d_center')
    einval(fit(rho=at(621)), 'd_rho overlaps d_scale')
    einval(fit(rho=at(1299)), 'd_coef overlaps d_rho')
    einval(fit(info=at(2100)), 'd_info overlaps the workspace')

    # what passes every check is refused under the dry run instead of launched
    assert lib.dsp_debug_host_dry_run(1) == 0
    try:
        einval(scaler(), 'dry_run: launches are refused')
        einval(scaler(valid=at(2000), ld_valid=9, centering=1, center=at(1010), q_lo=0.0, q_hi=100.0), 'dry_run: launches are refused')
        einval(var(), 'dry_run: launches are refused')
        einval(var(center=at(600), scale=at(620), mask=at(700)), 'dry_run: launches are refused')
        einval(fit(), 'dry_run: launches are refused')
        einval(fit(center=None, scale=None, P=1, max_iter=10000000), 'dry_run: launches are refused')
    finally:
        lib.dsp_debug_host_dry_run(0)


def test_python_refusals_need_no_device():
    from features import svmfit
    with pytest.raises(ValueError, match='two distinct labels'):
        svmfit._classes_of(np.array([1, 1, 1]), None)
    with pytest.raises(ValueError, match='two distinct labels'):
        svmfit._classes_of(np.array([0, 1, 2]), None)
    assert svmfit._classes_of(np.array([7, 6, 7]), None) == [6, 7] and svmfit._classes_of(None, (1, 0)) == [0, 1]
    assert svmfit.default_max_iter(400) == 40000 and svmfit.default_max_iter(50) == 10000
    folds = svmfit.stratified_folds(np.array([1, -1, 0, 1, 1, -1, -1, 1]), 2)
    assert folds.tolist() == [0, 0, -1, 1, 0, 1, 0, 1]
    with pytest.warns(svmfit.SvmConvergenceWarning):
        svmfit._raise_or_warn(1, 3, 3)
    for status in (2, 3, 4):
        with pytest.raises(ValueError, match=f'status {status}'):
            svmfit._raise_or_warn(status, 0, 3)


def test_package_still_imports_nothing_of_sklearn():
    pkg = os.path.join(ROOT, 'dsp-speech-recognition_amd', 'features')
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith('.py'):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r'^\s*(import|from)\s+(sklearn|matplotlib)', src, re.M), fn
    src = open(os.path.join(ROOT, 'tools', 'svm_fit_emul.py')).read()
    assert not re.search(r'^\s*(import|from)\s+sklearn', src, re.M)
    code = ('import sys; sys.path[:0] = [%r, %r]; import features, features.svmfit; '
            'bad = [m for m in sys.modules if m.split(".")[0] in ("sklearn", "matplotlib")]; assert not bad, bad'
            % (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd')))
    r = subprocess.run([sys.executable, '-c', code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]


def test_asan_svmfit_builds_and_exits_clean():
    """The stand-alone program behind ``make asan-svmfit`` (tools/asan_svmfit_args.cpp) holds the checks of each new entry
    point; it is built against the sanitized library and run as a program of its own (profiles/asan_svmfit.txt keeps one
    run's output)."""
    src = open(os.path.join(ROOT, 'tools', 'asan_svmfit_args.cpp')).read()
    for name, call in zip(NEW, ('dsp_robust_scale_fit_batch', 'dsp_var_all', 'dsp_svm_fit_workspace_bytes', 'FIT')):
        assert len(re.findall(r'EXPECT\(' + call + r'\(', src)) >= 5, name
    jobs = str(max(1, min(8, os.cpu_count() or 1)))
    r = subprocess.run(['make', '-C', CSRC, '-j', jobs, 'asan-svmfit'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'asan_svmfit_args: ok' in r.stdout, r.stdout[-4000:]
