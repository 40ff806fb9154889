"""Fitting the pitch model on the device (features/svmfit.py; dsp_robust_scale_fit_batch, dsp_var_all, dsp_svm_fit_batch)
against scikit-learn's stored results (tests/golden/svmfit_golden.npz) and conditions that need no reference
(tests/svmfit_ref.py).

Bars: scale_ / center_ equal scikit-learn's under ``==``; decisions of the fitted model within 4 d_ref of scikit-learn's,
d_ref being the stored distance of the NumPy restatement (tools/svm_fit_emul.py) to scikit-learn -- libsvm keeps its kernel
rows in float, the device differs from the restatement only in the rounding of exp and in summation order, the factor 4
covers a diverging pair sequence; predictions equal outside |sklearn decision| < 4 tol; support sets equal outside rows with
|coef| < 1e-4 on either side; gamma='scale' / 'auto' within 1e-12 relative of SVC._gamma; everything that is claimed bit for
bit under ``==`` on the bytes.  ``max_iter`` is passed explicitly (<= 200 000) everywhere."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, record

sys.path.insert(0, os.path.join(ROOT, 'tools'))

import svm_fit_emul as emul  # noqa: E402
from svmfit_cases import CASES, MAX_ITER, TOLS, case, key  # noqa: E402
from svmfit_ref import check_conditions  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 4096
SENT32 = np.int32(0x7fc0beef)            # a quiet-NaN pattern: never a result


@pytest.fixture(scope='module')
def sgold():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'svmfit_golden.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def env():
    import types

    import torch
    from features import _native as nat
    from features import ensemble, svmfit
    nat.require_device()
    return types.SimpleNamespace(nat=nat, lib=nat.load(), ens=ensemble, fit=svmfit, torch=torch, dev=torch.device('cuda', 0))


def _dev(env, arr):
    return env.torch.from_numpy(np.ascontiguousarray(arr)).to(env.dev)


def _guarded(env, nbytes):
    torch = env.torch
    total = (PAD + nbytes + PAD + 3) // 4 * 4
    buf = torch.empty(total // 4, dtype=torch.int32, device=env.dev)
    buf.fill_(int(SENT32))
    raw = buf.view(torch.uint8)

    def check(what):
        torch.cuda.synchronize(env.dev)
        host = raw.cpu().numpy()
        sent = np.full(total // 4, SENT32, dtype=np.int32).view(np.uint8)
        assert np.array_equal(host[:PAD], sent[:PAD]), f'{what}: bytes BEFORE the buffer were written'
        assert np.array_equal(host[PAD + nbytes:], sent[PAD + nbytes:]), f'{what}: bytes AFTER the buffer were written'
        return host[PAD:PAD + nbytes]
    return buf, buf.data_ptr() + PAD, check


def _stream(env):
    return env.torch.cuda.current_stream(env.dev).cuda_stream


@pytest.fixture(scope='module')
def pair01(env, sgold):
    """The 400-row training set with its scaler and sklearn's gamma, on the host and on the device (computed once)."""
    import types
    X, y, Q, a = case('pair01_c1')
    scale = sgold['pair01_c1/scale']
    gamma = float(sgold[key('pair01_c1', 1e-3) + '/gamma'])
    return types.SimpleNamespace(X=X, y=y, Q=Q, scale=scale, gamma=gamma, Xs=X / scale, yrow=np.where(y == 1, 1, -1).astype(np.int8),
                                 dX=_dev(env, X), dscale=_dev(env, scale))


def _host(r):
    return r.coef.cpu().numpy(), r.rho.cpu().numpy(), r.info.cpu().numpy()


# ---- 1: the scaler ----
@pytest.mark.parametrize('name', list(CASES))
def test_scaler_equals_sklearn(env, sgold, name):
    torch = env.torch
    X, _, _, a = case(name)
    want_scale = sgold[f'{name}/scale']
    want_center = sgold[f'{name}/center'] if a['with_centering'] else None
    kw = dict(with_centering=a['with_centering'], quantile_range=a['quantile_range'])
    # host array in, host arrays out
    center, scale = env.fit.robust_scale_fit(X, **kw)
    assert np.array_equal(scale, want_scale), (scale, want_scale)
    assert (center is None) if want_center is None else np.array_equal(center, want_center)
    # a strided view on the device, and the valid column with stride 9 as the pitch features leave it: two invalid rows whose
    # values would move every quantile are excluded
    n, F = X.shape
    wide = np.full((n + 2, F + 3), 1e6)
    wide[1:n + 1, :F] = X
    d_wide = _dev(env, wide)
    aux = np.zeros((n + 2, 9), dtype=np.int32)
    aux[1:n + 1, 8] = 1
    d_aux = _dev(env, aux)
    center_d, scale_d, info = env.fit.robust_scale_fit(d_wide[:, :F], valid=d_aux[:, 8], return_info=True, **kw)
    assert d_wide[:, :F].stride(0) == F + 3 and d_aux[:, 8].stride(0) == 9
    assert info.cpu().numpy().tolist() == [n, 0]
    assert scale_d.cpu().numpy().tobytes() == want_scale.tobytes()
    if want_center is not None:
        assert center_d.cpu().numpy().tobytes() == want_center.tobytes()


def test_scaler_nan_in_a_valid_row_writes_nothing_but_the_info(env):
    torch = env.torch
    X, _, _, _ = case('pair01_c1')
    bad = X.copy()
    bad[17, 3] = np.nan
    d_X = _dev(env, bad)
    hold_s, p_scale, check_s = _guarded(env, 5 * 8)
    hold_c, p_center, check_c = _guarded(env, 5 * 8)
    hold_i, p_info, check_i = _guarded(env, 8)
    for centering in (0, 1):
        env.nat.check(env.lib.dsp_robust_scale_fit_batch(d_X.data_ptr(), 5, len(X), 5, None, 0, 25.0, 75.0, centering, p_scale, p_center,
                                                         p_info, _stream(env)))
        assert check_i('d_info').view(np.int32).tolist() == [len(X), 2]
        sent = np.full(10, SENT32, dtype=np.int32).view(np.uint8)
        assert np.array_equal(check_s('d_scale'), sent) and np.array_equal(check_c('d_center'), sent)
    # the same NaN in a row that is not valid: fitted, and only d_scale / d_info written (no centering: d_center untouched)
    valid = np.ones(len(X), dtype=np.int32)
    valid[17] = 0
    d_valid = _dev(env, valid)
    env.nat.check(env.lib.dsp_robust_scale_fit_batch(d_X.data_ptr(), 5, len(X), 5, d_valid.data_ptr(), 1, 25.0, 75.0, 0, p_scale, p_center,
                                                     p_info, _stream(env)))
    assert check_i('d_info').view(np.int32).tolist() == [len(X) - 1, 0]
    _, want, st = emul.robust_scale_fit(bad, valid)
    assert st == 0 and check_s('d_scale').view(np.float64).tobytes() == want.tobytes()
    assert np.array_equal(check_c('d_center'), np.full(10, SENT32, dtype=np.int32).view(np.uint8))
    with pytest.raises(ValueError, match='non-finite'):
        env.fit.robust_scale_fit(bad)
    with pytest.raises(ValueError, match='no valid row'):
        env.fit.robust_scale_fit(X, valid=np.zeros(len(X)))


# ---- 2 + 3: conditions that need no reference, and scikit-learn's stored numbers ----
@pytest.mark.parametrize('name', list(CASES))
def test_fit_against_sklearn_and_the_conditions(env, sgold, name):
    X, y, Q, a = case(name)
    classes = sgold[f'{name}/classes']
    scale = sgold[f'{name}/scale']
    center = sgold[f'{name}/center'] if a['with_centering'] else None
    Xs = emul.transform(X, scale, center)
    d_X, d_y, d_Q = _dev(env, X), _dev(env, y.astype(np.int64)), _dev(env, Q)
    for tol in TOLS:
        k = key(name, tol)
        svm = env.fit.fit_pitch_svm(d_X, d_y, C=a['C'], gamma=a['gamma'], tol=tol, max_iter=MAX_ITER, with_centering=a['with_centering'],
                                    quantile_range=a['quantile_range'])
        info = svm.fit_info
        assert info['status'] == 0 and svm.classes == tuple(int(c) for c in classes)
        assert svm.scale.tobytes() == scale.tobytes() and ((svm.center is None) if center is None else svm.center.tobytes() == center.tobytes())
        # 4: the resolved gamma
        want_gamma = float(sgold[f'{k}/gamma'])
        assert abs(svm.gamma - want_gamma) <= 1e-12 * want_gamma, (svm.gamma, want_gamma)
        # the model's layout: classes[0] rows first, each class in row order; intercept = -rho
        coef = np.zeros(len(X))
        coef[info['support']] = svm.dual_coef
        neg, pos = np.flatnonzero(coef < 0), np.flatnonzero(coef > 0)
        assert info['support'].tolist() == neg.tolist() + pos.tolist() and (y[neg] == classes[0]).all() and (y[pos] == classes[1]).all()
        assert svm.intercept == -info['rho'] and svm.support_vectors.tobytes() == Xs[info['support']].tobytes()
        # 2: the conditions, from a fresh gradient on the host
        yrow = np.where(y == classes[1], 1, -1)
        gap, drift = check_conditions(Xs, yrow, coef, info['rho'], info['n_iter'], info['n_sv'], info['n_bounded'], a['C'], svm.gamma, tol)
        # 3: scikit-learn's stored numbers
        dec = svm.decision_function(d_Q).cpu().numpy()
        want = sgold[f'{k}/decision']
        d_ref = float(sgold[f'{k}/d_ref'])
        d = float(np.max(np.abs(dec - want)))
        print(k, 'n_iter', info['n_iter'], '(sklearn', int(sgold[f'{k}/n_iter']), ') n_sv', info['n_sv'], 'KKT gap', gap, 'drift', drift,
              'max |device - sklearn|', d, 'd_ref', d_ref)
        record(f'svmfit_decision_{k}', d)
        record(f'svmfit_decision_over_dref_{k}', d / d_ref)
        assert d <= 4 * d_ref, (k, d, d_ref)
        near = np.abs(want) < 4 * tol
        pred = svm.predict(d_Q).cpu().numpy()
        assert (pred == sgold[f'{k}/predict'])[~near].all()
        coef_sk = np.zeros(len(X))
        coef_sk[sgold[f'{k}/support']] = sgold[f'{k}/dual_coef']
        small = ((np.abs(coef_sk) > 0) & (np.abs(coef_sk) < 1e-4)) | ((np.abs(coef) > 0) & (np.abs(coef) < 1e-4))
        assert np.array_equal((coef_sk != 0) | small, (coef != 0) | small), np.flatnonzero(((coef_sk != 0) != (coef != 0)) & ~small)


# ---- 5: bits ----
def test_same_bytes_every_run_every_batch_every_layout(env, pair01):
    torch = env.torch
    f = pair01
    n = len(f.X)
    Cs = np.array([1.0, 0.01, 100.0, 1.0, 3.0, 0.5, 10.0])
    gs = np.array([f.gamma, f.gamma, f.gamma, 0.5, 0.05, f.gamma, 1.0])
    masked = f.yrow.copy()
    masked[::3] = 0
    masked[5] = 0
    Y = np.stack([f.yrow] * 6 + [masked])
    kw = dict(tol=1e-3, max_iter=MAX_ITER, scale=f.dscale)
    batch = _host(env.fit.svm_fit_problems(f.dX, Y, Cs, gs, **kw))
    again = _host(env.fit.svm_fit_problems(f.dX, Y, Cs, gs, **kw))
    for a, b in zip(batch, again):
        assert a.tobytes() == b.tobytes()                                            # two runs, the same bytes
    assert (batch[2][:, 1] == 0).all()
    for p in (0, 2, 4, 6):                                                           # problem p of the batch = the P = 1 call
        one = _host(env.fit.svm_fit_problems(f.dX, Y[p], Cs[p], gs[p], **kw))
        assert one[0][0].tobytes() == batch[0][p].tobytes() and one[1][0] == batch[1][p] and one[2][0].tolist() == batch[2][p].tolist()
    # the masked problem = the same problem on the compacted matrix (fewer rows: another workgroup size at n <= 512 / 256)
    keep = masked != 0
    comp = _host(env.fit.svm_fit_problems(_dev(env, f.X[keep]), masked[keep], Cs[6], gs[6], **kw))
    assert comp[0][0].tobytes() == batch[0][6][keep].tobytes() and comp[1][0] == batch[1][6]
    assert comp[2][0].tolist() == batch[2][6].tolist() and (batch[0][6][~keep] == 0).all() and batch[2][6][4] == keep.sum()
    small = keep & (np.arange(n) < 185)                                              # 128 rows or fewer: one row per thread
    y_small = np.where(small, masked, 0)
    assert 64 < small.sum() <= 128
    a = _host(env.fit.svm_fit_problems(f.dX, y_small, 1.0, f.gamma, **kw))
    b = _host(env.fit.svm_fit_problems(_dev(env, f.X[small]), masked[small], 1.0, f.gamma, **kw))
    assert a[0][0][small].tobytes() == b[0][0].tobytes() and a[1][0] == b[1][0] and a[2][0].tolist() == b[2][0].tolist()
    # a strided X at the weakest alignment an fp64 matrix can have (8 bytes, not 16) = the dense, 16-byte-aligned one
    wide = torch.zeros((n, 7), dtype=torch.float64, device=env.dev)
    wide[:, 1:6] = f.dX
    strided = wide[:, 1:6]
    assert strided.stride(0) == 7 and strided.data_ptr() % 16 == 8
    s = _host(env.fit.svm_fit_problems(strided, Y, Cs, gs, **kw))
    for a, b in zip(batch, s):
        assert a.tobytes() == b.tobytes()


# ---- 6: status paths ----
def test_status_paths(env, pair01):
    torch = env.torch
    f = pair01
    n = len(f.X)
    r = env.fit.svm_fit_problems(f.dX, f.yrow, 1.0, f.gamma, tol=1e-3, max_iter=3, scale=f.dscale)
    coef, rho, info = _host(r)
    assert info[0].tolist()[:2] == [3, 1] and info[0][4] == n
    check_conditions(f.Xs, f.yrow, coef[0], float(rho[0]), 3, int(info[0][2]), int(info[0][3]), 1.0, f.gamma, 1e-3, check_gap=False)
    want = emul.svm_fit(f.Xs, f.yrow, 1.0, f.gamma, max_iter=3)
    assert np.array_equal(coef[0] != 0, want['coef'] != 0) and np.max(np.abs(coef[0] - want['coef'])) <= 1e-12
    with pytest.warns(env.fit.SvmConvergenceWarning):
        svm = env.fit.fit_pitch_svm(f.dX, f.y, C=1.0, gamma=f.gamma, tol=1e-3, max_iter=3)
    assert svm.fit_info['status'] == 1 and svm.fit_info['n_iter'] == 3 and svm.n_sv == int(info[0][2])

    # one class only, a NaN in an active row, a bad C: status 3 / 2 / 4, nothing but the info written; a healthy problem in
    # the same launch is solved.  Guard bytes around every output.
    bad = f.X.copy()
    bad[9, 1] = np.inf
    without9 = f.yrow.copy()
    without9[9] = 0
    cases = ((f.X, [np.abs(f.yrow), f.yrow, f.yrow, f.yrow], [1.0, 1.0, -1.0, np.nan], [3, 0, 4, 4]),
             (bad, [np.abs(without9), f.yrow, without9, f.yrow], [1.0, 1.0, 1.0, 1.0], [3, 2, 0, 2]))
    for X_in, Y, Cs, want_status in cases:
        Y = np.stack(Y).astype(np.int8)
        d_X, d_Y = _dev(env, X_in), _dev(env, Y)
        d_C, d_g = _dev(env, np.array(Cs)), _dev(env, np.full(4, f.gamma))
        need = env.nat.c_i64(0)
        env.nat.check(env.lib.dsp_svm_fit_workspace_bytes(n, 5, 4, env.nat.C.byref(need)))
        hold_c, p_coef, check_c = _guarded(env, 4 * n * 8)
        hold_r, p_rho, check_r = _guarded(env, 4 * 8)
        hold_i, p_info, check_i = _guarded(env, 4 * 20)
        hold_w, p_work, check_w = _guarded(env, need.value)
        env.nat.check(env.lib.dsp_svm_fit_batch(d_X.data_ptr(), 5, n, 5, None, f.dscale.data_ptr(), d_Y.data_ptr(), n, 4, d_C.data_ptr(),
                                                d_g.data_ptr(), 1e-3, MAX_ITER, p_coef, n, p_rho, p_info, p_work, need.value, _stream(env)))
        check_w('the workspace')
        info = check_i('d_info').view(np.int32).reshape(4, 5)
        coef = check_c('d_coef').view(np.int32).reshape(4, 2 * n)
        rho = check_r('d_rho').view(np.int32).reshape(4, 2)
        assert info[:, 1].tolist() == want_status
        for p, st in enumerate(want_status):
            if st:
                assert (coef[p] == SENT32).all() and (rho[p] == SENT32).all() and info[p].tolist() == [0, st, 0, 0, int((Y[p] != 0).sum())]
            else:
                assert not (coef[p] == SENT32).any() and info[p][0] > 0
    r = env.fit.svm_fit_problems(f.dX, f.yrow, _dev(env, np.array([-1.0])), f.gamma, tol=1e-3, max_iter=MAX_ITER, scale=f.dscale)
    assert r.status.cpu().numpy().tolist() == [4]
    with pytest.raises(ValueError, match='status 3'):
        env.fit.fit_pitch_svm(f.dX, np.where(f.y == 1, 1, 5), classes=(0, 1), max_iter=MAX_ITER)
    with pytest.raises(ValueError, match='status 2'):
        env.fit.fit_pitch_svm(bad, f.y, max_iter=MAX_ITER)
    with pytest.raises(ValueError, match='finite and positive'):
        env.fit.fit_pitch_svm(f.dX, f.y, C=0.0, max_iter=MAX_ITER)
    # rows of other labels and invalid rows are ignored: the fit equals the one on the kept rows
    y3 = f.y.copy()
    y3[::7] = 9
    valid = np.ones(n, dtype=np.int32)
    valid[3::11] = 0
    keep = (y3 != 9) & (valid != 0)
    a = env.fit.fit_pitch_svm(f.dX, y3, classes=(0, 1), valid=_dev(env, valid), max_iter=MAX_ITER)
    b = env.ens.PitchSVM.fit(f.X[keep], y3[keep], max_iter=MAX_ITER)
    assert a.dual_coef.tobytes() == b.dual_coef.tobytes() and a.intercept == b.intercept and a.gamma == b.gamma
    assert a.scale.tobytes() == b.scale.tobytes() and a.support_vectors.tobytes() == b.support_vectors.tobytes()
    assert np.flatnonzero(keep)[b.fit_info['support']].tolist() == a.fit_info['support'].tolist()


# ---- 7: the grid ----
def test_grid_search_equals_single_fits(env, pair01):
    f = pair01
    Cs, gammas, K = [0.1, 1.0, 10.0], [0.05, f.gamma, 0.5], 4
    g = env.fit.grid_search(f.dX, f.y, Cs, gammas, n_folds=K, tol=1e-3, max_iter=MAX_ITER)
    assert g.accuracy.shape == (3, 3) and g.fold_accuracy.shape == (3, 3, 4) and (g.status == 0).all()
    folds = g.fold_ids
    assert sorted(set(folds.tolist())) == [0, 1, 2, 3]
    # single fits on the same folds with the scaler of ALL rows, as the grid (and the reference) fits it once
    for a, C in enumerate(Cs):
        for b, gamma in enumerate(gammas):
            accs = []
            for k in range(K):
                train = folds != k
                r = env.fit.svm_fit_problems(f.dX, np.where(train, f.yrow, 0), C, gamma, tol=1e-3, max_iter=MAX_ITER, scale=f.dscale)
                coef, rho, _ = _host(r)
                svm, _ = env.fit._assemble(f.X, coef[0], rho[0], gamma, [0, 1], f.scale, None)
                pred = svm.predict(f.X[~train])
                accs.append(float(np.mean(pred == f.y[~train])))
            assert g.fold_accuracy[a, b].tolist() == accs, (C, gamma)
            assert g.accuracy[a, b] == np.mean(accs)
    a, b = np.unravel_index(int(np.argmax(g.accuracy)), g.accuracy.shape)
    assert g.best == (Cs[a], gammas[b])
    want = env.fit.fit_pitch_svm(f.dX, f.y, C=Cs[a], gamma=gammas[b], tol=1e-3, max_iter=MAX_ITER)
    assert g.model.dual_coef.tobytes() == want.dual_coef.tobytes() and g.model.intercept == want.intercept
    print('grid accuracy', g.accuracy.tolist(), 'best', g.best)


# ---- 8: end to end ----
def test_trainer_on_the_stored_clips(env):
    torch = env.torch
    from ensemble_cases import make_clips
    from features import pitch
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ensemble_golden.npz')) as z:
        endpoints = z['gate/endpoints']                  # the reference's, which the device endpointing reproduces
    clips, rate = make_clips()
    labels = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 5, 1, 0, 1])              # one clip of a label the model ignores
    tr = env.fit.PitchModelTrainer((0, 1), rate, max_iter=MAX_ITER)
    for lo, hi, on_device in ((0, 8, False), (8, 14, True)):                     # two batches: a host array and a device tensor
        flat = np.concatenate(clips[lo:hi])
        so = np.concatenate([[0], np.cumsum([len(c) for c in clips[lo:hi]])]).astype(np.int64)
        tr.add_batch(_dev(env, flat) if on_device else flat, so, _dev(env, labels[lo:hi]) if on_device else labels[lo:hi])
    feat, valid, y = tr.rows()
    assert feat.shape == (14, 5) and y.cpu().numpy().tolist() == labels.tolist()
    # the same rows from the host chain: endpoints, float64 pre-emphasis over the whole clip, the slice, fp32, pitch_feature_batch
    trimmed = []
    for c, (l, r) in zip(clips, endpoints):
        x = c.astype(np.float64)
        pre = np.concatenate([x[:1], x[1:] - 0.97 * x[:-1]])
        trimmed.append(pre[l:r].astype(np.float32))
    so = np.concatenate([[0], np.cumsum([len(t) for t in trimmed])]).astype(np.int64)
    want_feat, want_valid = pitch.pitch_feature_batch(np.concatenate(trimmed), so, rate)
    assert (valid.cpu().numpy() != 0).tolist() == want_valid.tolist() and want_valid.all()
    assert feat.cpu().numpy().tobytes() == want_feat.tobytes()
    svm = tr.fit()
    want = env.fit.fit_pitch_svm(want_feat, labels, classes=(0, 1), valid=want_valid, max_iter=MAX_ITER)
    assert svm.dual_coef.tobytes() == want.dual_coef.tobytes() and svm.intercept == want.intercept and svm.gamma == want.gamma
    assert svm.scale.tobytes() == want.scale.tobytes() and svm.support_vectors.tobytes() == want.support_vectors.tobytes()
    assert svm.fit_info['n_active'] == 13 and svm.fit_info['status'] == 0
    # ... and it is a rule of the gate: low-confidence logits for label 0 everywhere, so the SVM decides every clip
    logits = np.full((14, 20), -1.0, dtype=np.float32)
    logits[:, 0] = -0.5
    pred, prob, used, dec = env.ens.ensemble_decide(_dev(env, logits), [((0, 1), 0.8, svm)], feat, valid)
    alone = svm.decision_function(feat)
    assert used.cpu().numpy().tolist() == [1] * 14 and dec.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    assert pred.cpu().numpy().tolist() == svm.predict(feat).cpu().numpy().tolist()
