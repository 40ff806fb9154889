#!/usr/bin/env python3
"""Generate tests/golden/svmfit_golden.npz: scikit-learn's RESULTS of RobustScaler.fit + SVC(kernel='rbf').fit on the seeded
cases of tests/svmfit_cases.py (the training rows and queries are regenerated from their seeds, never stored), and per case
the distance of the NumPy restatement (tools/svm_fit_emul.py) to scikit-learn's decisions, `d_ref`.

    python tests/golden/make_svmfit_golden.py     # needs scikit-learn; rewrites svmfit_golden.npz + svmfit_manifest.json

Refuses to write a fixture with a case where more than 2 % of the queries have |decision| < 4 tol, more than 1 % of the
training rows have 0 < |coef| < 1e-4 (on either side), the restatement disagrees with scikit-learn in a prediction
outside those queries, or its support set differs from scikit-learn's outside those rows (at tol 1e-3 a problem with many
nearly interchangeable rows, one feature and heavy overlap for instance, has several solutions within the tolerance whose
support sets differ: such data cannot carry a support-set comparison, pick other data).
"""
import io
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), 'tools'))

import svm_fit_emul as emul  # noqa: E402
from svmfit_cases import CASES, MAX_ITER, TOLS, case, key  # noqa: E402


def main():
    import sklearn
    from sklearn.preprocessing import RobustScaler
    from sklearn.svm import SVC
    out = {}
    for name in CASES:
        X, y, Q, a = case(name)
        scaler = RobustScaler(with_centering=a['with_centering'], quantile_range=a['quantile_range']).fit(X)
        Xs, Qs = scaler.transform(X), scaler.transform(Q)
        classes = np.unique(y)
        center, scale, st = emul.robust_scale_fit(X, None, a['with_centering'], a['quantile_range'])
        assert st == 0
        for tol in TOLS:
            clf = SVC(kernel='rbf', C=a['C'], gamma=a['gamma'], tol=tol)
            with warnings.catch_warnings():
                warnings.simplefilter('error')                     # a ConvergenceWarning is a refusal
                clf.fit(Xs, y)
            dec = clf.decision_function(Qs)
            coef_sk = np.zeros(len(X))
            coef_sk[clf.support_] = clf.dual_coef_[0]
            r = emul.svm_fit(emul.transform(X, scale, center), np.where(y == classes[1], 1, -1), a['C'], clf._gamma, tol=tol,
                             max_iter=MAX_ITER)
            assert r['status'] == 0, (name, tol, r['status'])
            dec_e = emul.decision(emul.transform(X, scale, center), r['coef'], r['rho'], clf._gamma, emul.transform(Q, scale, center))
            d_ref = float(np.max(np.abs(dec_e - dec)))
            near = np.abs(dec) < 4 * tol
            small = ((np.abs(coef_sk) > 0) & (np.abs(coef_sk) < 1e-4)) | ((np.abs(r['coef']) > 0) & (np.abs(r['coef']) < 1e-4))
            pred = clf.predict(Qs)
            pred_e = classes[(dec_e > 0).astype(int)]
            k = key(name, tol)
            if near.mean() > 0.02:
                raise SystemExit(f'{k}: {near.mean():.1%} of the queries have |decision| < 4 tol')
            if small.mean() > 0.01:
                raise SystemExit(f'{k}: {small.mean():.1%} of the rows have 0 < |coef| < 1e-4')
            if (pred != pred_e)[~near].any():
                raise SystemExit(f'{k}: the restatement disagrees with scikit-learn in a prediction away from the boundary')
            same_sv = np.array_equal((coef_sk != 0) | small, (r['coef'] != 0) | small)
            if not same_sv:
                raise SystemExit(f'{k}: the support set of the restatement differs from scikit-learn\'s: pick other data')
            out.update({f'{k}/support': clf.support_.astype(np.int32), f'{k}/dual_coef': clf.dual_coef_[0],
                        f'{k}/intercept': np.float64(clf.intercept_[0]), f'{k}/gamma': np.float64(clf._gamma),
                        f'{k}/n_iter': np.int64(np.asarray(clf.n_iter_).reshape(-1)[0]), f'{k}/fit_status': np.int64(clf.fit_status_),
                        f'{k}/decision': dec, f'{k}/predict': pred.astype(np.int64), f'{k}/d_ref': np.float64(d_ref)})
            print(f"{k:22s} n {len(X):5d} F {X.shape[1]:2d} gamma {clf._gamma:.4g} n_sv {len(clf.support_):5d} / {r['n_sv']:5d} "
                  f"bounded {r['n_bounded']:5d} iter {int(out[f'{k}/n_iter']):6d} / {r['n_iter']:6d} d_ref {d_ref:.2e} "
                  f"near {near.mean():.1%} small {small.mean():.1%} same_sv {same_sv} scale== {np.array_equal(scale, scaler.scale_)}")
        out[f'{name}/scale'] = scaler.scale_
        out[f'{name}/classes'] = classes.astype(np.int64)
        if a['with_centering']:
            out[f'{name}/center'] = scaler.center_
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    assert len(buf.getvalue()) < (1 << 20), len(buf.getvalue())
    with open(os.path.join(HERE, 'svmfit_golden.npz'), 'wb') as f:
        f.write(buf.getvalue())
    with open(os.path.join(HERE, 'svmfit_manifest.json'), 'w') as f:
        json.dump({'numpy': np.__version__, 'sklearn': sklearn.__version__,
                   'arrays': {k: [list(np.shape(v)), str(np.asarray(v).dtype)] for k, v in out.items()}}, f, indent=1, sort_keys=True)
    print(f'wrote svmfit_golden.npz: {len(out)} arrays, {len(buf.getvalue()) / 1e6:.2f} MB')


if __name__ == '__main__':
    main()
