#!/usr/bin/env python3
"""The scaler fit and the SVM solver of csrc/kernels_svmfit.h restated in NumPy fp64, rule for rule: positions in the
ascending list of a problem's rows, first-index ties in both selections, the 1e-12 curvature floor, libsvm's four clipping
cases and its calculate_rho.  It is the yardstick between scikit-learn (whose libsvm keeps its kernel rows in `float`) and
the device (which differs from this file only in the rounding of exp, the fused squared distance and the order of the sum
behind rho).  tests/golden/make_svmfit_golden.py stores this file's distance to scikit-learn per fixture; nothing here
imports scikit-learn.

    python tools/svm_fit_emul.py            # a small self-check: KKT conditions on a seeded problem
"""
import numpy as np

TAU = 1e-12
OK, MAX_ITER, NONFINITE, ONE_CLASS, BAD_HYPER = 0, 1, 2, 3, 4


def percentile_linear(sorted_vals, percent):
    """np.percentile(..., method='linear') on an ascending 1-D array, every rounding spelled out."""
    m = len(sorted_vals)
    q = np.float64(percent) / np.float64(100.0)
    vi = (np.float64(m) * q + (np.float64(1.0) - q)) - np.float64(1.0)
    if vi >= m - 1:
        return np.float64(sorted_vals[m - 1])
    if vi < 0:
        return np.float64(sorted_vals[0])
    k = int(np.floor(vi))
    a, b, t = np.float64(sorted_vals[k]), np.float64(sorted_vals[k + 1]), vi - np.floor(vi)
    d = b - a
    if t >= 0.5:
        return b - d * (np.float64(1.0) - t)
    return a + d * t


def robust_scale_fit(X, valid=None, with_centering=False, quantile_range=(25.0, 75.0)):
    """-> (center or None, scale, status): RobustScaler(with_centering).fit on the valid rows; status 1 = no valid row,
    2 = a valid row holds a non-finite value (center and scale are None then)."""
    X = np.asarray(X, dtype=np.float64)
    rows = X if valid is None else X[np.asarray(valid) != 0]
    if len(rows) < 1:
        return None, None, 1
    if not np.isfinite(rows).all():
        return None, None, NONFINITE
    F = X.shape[1]
    scale, center = np.empty(F), np.empty(F)
    for f in range(F):
        s = np.sort(rows[:, f])
        sc = percentile_linear(s, quantile_range[1]) - percentile_linear(s, quantile_range[0])
        scale[f] = 1.0 if sc < 10 * np.finfo(np.float64).eps else sc
        center[f] = (s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2.0
    return (center if with_centering else None), scale, OK


def transform(X, scale=None, center=None):
    X = np.asarray(X, dtype=np.float64)
    if center is not None:
        X = X - center
    return X / scale if scale is not None else X.copy()


def rbf_row(Xs, i, gamma):
    d = Xs - Xs[i]
    d2 = np.zeros(len(Xs))
    for f in range(Xs.shape[1]):            # in feature order, as the kernel adds them
        d2 = d2 + d[:, f] * d[:, f]
    return np.exp(-gamma * d2)


def svm_fit(Xs, y, C, gamma, tol=1e-3, max_iter=None):
    """One problem.  ``Xs`` [n, F]: the SCALED rows; ``y`` [n] in {-1, 0, +1}, 0 = the row is not in the problem.
    -> dict(coef [n] = y alpha with exact zeros, rho, n_iter, status, n_sv, n_bounded, n_active, G (active positions))."""
    Xs = np.asarray(Xs, dtype=np.float64)
    y_all = np.sign(np.asarray(y)).astype(np.int64)
    n = len(y_all)
    if max_iter is None:
        max_iter = max(10000, 100 * n)
    rows = np.flatnonzero(y_all != 0)
    na = len(rows)
    out = dict(coef=np.zeros(n), rho=0.0, n_iter=0, n_sv=0, n_bounded=0, n_active=na, G=None)
    X = Xs[rows]
    y = y_all[rows].astype(np.float64)
    if not np.isfinite(X).all():
        return dict(out, status=NONFINITE)
    if not (np.isfinite(C) and C > 0 and np.isfinite(gamma) and gamma > 0):
        return dict(out, status=BAD_HYPER)
    if (y > 0).sum() < 1 or (y < 0).sum() < 1:
        return dict(out, status=ONE_CLASS)
    alpha, G = np.zeros(na), -np.ones(na)
    pos = y > 0
    status, it = MAX_ITER, 0
    while it < max_iter:
        v = -y * G
        up = np.where(pos, alpha < C, alpha > 0)
        low = np.where(pos, alpha > 0, alpha < C)
        if not up.any() or not low.any():
            status = OK
            break
        i = int(np.argmax(np.where(up, v, -np.inf)))             # first index among equals
        m, M = v[i], np.min(v[low])
        if m - M < tol:
            status = OK
            break
        Ki = rbf_row(X, i, gamma)
        b = m - v
        cand = low & (b > 0)
        if not cand.any():
            status = OK
            break
        a = 2.0 - 2.0 * Ki
        a = np.where(a <= 0, TAU, a)
        obj = np.where(cand, -(b * b) / a, np.inf)
        j = int(np.argmin(obj))                                  # first index among equals
        Kj = rbf_row(X, j, gamma)
        quad = 2.0 - 2.0 * Ki[j]
        if quad <= 0:
            quad = TAU
        ai, aj = alpha[i], alpha[j]
        ni, nj = ai, aj
        if y[i] != y[j]:
            delta = (-G[i] - G[j]) / quad
            diff = ai - aj
            ni, nj = ni + delta, nj + delta
            if diff > 0:
                if nj < 0:
                    nj, ni = 0.0, diff
            else:
                if ni < 0:
                    ni, nj = 0.0, -diff
            if diff > 0:
                if ni > C:
                    ni, nj = C, C - diff
            else:
                if nj > C:
                    nj, ni = C, C + diff
        else:
            delta = (G[i] - G[j]) / quad
            s = ai + aj
            ni, nj = ni - delta, nj + delta
            if s > C:
                if ni > C:
                    ni, nj = C, s - C
            else:
                if nj < 0:
                    nj, ni = 0.0, s
            if s > C:
                if nj > C:
                    nj, ni = C, s - C
            else:
                if ni < 0:
                    ni, nj = 0.0, s
        di, dj = ni - ai, nj - aj
        G = G + (y[i] * y * Ki) * di + (y[j] * y * Kj) * dj
        alpha[i], alpha[j] = ni, nj
        it += 1
    rho, n_sv, n_bounded = calculate_rho(alpha, G, y, C)
    coef = np.zeros(n)
    coef[rows] = np.where(alpha > 0, y * alpha, 0.0)
    return dict(coef=coef, rho=rho, n_iter=it, status=status, n_sv=n_sv, n_bounded=n_bounded, n_active=na, G=G)


def calculate_rho(alpha, G, y, C):
    """libsvm's rule -> (rho, n_sv, n_bounded): the mean of y G over the free alpha, else the midpoint of the bounds."""
    yG = y * G
    pos = y > 0
    at_c, at_0 = alpha >= C, alpha <= 0
    free = ~at_c & ~at_0
    ub_set = (at_c & ~pos) | (at_0 & pos)
    lb_set = (at_c & pos) | (at_0 & ~pos)
    ub = np.min(yG[ub_set]) if ub_set.any() else np.inf
    lb = np.max(yG[lb_set]) if lb_set.any() else -np.inf
    rho = yG[free].sum() / free.sum() if free.any() else (ub + lb) / 2.0
    return float(rho), int((alpha > 0).sum()), int(at_c.sum())


def decision(Xs_train, coef, rho, gamma, Qs):
    """sum_i coef_i exp(-gamma |q - x_i|^2) - rho for SCALED queries ``Qs`` against SCALED training rows."""
    sv = np.flatnonzero(coef != 0)
    d2 = ((Qs[:, None, :] - Xs_train[None, sv, :]) ** 2).sum(-1)
    return np.exp(-gamma * d2) @ coef[sv] - rho


def kkt(Xs, y, coef, C, gamma):
    """A fresh gradient from the coefficients -> (m - M, max |G|, G, alpha, y) over the problem's rows."""
    y_all = np.sign(np.asarray(y)).astype(np.float64)
    rows = np.flatnonzero(y_all != 0)
    X, yy = np.asarray(Xs, dtype=np.float64)[rows], y_all[rows]
    alpha = np.abs(np.asarray(coef, dtype=np.float64)[rows])
    d2 = np.zeros((len(X), len(X)))
    for f in range(X.shape[1]):
        d2 += (X[:, f, None] - X[None, :, f]) ** 2
    G = (yy[:, None] * yy[None, :] * np.exp(-gamma * d2)) @ alpha - 1.0
    v = -yy * G
    up = np.where(yy > 0, alpha < C, alpha > 0)
    low = np.where(yy > 0, alpha > 0, alpha < C)
    m = np.max(v[up]) if up.any() else -np.inf
    M = np.min(v[low]) if low.any() else np.inf
    return m - M, float(np.max(np.abs(G))), G, alpha, yy


if __name__ == '__main__':
    rng = np.random.default_rng(0)
    yy = rng.integers(0, 2, 300) * 2 - 1
    XX = rng.standard_normal((300, 5)) + 0.8 * yy[:, None]
    _, sc, _ = robust_scale_fit(XX)
    Xs = transform(XX, sc)
    for tol in (1e-3, 1e-6):
        r = svm_fit(Xs, yy, 1.0, 0.2, tol=tol)
        gap = kkt(Xs, yy, r['coef'], 1.0, 0.2)[0]
        print(f"tol {tol:g}: n_iter {r['n_iter']} n_sv {r['n_sv']} bounded {r['n_bounded']} rho {r['rho']:.6f} fresh KKT gap {gap:.3e}")
        assert r['status'] == OK and gap < tol + 1e-9
