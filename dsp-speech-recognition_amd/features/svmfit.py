"""PitchModel.train (pitch_model.py:26-50) on the device: ``scaler.fit`` (RobustScaler), ``scaler.transform`` and ``clf.fit``
(SVC(kernel='rbf')) as launches of csrc/kernels_svmfit.h, so that the pitch models of the ensemble are fitted where their
features are made and evaluated -- nothing here imports scikit-learn.

* ``robust_scale_fit`` -- RobustScaler.fit: per feature the percentiles of the valid rows (``dsp_robust_scale_fit_batch``).
* ``svm_fit_problems`` -- P independent two-class C-SVC duals over ONE matrix in ONE launch (``dsp_svm_fit_batch``): libsvm's
  solver without shrinking and without a kernel cache, fp64, one workgroup per problem.  A problem is a row of labels
  -1 / 0 / +1, 0 = the row is not in it: label pairs, folds, grid points and invalid rows are all that.
* ``fit_pitch_svm`` -- the pair of pitch_model.py:48-50 -> a ``PitchSVM`` (also ``PitchSVM.fit``).
* ``grid_search`` -- every (C, gamma, fold) problem in one launch, the accuracy table and the refitted best model.
* ``PitchModelTrainer`` -- PitchModel.train's loop for batches of raw clips: endpointing, the pre-emphasised trim and the pitch
  features as ``EnsembleBatch`` runs them, rows accumulated on the device, then ``fit()``.

The solver differs from scikit-learn's libsvm where libsvm keeps its kernel rows in ``float`` and breaks ties towards the last
index; tools/svm_fit_emul.py restates the kernel's rules in NumPy and DESIGN.md section 7.15 records the distances.
"""
from __future__ import annotations

import types
import warnings

import numpy as np

from . import _native as nat
from .batch import _is_device_tensor, _stream_ptr
from .ensemble import MAX_FEATURES, PitchSVM

MAX_FIT_ROWS, MAX_PROBLEMS = 8192, 65535
STATUS_OK, STATUS_MAX_ITER, STATUS_NONFINITE, STATUS_ONE_CLASS, STATUS_BAD_HYPER = 0, 1, 2, 3, 4
_STATUS_TEXT = {STATUS_NONFINITE: 'a row of the problem is not finite after scaling',
                STATUS_ONE_CLASS: 'fewer than one row in either class',
                STATUS_BAD_HYPER: 'C or gamma is not finite and positive'}


class SvmConvergenceWarning(RuntimeWarning):
    """The solver stopped at ``max_iter`` (status 1); the model holds the solution so far, as scikit-learn's does under its
    ConvergenceWarning."""


def _device():
    import torch
    nat.require_device()
    return torch.device('cuda', nat.current_device())


def _stream(dev):
    import torch
    return _stream_ptr(torch.cuda.current_stream(dev))


def _matrix(X, dev=None):
    """-> (fp64 device tensor [n, F] with a unit inner stride, was it a device tensor)."""
    import torch
    on_device = _is_device_tensor(X)
    if on_device:
        if X.dtype != torch.float64:
            raise TypeError(f'a matrix on the device must be float64, got {X.dtype}')
        x = X
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float64))).to(dev or _device())
    if x.dim() != 2 or not 1 <= x.shape[1] <= MAX_FEATURES:
        raise ValueError(f'the matrix must be [n, 1 .. {MAX_FEATURES}], got {tuple(x.shape)}')
    if not 1 <= x.shape[0] <= MAX_FIT_ROWS:
        raise ValueError(f'n = {x.shape[0]} rows: 1 .. {MAX_FIT_ROWS} are served')
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x, on_device


def _vector(v, F, dev, name):
    import torch
    if v is None:
        return None
    t = v if _is_device_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))).to(dev)
    if t.dtype != torch.float64 or t.dim() != 1 or t.shape[0] != F:
        raise ValueError(f'{name} must be {F} float64 values')
    return t.contiguous()


def robust_scale_fit(X, valid=None, with_centering=False, quantile_range=(25.0, 75.0), return_info=False):
    """RobustScaler(with_centering=..., quantile_range=...).fit(X[valid]) -> ``(center or None, scale)``, fp64 [F].

    ``X``: [n, F] fp64, a device tensor (any row stride; its results are device tensors and nothing is synchronised) or a host
    array (host arrays come back; a non-finite valid row or no valid row raises ValueError).  ``valid``: one flag per row,
    e.g. ``aux[:, 8]`` of the pitch features as it lies (int32, any stride), or None for every row.  On the device path a
    failed fit leaves NaN in ``scale`` (so a fit on it reports status 2); ``return_info=True`` adds the int32 [2] tensor
    (valid rows, status: 0 fitted, 1 no valid row, 2 non-finite value)."""
    import torch
    x, on_device = _matrix(X)
    dev, (n, F) = x.device, x.shape
    p_valid, ld_valid = None, 0
    if valid is not None:
        v = valid if _is_device_tensor(valid) else torch.from_numpy(np.ascontiguousarray(np.asarray(valid) != 0).astype(np.int32)).to(dev)
        if v.dtype != torch.int32:
            v = (v != 0).to(torch.int32)
        if v.dim() != 1 or v.shape[0] != n:
            raise ValueError(f'valid must hold one flag per row ({n}), got {tuple(v.shape)}')
        if n > 1 and v.stride(0) < 1:
            v = v.contiguous()
        p_valid, ld_valid = v.data_ptr(), max(int(v.stride(0)), 1)
    scale = torch.full((F,), float('nan'), dtype=torch.float64, device=dev)
    center = torch.full((F,), float('nan'), dtype=torch.float64, device=dev) if with_centering else None
    info = torch.empty(2, dtype=torch.int32, device=dev)
    q_lo, q_hi = (float(q) for q in quantile_range)
    rc = nat.load().dsp_robust_scale_fit_batch(x.data_ptr(), x.stride(0), n, F, p_valid, ld_valid, q_lo, q_hi, int(bool(with_centering)),
                                               scale.data_ptr(), None if center is None else center.data_ptr(), info.data_ptr(),
                                               _stream(dev))
    nat.check_value(rc, 'invalid argument')
    if not on_device:
        count, status = (int(v) for v in info.cpu().numpy())
        if status != 0:
            raise ValueError('no valid row to fit the scaler on' if status == 1 else 'a valid row holds a non-finite value')
        out = (None if center is None else center.cpu().numpy(), scale.cpu().numpy())
    else:
        out = (center, scale)
    return out + (info,) if return_info else out


def scaled_variance(X, scale=None, center=None, mask=None):
    """np.var over every entry of the rows of ``(X - center) / scale`` that ``mask`` keeps (``dsp_var_all``) -> a device
    tensor [2] fp64: the variance and the number of entries.  Everything on the device, nothing synchronised."""
    import torch
    x, _ = _matrix(X)
    dev, (n, F) = x.device, x.shape
    sc, ce = _vector(scale, F, dev, 'scale'), _vector(center, F, dev, 'center')
    m = None
    if mask is not None:
        m = mask if _is_device_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0)).to(dev)
        m = (m != 0).to(torch.int8).contiguous()
        if m.dim() != 1 or m.shape[0] != n:
            raise ValueError(f'mask must hold one flag per row ({n})')
    out = torch.empty(2, dtype=torch.float64, device=dev)
    rc = nat.load().dsp_var_all(x.data_ptr(), x.stride(0), n, F, None if ce is None else ce.data_ptr(), None if sc is None else sc.data_ptr(),
                                None if m is None else m.data_ptr(), out.data_ptr(), _stream(dev))
    nat.check_value(rc, 'invalid argument')
    return out


def _per_problem(v, P, dev, name):
    import torch
    if _is_device_tensor(v):
        t = v.to(torch.float64).reshape(-1)
    else:
        a = np.asarray(v, dtype=np.float64).reshape(-1)
        if not (np.isfinite(a).all() and (a > 0).all()):
            raise ValueError(f'{name} must be finite and positive, got {a.tolist()[:8]}')
        t = torch.from_numpy(a).to(dev)
    if t.shape[0] == 1 and P > 1:
        t = t.expand(P)
    if t.shape[0] != P:
        raise ValueError(f'{name} must hold one value per problem ({P}), got {t.shape[0]}')
    return t.contiguous()


def default_max_iter(n):
    return max(10000, 100 * int(n))


def svm_fit_problems(X, Y, C, gamma, tol=1e-3, max_iter=None, scale=None, center=None):
    """P two-class RBF C-SVC fits over one matrix, one launch (``dsp_svm_fit_batch``).

    ``X`` [n, F] fp64 (device tensor or host array), scaled inside the launch by ``(X - center) / scale`` (device tensors or
    host arrays [F], None = 0 / 1).  ``Y`` [P, n] (or [n]) int8, values -1 / 0 / +1, 0 = the row is not in the problem.  ``C``,
    ``gamma``: a number, P numbers or a device tensor [P] (a value that is not finite and positive gives status 4 there; host
    values raise ValueError).  ``max_iter=None`` means max(10 000, 100 n).  Returns a namespace of DEVICE tensors -- coef
    [P, n] fp64 (y alpha, exact zeros elsewhere), rho [P], n_iter, status, n_sv, n_bounded, n_active [P] int32 (views of
    ``info`` [P, 5]) -- and nothing is synchronised.  status: 0 converged, 1 max_iter reached (solution so far), 2 non-finite
    input, 3 fewer than one row in either class, 4 bad C / gamma; with 2 .. 4 the row of coef and rho are left as allocated
    (NaN)."""
    import torch
    x, _ = _matrix(X)
    dev, (n, F) = x.device, x.shape
    if n < 2:
        raise ValueError('a fit needs at least two rows')
    y = Y if _is_device_tensor(Y) else torch.from_numpy(np.ascontiguousarray(np.asarray(Y).astype(np.int8))).to(dev)
    if y.dtype != torch.int8:
        y = y.to(torch.int8)
    if y.dim() == 1:
        y = y.reshape(1, -1)
    if y.dim() != 2 or y.shape[1] != n:
        raise ValueError(f'Y must be [P, {n}], got {tuple(y.shape)}')
    if y.stride(1) != 1 or (y.shape[0] > 1 and y.stride(0) < n):
        y = y.contiguous()
    P = y.shape[0]
    if not 1 <= P <= MAX_PROBLEMS:
        raise ValueError(f'P = {P} problems: 1 .. {MAX_PROBLEMS} are served')
    d_C, d_gamma = _per_problem(C, P, dev, 'C'), _per_problem(gamma, P, dev, 'gamma')
    sc, ce = _vector(scale, F, dev, 'scale'), _vector(center, F, dev, 'center')
    max_iter = default_max_iter(n) if max_iter is None else int(max_iter)
    lib = nat.load()
    need = nat.c_i64(0)
    nat.check_value(lib.dsp_svm_fit_workspace_bytes(n, F, P, nat.C.byref(need)), 'invalid sizes')
    work = torch.empty(need.value + 16, dtype=torch.uint8, device=dev)
    coef = torch.full((P, n), float('nan'), dtype=torch.float64, device=dev)
    rho = torch.full((P,), float('nan'), dtype=torch.float64, device=dev)
    info = torch.empty((P, 5), dtype=torch.int32, device=dev)
    p_work = (work.data_ptr() + 15) // 16 * 16
    rc = lib.dsp_svm_fit_batch(x.data_ptr(), x.stride(0), n, F, None if ce is None else ce.data_ptr(), None if sc is None else sc.data_ptr(),
                               y.data_ptr(), y.stride(0) if P > 1 else n, P, d_C.data_ptr(), d_gamma.data_ptr(), float(tol), max_iter,
                               coef.data_ptr(), n, rho.data_ptr(), info.data_ptr(), p_work, need.value, _stream(dev))
    nat.check_value(rc, 'invalid argument')
    return types.SimpleNamespace(coef=coef, rho=rho, info=info, n_iter=info[:, 0], status=info[:, 1], n_sv=info[:, 2],
                                 n_bounded=info[:, 3], n_active=info[:, 4], C=d_C, gamma=d_gamma, max_iter=max_iter, tol=float(tol),
                                 _hold=(x, y, sc, ce, work))


def _labels_tensor(y, n, dev):
    import torch
    t = y if _is_device_tensor(y) else torch.from_numpy(np.ascontiguousarray(np.asarray(y).astype(np.int64).reshape(-1))).to(dev)
    t = t.reshape(-1).to(torch.int64)
    if t.shape[0] != n:
        raise ValueError(f'{t.shape[0]} labels for {n} rows')
    return t


def _classes_of(y, classes):
    """The two class labels in ascending order (SVC.classes_).  ``classes=None`` reads them from ``y`` (for labels on the
    device that is a synchronisation of its own)."""
    if classes is None:
        classes = np.unique(y.cpu().numpy() if _is_device_tensor(y) else np.asarray(y))
    cls = sorted(int(c) for c in np.asarray(classes).reshape(-1))
    if len(cls) != 2 or cls[0] == cls[1]:
        raise ValueError(f'a two-class fit needs two distinct labels, got {cls}')
    return cls


def _problem_row(y_t, cls, valid, dev):
    """-> int8 [n]: +1 for classes[1], -1 for classes[0], 0 for every other label (the `label not in self.label` filter of
    pitch_model.py:36) and every invalid row."""
    import torch
    row = (y_t == cls[1]).to(torch.int8) - (y_t == cls[0]).to(torch.int8)
    if valid is not None:
        v = valid if _is_device_tensor(valid) else torch.from_numpy(np.ascontiguousarray(np.asarray(valid) != 0)).to(dev)
        row = row * (v.reshape(-1) != 0).to(torch.int8)
    return row


def _resolve_gamma(gamma, x, F, scale, center, row):
    """'scale' -> 1 / (F var) of the scaled rows of the problem (1 where the variance is 0), 'auto' -> 1 / F, a number ->
    itself; 'scale' stays a device tensor."""
    import torch
    if isinstance(gamma, str):
        if gamma == 'auto':
            return 1.0 / F
        if gamma != 'scale':
            raise ValueError(f"gamma must be 'scale', 'auto' or a number, got {gamma!r}")
        var = scaled_variance(x, scale, center, row)[0:1]
        return torch.where(var != 0, 1.0 / (F * var), torch.ones_like(var))
    return float(gamma)


def _assemble(X_host, coef, rho, gamma, cls, scale, center):
    """The arrays of one solved problem -> (PitchSVM, support indices): support vectors in scikit-learn's order (classes[0]
    rows first, each class in row order), scaled on the host by the same true division the kernels use."""
    neg, pos = np.flatnonzero(coef < 0), np.flatnonzero(coef > 0)
    support = np.concatenate([neg, pos])
    sv = X_host[support]
    if center is not None:
        sv = sv - center
    if scale is not None:
        sv = sv / scale
    return PitchSVM(sv, coef[support], -float(rho), float(gamma), cls, scale=scale, center=center), support


def _raise_or_warn(status, n_iter, max_iter, what='the fit'):
    if status in _STATUS_TEXT:
        raise ValueError(f'{what}: {_STATUS_TEXT[status]} (status {status})')
    if status == STATUS_MAX_ITER:
        warnings.warn(f'{what} stopped at max_iter = {max_iter} before reaching the tolerance; the model holds the solution so far',
                      SvmConvergenceWarning, stacklevel=3)


def fit_pitch_svm(X, y, classes=None, C=1.0, gamma='scale', tol=1e-3, max_iter=None, with_centering=False,
                  quantile_range=(25.0, 75.0), valid=None, scaler=True):
    """pitch_model.py:48-50 -- ``scaler.fit(X); X = scaler.transform(X); clf.fit(X, y)`` -- on the device -> a ``PitchSVM``.

    ``X`` [n, F] fp64 and ``y`` [n] integer labels, device tensors (e.g. the ``feat`` of ``pitch_features_device``) or host
    arrays; ``valid``: one flag per row (``aux[:, 8]``) or None.  Rows whose label is not in ``classes`` are ignored, as the
    `label not in self.label` filter of pitch_model.py:36 ignores them; ``classes=None`` takes the two labels found in ``y``.
    ``scaler=False`` fits the SVM on the rows as they are.  gamma: 'scale' = 1 / (F var(scaled rows)) as SVC's default,
    'auto' = 1 / F, or a number.  The model is scikit-learn's layout: support vectors of ``classes[0]`` first, each class in
    row order, ``intercept = -rho``, ``decision > 0 -> classes[1]``.  ``fit_info`` on the result holds n_iter, status, n_sv,
    n_bounded, n_active, gamma and the support rows.

    Three launches (scaler, variance, solver) and then ONE download -- every result packed into one buffer, one transfer --
    that builds the arrays: that one synchronisation per fit is by design -- a ``PitchSVM`` is a host object that owns its tables.  Status 1 (``max_iter`` reached) warns with
    ``SvmConvergenceWarning`` and returns the solution so far; status 2 (a non-finite row), 3 (fewer than one row in either
    class) and 4 raise ValueError."""
    import torch
    x, on_device = _matrix(X)
    dev, (n, F) = x.device, x.shape
    y_t = _labels_tensor(y, n, dev)
    cls = _classes_of(y, classes)
    row = _problem_row(y_t, cls, valid, dev)
    center = scale = None
    if scaler:
        center, scale = robust_scale_fit(x, row.to(torch.int32), with_centering, quantile_range)
    g = _resolve_gamma(gamma, x, F, scale, center, row)
    r = svm_fit_problems(x, row, C, g, tol=tol, max_iter=max_iter, scale=scale, center=center)
    # the one download: coefficients, rho, info (int32 is exact in fp64), gamma, C, the scaler -- and the rows, if they were
    # not the host's already -- packed into ONE fp64 buffer, one transfer, one synchronisation
    parts = [r.coef[0], r.rho, r.info[0].to(torch.float64), r.gamma, r.C]
    parts += [t for t in (scale, center) if t is not None]
    if on_device:
        parts.append(x.reshape(-1))
    host = torch.cat(parts).cpu().numpy()
    coef, rho, info, gamma_v, C_v = host[:n].copy(), float(host[n]), host[n + 1:n + 6], float(host[n + 6]), float(host[n + 7])
    at = n + 8
    scale_h = center_h = None
    if scale is not None:
        scale_h, at = host[at:at + F].copy(), at + F
    if center is not None:
        center_h, at = host[at:at + F].copy(), at + F
    n_iter, status, n_sv, n_bounded, n_active = (int(v) for v in info)
    _raise_or_warn(status, n_iter, r.max_iter)
    X_host = host[at:].reshape(n, F) if on_device else np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    svm, support = _assemble(X_host, coef, rho, gamma_v, cls, scale_h, center_h)
    svm.fit_info = dict(n_iter=n_iter, status=status, n_sv=n_sv, n_bounded=n_bounded, n_active=n_active, gamma=gamma_v, rho=rho,
                        support=support, C=C_v, tol=r.tol, max_iter=r.max_iter)
    return svm


def stratified_folds(row, n_folds):
    """Fold numbers for the rows of a problem (host int8 row of -1 / 0 / +1): each class dealt round-robin in row order; -1
    for rows outside the problem."""
    row = np.asarray(row)
    out = np.full(len(row), -1, dtype=np.int64)
    for s in (-1, 1):
        idx = np.flatnonzero(row == s)
        out[idx] = np.arange(len(idx)) % n_folds
    return out


def grid_search(X, y, Cs, gammas, n_folds=5, fold_ids=None, classes=None, tol=1e-3, max_iter=None, with_centering=False,
                quantile_range=(25.0, 75.0), valid=None, scaler=True):
    """Cross-validated choice of (C, gamma): all ``len(Cs) * len(gammas) * n_folds`` training problems go in ONE
    ``dsp_svm_fit_batch`` launch -- a fold is the full problem with its held-out rows set to 0.

    The scaler is fitted once on all rows of the problem, as the reference fits it once (pitch_model.py:48).  ``gammas``:
    numbers (or 'scale' / 'auto', resolved on all rows of the problem).  ``fold_ids``: one fold number in [0, n_folds) per
    row, or None for ``stratified_folds``.  Held-out rows are scored with ``dsp_svm_decision_batch`` on each fold's model
    (the arithmetic ``PitchSVM.predict`` uses), so an entry equals what single ``fit_pitch_svm`` calls on the same folds give.
    Returns a namespace: ``accuracy`` [len(Cs), len(gammas)] (the mean of the folds' accuracies), ``fold_accuracy``
    [len(Cs), len(gammas), n_folds], ``status`` of every problem in that shape, ``best`` = (C, gamma) of the first largest
    entry, ``model`` = ``fit_pitch_svm`` refitted on all rows with it, ``fold_ids``.  A fold that fails (status 2 .. 4) raises
    ValueError, one that reaches ``max_iter`` warns.

    Cost: training is one launch, SCORING IS NOT: after one download of all coefficients, every one of the P problems builds a
    host ``PitchSVM``, uploads its tables (a blocking copy), launches ``dsp_svm_decision_batch`` once and downloads its
    predictions -- P synchronising round trips, then the refit.  Fine for the tens of problems of a pitch model's grid; a
    grid of thousands wants a scoring kernel over the coefficient matrix, which this module does not have."""
    import torch
    x, on_device = _matrix(X)
    dev, (n, F) = x.device, x.shape
    y_t = _labels_tensor(y, n, dev)
    cls = _classes_of(y, classes)
    row = _problem_row(y_t, cls, valid, dev)
    center = scale = None
    if scaler:
        center, scale = robust_scale_fit(x, row.to(torch.int32), with_centering, quantile_range)
    row_h = row.cpu().numpy()
    folds = stratified_folds(row_h, n_folds) if fold_ids is None else np.asarray(fold_ids, dtype=np.int64).reshape(-1)
    if len(folds) != n or (folds[row_h != 0] < 0).any() or (folds >= n_folds).any():
        raise ValueError(f'fold_ids must hold one fold number in [0, {n_folds}) per row')
    Cs = [float(c) for c in Cs]
    g_res = [_resolve_gamma(g, x, F, scale, center, row) for g in gammas]
    g_vals = [float(g.cpu().numpy()[0]) if _is_device_tensor(g) else float(g) for g in g_res]
    nC, nG, K = len(Cs), len(g_vals), int(n_folds)
    Y = np.repeat(row_h[None, :], nC * nG * K, axis=0).reshape(nC, nG, K, n)
    for k in range(K):
        Y[:, :, k, folds == k] = 0
    r = svm_fit_problems(x, Y.reshape(-1, n), np.repeat(Cs, nG * K), np.tile(np.repeat(g_vals, K), nC), tol=tol, max_iter=max_iter,
                         scale=scale, center=center)
    coef, rho, info = r.coef.cpu().numpy(), r.rho.cpu().numpy(), r.info.cpu().numpy()
    scale_h = None if scale is None else scale.cpu().numpy()
    center_h = None if center is None else center.cpu().numpy()
    X_host = x.cpu().numpy() if on_device else np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    truth = np.where(row_h > 0, cls[1], cls[0])
    fold_acc = np.zeros((nC, nG, K))
    for p in range(nC * nG * K):
        a, b, k = np.unravel_index(p, (nC, nG, K))
        _raise_or_warn(int(info[p, 1]), int(info[p, 0]), r.max_iter, what=f'fold {k} at C = {Cs[a]}, gamma = {g_vals[b]}')
        svm, _ = _assemble(X_host, coef[p], rho[p], g_vals[b], cls, scale_h, center_h)
        held = np.flatnonzero((folds == k) & (row_h != 0))
        pred = svm.predict(x[torch.from_numpy(held).to(dev)]).cpu().numpy()
        fold_acc[a, b, k] = float(np.mean(pred == truth[held])) if len(held) else 0.0
    acc = fold_acc.mean(axis=2)
    a, b = np.unravel_index(int(np.argmax(acc)), acc.shape)
    model = fit_pitch_svm(x, y_t, classes=cls, C=Cs[a], gamma=g_vals[b], tol=tol, max_iter=max_iter, with_centering=with_centering,
                          quantile_range=quantile_range, valid=valid, scaler=scaler)
    return types.SimpleNamespace(accuracy=acc, fold_accuracy=fold_acc, status=info[:, 1].reshape(nC, nG, K), best=(Cs[a], g_vals[b]),
                                 model=model, fold_ids=folds, Cs=Cs, gammas=g_vals)


class PitchModelTrainer:
    """pitch_model.PitchModel.train (pitch_model.py:26-50) for batches of raw clips, device-resident.

    ``add_batch`` takes clips and their labels through ``EnsembleBatch.pitch_rows`` -- endpointing,
    ``dsp_trim_preemph_batch`` (pitch_model.py:38-39), ``pitch_features_device`` (pitch_model.py:41): the launches the
    ensemble's own tail makes -- on torch's current stream without a synchronisation and keeps ``feat`` [B, 5] fp64, ``valid`` [B]
    int32 and the labels on the device; ``fit()`` is ``fit_pitch_svm`` on the accumulated rows.  Clips whose label is not in
    ``labels`` stay in the rows and are ignored by the fit (pitch_model.py:36); clips the reference's ``pitch_feature`` raises
    on are invalid rows and are ignored too."""

    def __init__(self, labels, rate, frame=0.03, step=0.01, coeff=0.97, **fit_kwargs):
        from .ensemble import EnsembleBatch
        self.labels = tuple(int(v) for v in labels)
        if len(self.labels) != 2:
            raise ValueError(f'a pitch model separates two labels, got {self.labels}')
        self.rate, self.fit_kwargs = rate, dict(fit_kwargs)
        self._eb = EnsembleBatch(rate, None, [], frame=frame, step=step, coeff=coeff)     # for pitch_rows alone: no head, no rules
        self._feat, self._valid, self._y = [], [], []

    def add_batch(self, waves, sample_offsets, labels):
        """``waves``: concatenated clips (host array or device tensor, int16 / float32), ``sample_offsets`` [B + 1],
        ``labels`` [B] (host or device).  -> (feat, valid) of this batch, device tensors."""
        feat, valid = self._eb.pitch_rows(waves, sample_offsets)
        self._feat.append(feat)
        self._valid.append(valid)
        self._y.append(_labels_tensor(labels, feat.shape[0], feat.device))
        return feat, valid

    def rows(self):
        """-> (feat [n, 5] fp64, valid [n] int32, labels [n] int64): everything accumulated so far, device tensors."""
        import torch
        if not self._feat:
            raise ValueError('no batch was added')
        return torch.cat(self._feat), torch.cat(self._valid), torch.cat(self._y)

    def fit(self, **overrides):
        """``fit_pitch_svm`` on the accumulated rows with the labels of this trainer -> a ``PitchSVM``.  An invalid row holds
        NaN features; ``valid`` keeps it out of the scaler, the variance and the fit, and no kernel looks at it."""
        feat, valid, y = self.rows()
        kw = dict(self.fit_kwargs)
        kw.update(overrides)
        return fit_pitch_svm(feat, y, classes=self.labels, valid=valid, **kw)
