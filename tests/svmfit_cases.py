"""Cases of the device-side fit (features/svmfit.py): seeded generators only.  tests/golden/make_svmfit_golden.py fits the
real scikit-learn RobustScaler + SVC on them and stores only scikit-learn's results (tests/golden/svmfit_golden.npz); the
training rows and the queries are regenerated here.  The shapes are the smallest at which each mechanism can break:

  pair01 / pair67 at C = 1, 0.01 (every alpha at its bound: rho from the midpoint) and 100 (many free alpha)
  n2 (one iteration), n3, dup65 (ten duplicated rows of opposite label: the curvature floor; one row past a wavefront)
  f1_1025 (F = 1, more than one row per thread), f16_300 (F = 16, C = 10, gamma='auto'), n2500 (several rows per thread, a
  few thousand iterations), quant (a quantised feature with zero inter-quartile range: scale 1), center
  (with_centering=True), q1090 (quantile pair 10 / 90, a given gamma)
each at tol 1e-3 (the reference's) and 1e-6.
"""
import numpy as np

from ensemble_cases import svm_queries, svm_training_set

TOLS = (1e-3, 1e-6)
MAX_ITER = 200000


def _blobs(seed, n, F, sep=1.0):
    """Two overlapping classes of F columns at different scales per column -> (X, y in {0, 1})."""
    rng = np.random.default_rng(seed)
    col = 10.0 ** rng.uniform(-2, 1, F)
    mean = rng.standard_normal((2, F)) * sep
    y = rng.integers(0, 2, n)
    y[:2] = (0, 1)                                          # both classes, whatever n
    return (mean[y] + rng.standard_normal((n, F))) * col, y


def _gen(seed, n, F, labels=(0, 1), nq=256, sep=1.0):
    X, y = _blobs(seed, n, F, sep)
    Q, _ = _blobs(seed, nq + n, F, sep)                     # the same mixture (same column scales and means), later rows
    return X, np.array(labels)[y], Q[n:]


def _pair(k):
    X, y = svm_training_set(k)
    return X, y, svm_queries(k)


def _dup65():
    X, y, Q = _gen(65, 65, 5, labels=(6, 7))
    X[55:] = X[:10]
    y[55:] = np.where(y[:10] == 6, 7, 6)
    return X, y, Q


def _quant():
    X, y, Q = _gen(77, 200, 5)
    for A in (X, Q):
        A[:, 2] = np.round(A[:, 2] / np.abs(X[:, 2]).max() * 0.6)     # most rows 0, a few -1 / +1: the quartiles coincide
    return X, y, Q


# name -> (generator, SVC / RobustScaler arguments)
CASES = {
    'pair01_c1': (lambda: _pair(0), dict(C=1.0)),
    'pair01_c001': (lambda: _pair(0), dict(C=0.01)),
    'pair01_c100': (lambda: _pair(0), dict(C=100.0)),
    'pair67_c1': (lambda: _pair(1), dict(C=1.0)),
    'pair67_c001': (lambda: _pair(1), dict(C=0.01)),
    'pair67_c100': (lambda: _pair(1), dict(C=100.0)),
    'n2': (lambda: _gen(2, 2, 5, sep=2.0), dict(C=1.0)),
    'n3': (lambda: _gen(3, 3, 5, sep=2.0), dict(C=1.0)),
    'dup65': (_dup65, dict(C=1.0)),
    'f1_1025': (lambda: _gen(1025, 1025, 1, sep=2.5), dict(C=1.0)),
    'f16_300': (lambda: _gen(300, 300, 16, sep=0.5), dict(C=10.0, gamma='auto')),
    'n2500': (lambda: _gen(2500, 2500, 5), dict(C=1.0)),
    'quant': (_quant, dict(C=1.0)),
    'center': (lambda: _gen(91, 150, 5), dict(C=1.0, with_centering=True)),
    'q1090': (lambda: _gen(92, 151, 3), dict(C=2.0, gamma=0.3, quantile_range=(10.0, 90.0))),
}


def case(name):
    """-> (X [n, F], y [n] labels, Q [nq, F], dict(C, gamma, with_centering, quantile_range))."""
    gen, kw = CASES[name]
    X, y, Q = gen()
    args = dict(C=1.0, gamma='scale', with_centering=False, quantile_range=(25.0, 75.0))
    args.update(kw)
    return np.ascontiguousarray(X), np.asarray(y), np.ascontiguousarray(Q), args


def key(name, tol):
    return f'{name}/tol{tol:g}'
