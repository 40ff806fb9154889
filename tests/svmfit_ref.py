"""What the tests of the device-side fit share (tests/test_svmfit_host.py, tests/test_gpu_svmfit.py): the conditions a solution
must meet whatever produced it, recomputed on the host in fp64 from the returned coefficients with a FRESH gradient
(tools/svm_fit_emul.py: kkt, calculate_rho).

The drift term: the solver updates its gradient incrementally, two fused products per update, each rounded to 2^-53 relative
of the running magnitude, so after n_iter updates the gradient it stopped on differs from a fresh one by at most
4 n_iter 2^-53 (1 + max |G|).  The KKT gap of the fresh gradient may exceed tol by that much, and rho -- a mean or a midpoint
of gradient entries -- moves by no more.  The equality constraint: every update keeps y' alpha up to one rounding of values
below C, and so does the clipping: |sum y alpha| <= 4 (n_iter + n) C 2^-53."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

import svm_fit_emul as emul  # noqa: E402

U = 2.0 ** -53


def check_conditions(Xs, yrow, coef, rho, n_iter, n_sv, n_bounded, C, gamma, tol, check_gap=True):
    """The conditions that need no reference (shared with tests/test_gpu_svmfit.py): recomputed in fp64 from the returned
    coefficients with a fresh gradient."""
    yrow = np.asarray(yrow)
    assert (coef[yrow == 0] == 0).all()                                            # inactive rows exactly 0
    gap, gmax, G, alpha, yy = emul.kkt(Xs, yrow, coef, C, gamma)
    assert (alpha >= 0).all() and (alpha <= C).all()                               # bound values are exact: nothing above C
    assert (np.sign(coef[yrow != 0]) * yy >= 0).all()                              # coef = y alpha
    assert abs(float((yy * alpha).sum())) <= 4 * (n_iter + len(yrow)) * C * U
    drift = 4 * n_iter * U * (1 + gmax)
    if check_gap:
        assert gap < tol + drift, (gap, tol, drift)
    want_rho, want_sv, want_bounded = emul.calculate_rho(alpha, G, yy, C)
    assert (n_sv, n_bounded) == (want_sv, want_bounded)
    # the mean over the free alpha, or the midpoint of the two bounds: each value of the kernel's own G lies within the
    # drift of the fresh one
    assert abs(rho - want_rho) <= drift, (rho, want_rho, drift)
    return gap, drift
