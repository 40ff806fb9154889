#!/usr/bin/env python3
"""Times the device-side fit of the pitch model (features/svmfit.py; csrc/kernels_svmfit.h), device events around each call,
median and spread of --repeats calls after a warm-up:

  (a) one fit (F = 5, C = 1, gamma = 1 / (F var), tol 1e-3) at n = 400 / 1500 / 8192: time, iterations, microseconds per
      iteration;
  (b) batches of P = 1 / 25 / 125 / 256 / 512 problems at n = 400 (the same rows, C and gamma spread over a grid): time per
      launch -- where the compute units fill;
  (c) the scaler fit alone at the three sizes;
  (d) scikit-learn's RobustScaler + SVC on the same rows on this machine's host, if scikit-learn imports here; if it does
      not, that is said and no ratio is given.

Rows are the two-class mixture of tests/ensemble_cases.py at the size asked for.  Prints one JSON line.

    python tools/kbench_svmfit.py [--repeats 3] [--profile]      # --profile: one pass of each shape, no timing (for a tracer)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def rows(n, seed=5):
    from ensemble_cases import N_FEAT, _MEAN, _STD
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 2, n)
    return _MEAN[y] + _STD * rng.standard_normal((n, N_FEAT)), y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    import torch
    from features import _native as nat
    from features import svmfit
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())

    def timed(fn):
        """-> (median ms, [all ms]) of device events around fn(), after one warm call."""
        fn()
        torch.cuda.synchronize(dev)
        if args.profile:
            return 0.0, []
        out = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize(dev)
            out.append(a.elapsed_time(b))
        return float(np.median(out)), [round(t, 4) for t in out]

    res = dict(repeats=args.repeats, single=[], batch=[], scaler=[], sklearn=None)
    sets = {}
    for n in (400, 1500, 8192):
        X, y = rows(n)
        d_X = torch.from_numpy(X).to(dev)
        yrow = torch.from_numpy(np.where(y == 1, 1, -1).astype(np.int8)).to(dev)
        _, scale = svmfit.robust_scale_fit(d_X)
        var = svmfit.scaled_variance(d_X, scale)[0:1]
        gamma = 1.0 / (5 * var)
        sets[n] = (X, y, d_X, yrow, scale, gamma)
        ms, all_ms = timed(lambda: svmfit.robust_scale_fit(d_X))
        res['scaler'].append(dict(n=n, ms_median=ms, ms_all=all_ms))
        hold = {}

        def fit():
            hold['r'] = svmfit.svm_fit_problems(d_X, yrow, 1.0, gamma, tol=1e-3, max_iter=200000, scale=scale)
        ms, all_ms = timed(fit)
        n_iter, status, n_sv = (int(v) for v in hold['r'].info[0, :3].cpu().numpy())
        res['single'].append(dict(n=n, ms_median=ms, ms_all=all_ms, n_iter=n_iter, status=status, n_sv=n_sv,
                                  us_per_iter=1e3 * ms / max(n_iter, 1), gamma=float(gamma.cpu().numpy()[0])))
    X, y, d_X, yrow, scale, gamma = sets[400]
    g0 = float(gamma.cpu().numpy()[0])
    for P in (1, 25, 125, 256, 512):
        Cs = np.resize(np.array([0.1, 0.3, 1.0, 3.0, 10.0]), P)
        gs = np.resize(np.repeat(g0 * np.array([0.25, 0.5, 1.0, 2.0, 4.0]), 5), P)
        Y = yrow.reshape(1, -1).expand(P, -1).contiguous()
        d_C, d_g = torch.from_numpy(Cs).to(dev), torch.from_numpy(gs).to(dev)
        hold = {}

        def fit():
            hold['r'] = svmfit.svm_fit_problems(d_X, Y, d_C, d_g, tol=1e-3, max_iter=200000, scale=scale)
        ms, all_ms = timed(fit)
        it = hold['r'].n_iter.cpu().numpy()
        res['batch'].append(dict(P=P, n=400, ms_median=ms, ms_all=all_ms, iter_sum=int(it.sum()), iter_max=int(it.max()),
                                 status_max=int(hold['r'].status.max().cpu())))
    try:
        import sklearn
        from sklearn.preprocessing import RobustScaler
        from sklearn.svm import SVC
    except Exception as e:                                          # not installed on this machine: no host figure, no ratio
        res['sklearn'] = f'not importable here ({type(e).__name__}): no host figure, no ratio'
    else:
        res['sklearn'] = dict(version=sklearn.__version__, fits=[])
        for n in (400, 1500, 8192):
            X, y = sets[n][:2]
            out = []
            for _ in range(args.repeats + 1):
                t0 = time.perf_counter()
                sc = RobustScaler(with_centering=False).fit(X)
                t1 = time.perf_counter()
                clf = SVC(kernel='rbf').fit(sc.transform(X), y)
                out.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
            out = out[1:]
            res['sklearn']['fits'].append(dict(n=n, scaler_ms_median=float(np.median([o[0] for o in out])),
                                               svc_ms_median=float(np.median([o[1] for o in out])),
                                               svc_ms_all=[round(o[1], 3) for o in out], n_iter=int(np.asarray(clf.n_iter_).reshape(-1)[0])))
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(main())
