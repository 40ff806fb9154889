"""Shared by tests/test_hmrnn_golden.py (CPU) and tests/test_gpu_hmlstm.py: the fixture's inputs, and the guard rule of
the boundary threshold (tests/golden/make_hmrnn_golden.py explains it).

A decision whose reference z_hat lies within ``g`` of 0.5 may legitimately fall either way in another correct fp32
implementation.  In each batch column, bits and values are compared up to the first step that holds such a decision; from
there on the column's recurrent outputs are left out.  ``cut[b]`` is that step (T when the column has none)."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 1e-5          # tests/golden/hmrnn_golden.npz was generated with this guard (stored there as `guard`)
BAR = 2e-5            # the CPU bar of tests/test_classifier_golden.py: BAR * max(1, absmax)


def maker():
    spec = importlib.util.spec_from_file_location('_make_hmrnn_golden', os.path.join(HERE, 'golden', 'make_hmrnn_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_golden():
    with np.load(os.path.join(HERE, 'golden', 'hmrnn_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def cuts(z_hat_ref, g=GUARD):
    """z_hat_ref [T, 2, B] -> cut [B]: the first step with a decision inside the guard, T if there is none."""
    inside = (np.abs(np.asarray(z_hat_ref, dtype=np.float64) - 0.5) < g).any(axis=1)          # [T, B]
    T = inside.shape[0]
    return np.where(inside.any(axis=0), inside.argmax(axis=0), T)


def left_out_share(cut, T):
    return float(np.sum(T - cut)) / float(T * len(cut))


def scale(a):
    return max(1.0, float(np.max(np.abs(a)))) if np.size(a) else 1.0


def worst_before_cut(got_bt, ref_bt, cut, steps=None):
    """max |got - ref| over the rows [b, t] with t < cut[b].  got / ref: [B, T', ...]; steps: the step of each of the T' rows
    (all T when None)."""
    got_bt, ref_bt = np.asarray(got_bt, dtype=np.float64), np.asarray(ref_bt, dtype=np.float64)
    steps = np.arange(ref_bt.shape[1]) if steps is None else np.asarray(steps)
    keep = steps[None, :] < np.asarray(cut)[:, None]                                          # [B, T']
    d = np.abs(got_bt - ref_bt)
    d = d.reshape(d.shape[0], d.shape[1], -1).max(axis=2) if d.ndim > 2 else d
    return float(np.max(np.where(keep, d, 0.0))) if d.size else 0.0


def bits_equal_before_cut(got_bt, ref_bt, cut):
    got_bt, ref_bt = np.asarray(got_bt).reshape(np.asarray(ref_bt).shape[0], -1), np.asarray(ref_bt).reshape(np.asarray(ref_bt).shape[0], -1)
    keep = np.arange(ref_bt.shape[1])[None, :] < np.asarray(cut)[:, None]
    return bool(np.all((got_bt != 0)[keep] == (ref_bt != 0)[keep]))
