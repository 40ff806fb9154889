"""Shared by tests/test_bigru_golden.py (CPU) and tests/test_gpu_bigru.py: the fixture of the bidirectional GRU encoder
(tests/golden/make_bigru_golden.py -> tests/golden/bigru_golden.npz), its inputs, and the comparison against it."""
import importlib.util
import os

import numpy as np

from hmrnn_cases import BAR, scale      # noqa: F401  (2e-5 x max(1, absmax): a native fp32 recurrence against the CPU reference)

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_BAR = 2e-4           # the bar of the heads on ROCm (tests/test_classifier_golden.py)
TAGS = ('a', 'b', 'c')


def maker():
    spec = importlib.util.spec_from_file_location('_make_bigru_golden', os.path.join(HERE, 'golden', 'make_bigru_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_golden():
    with np.load(os.path.join(HERE, 'golden', 'bigru_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def encoder(g, tag):
    """features.classifier._DynEnc with the fixture's seeded parameters (eval mode, CPU)."""
    import torch
    from features.classifier import _DynEnc, fill_parameters
    I, H, L = (int(v) for v in g[tag + '_shape'])
    torch.manual_seed(0)
    enc = _DynEnc(I, H, L).eval()
    assert fill_parameters(enc, int(g[tag + '_seed'])) == [str(n) for n in g[tag + '_names']]
    return enc


def deviation(g, tag, y, hn):
    """Worst deviation of (y [T, B, H], h_n) from the fixture, each divided by max(1, absmax) of its reference; the all-row sum
    is held to the bar times the number of rows, so its deviation is divided by that number as well."""
    y, hn = np.asarray(y), np.asarray(hn)
    rows, want = g[tag + '_rows'], g[tag + '_out']
    assert y.shape[0] == int(maker().inputs(tag, np)[1].max()) and y.shape[1:] == want.shape[1:] and hn.shape == g[tag + '_hidden'].shape
    d_rows = float(np.max(np.abs(y[rows] - want))) / scale(want)
    d_sum = float(np.max(np.abs(y.astype(np.float64).sum(0) - g[tag + '_sum']))) / (y.shape[0] * scale(want))
    d_hn = float(np.max(np.abs(hn - g[tag + '_hidden']))) / scale(g[tag + '_hidden'])
    return max(d_rows, d_sum, d_hn)
