"""Cases of the ensemble path (features/ensemble.py): the pitch SVMs and the confidence gate.  Inputs are seeded and
generated, never stored; tests/golden/make_ensemble_golden.py fits the real scikit-learn models on them, drives the
reference's own gate loop and stores only the numbers (tests/golden/ensemble_golden.npz).

(A) two models, for the label pairs (0, 1) and (6, 7): 400 synthetic training rows of five columns at the scales
    pitch.pitch_feature produces on voiced chirps (slopes of a few tenths of a Hz per frame, quadratic terms of a few
    hundredths, a median shift of some Hz), two overlapping classes, and 512 query rows from the same mixture;
(B) fourteen int16 chirps at 16 kHz (pitch_cepstrum_cases.chirp) with designed logits [14, 20]: predictions 0 / 1 / 6 / 7
    below and above the thresholds 0.8 / 0.7 of ensemble.py:50-53, one between the two thresholds for each pair, and
    predictions outside both pairs with low and high confidence;
(C) three of those clips for the pre-emphasised trim (one whose segment starts at sample 0, two where it does not).
"""
import numpy as np

from pitch_cepstrum_cases import chirp

PAIRS = ((0, 1), (6, 7))
THRESHOLDS = (0.8, 0.7)                   # ensemble.py:50,52
MODEL_SEEDS = (11, 67)                    # kept by make_ensemble_golden.py's rule: no query with |decision| < 1e-6
N_TRAIN, N_QUERY, N_FEAT = 400, 512, 5
N_CLASSES = 20

_MEAN = np.array([[0.30, 0.30, 0.000, 0.000, 7.0], [0.45, 0.45, 0.004, -0.003, 12.0]])
_STD = np.array([0.12, 0.12, 0.012, 0.010, 3.5])


def _mixture(rng, n):
    y = rng.integers(0, 2, n)
    return _MEAN[y] + _STD * rng.standard_normal((n, N_FEAT)), y


def svm_training_set(k):
    """-> (X [400, 5] fp64, y [400] labels of PAIRS[k])."""
    X, y = _mixture(np.random.default_rng(MODEL_SEEDS[k]), N_TRAIN)
    return X, np.array(PAIRS[k])[y]


def svm_queries(k):
    """-> [512, 5] fp64: rows of the training mixture, every fourth one pushed out to three times the spread."""
    rng = np.random.default_rng(MODEL_SEEDS[k] + 1000)
    X, _ = _mixture(rng, N_QUERY)
    X[::4] += 2.0 * _STD * rng.standard_normal((len(X[::4]), N_FEAT))
    return X


RATE = 16000
# a chirp stays only if the reference's single-precision track equals its double-precision one, pitch.pitch_feature does
# not raise on it and the margins of the gate hold (make_ensemble_golden.py refuses otherwise)
CLIP_SEEDS = [301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311, 312, 313, 314]
TRIM_CLIPS = (1, 2, 5)                    # fixture (C): indices into the clips


def make_clips():
    """-> (list of int16 clips, rate)."""
    out = []
    for seed in CLIP_SEEDS:
        rng = np.random.default_rng(seed)
        out.append(chirp(rng, RATE, rng.uniform(0.5, 0.9)).astype(np.int16))
    return out, RATE


# (arg-max, its designed softmax probability) per clip
DESIGN = [(0, 0.55), (0, 0.93), (1, 0.62), (1, 0.88), (6, 0.50), (6, 0.90), (7, 0.64), (7, 0.81), (6, 0.75), (0, 0.75),
          (3, 0.40), (12, 0.97), (1, 0.30), (7, 0.65)]


def design_logits():
    """[14, 20] fp32: class k gets log(19 p / (1 - p)) over a floor of small seeded values, so softmax[k] is about p."""
    rng = np.random.default_rng(7)
    out = rng.uniform(-0.05, 0.05, (len(DESIGN), N_CLASSES))
    for b, (k, p) in enumerate(DESIGN):
        out[b, k] = np.log((N_CLASSES - 1) * p / (1 - p))
    return out.astype(np.float32)
