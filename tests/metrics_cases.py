"""Cases of the loss / metrics kernels (csrc/kernels_loss.h, tools/metrics_emul.py), seeded and generated, never stored.

Shapes (B, C): one clip; a batch that does not fill a block of four rows; more than one wave's worth of clips (and with 67 a
batch that is no multiple of the rows per block); a class count above half a wavefront and the full 64; the working size.

``make(B, C)`` -> namespace(logits fp32 [B, C], labels int64 [B], pred_in int32 [B]):
  * a seeded normal x 3;
  * row 1 (where there is one) has two equal maxima, row 2 three (C >= 3), placed at the highest indices so that "the lowest
    index among the largest" is not the first column;
  * row 3 holds +195 and -195 (the magnitude the attention tests use: exp(-390) is a normal fp64 number, nothing overflows);
  * labels are seeded; where B >= 5 every seventh from the fourth on is -100 and label 0 is out of range (C + 3), so the batch
    holds ignored clips of both kinds; small batches keep valid labels;
  * pred_in: the labels with every third one moved to the next class -- a scoring that differs from the arg-max.
"""
import types

import numpy as np

SHAPES = [(1, 2), (5, 20), (32, 20), (67, 20), (64, 35), (3, 64), (512, 20)]
IGNORE = -100
PAD = 3                                   # the row stride of the strided cases is C + PAD
CANARY32 = np.float32(np.frombuffer(np.uint32(0x7fc0beef).tobytes(), np.float32)[0])     # a quiet NaN: never a result


def make(B, C, seed=0):
    rng = np.random.default_rng(1000 * B + C + seed)
    logits = (3.0 * rng.standard_normal((B, C))).astype(np.float32)
    if B > 1:
        logits[1, C - 2:] = logits[1].max() + np.float32(1.0)
    if B > 2 and C >= 3:
        logits[2, C - 3:] = logits[2].max() + np.float32(0.5)
    if B > 3:
        logits[3, 0], logits[3, C - 1] = np.float32(195.0), np.float32(-195.0)
    labels = rng.integers(0, C, B).astype(np.int64)
    if B >= 5:
        labels[3::7] = IGNORE
        labels[0] = C + 3
    pred_in = labels.astype(np.int32)
    pred_in[::3] = (pred_in[::3] + 1) % C
    pred_in[labels < 0] = 0
    pred_in[labels >= C] = 1
    return types.SimpleNamespace(logits=logits, labels=labels, pred_in=pred_in)


def strided(logits, fill=CANARY32):
    """[B, C] -> ([B, C + PAD] buffer with canaries behind every row, the [B, C] view of it)."""
    B, C = logits.shape
    buf = np.full((B, C + PAD), fill, dtype=np.float32)
    buf[:, :C] = logits
    return buf


def n_equal_maxima(logits):
    return (logits == logits.max(axis=1, keepdims=True)).sum(axis=1)
