"""NumPy restatement of csrc/kernels_loss.h (include/dsp_frontend.h: dsp_xent_metrics_batch) in fp64 / int64: the loss, its
gradient, the prediction and the epoch state field by field.  The yardstick between torch and the device: tests hold this file
to torch on the CPU, and the kernels to this file.

    out = xent(logits, labels, pred_in=None, grad_out=1.0)      # per-call values
    st = State(n_classes, wrong_capacity); st.update(logits, labels, pred_in=None); st.result()
"""
from __future__ import annotations

import types

import numpy as np

IGNORE_INDEX = -100
N_COUNTS = 8
SEEN, SCORED, CORRECT, IGNORED, BAD_LABEL, WRONG_TOTAL, CALLS, RESERVED = range(N_COUNTS)


def state_bytes(n_classes, wrong_capacity):
    """dsp_metrics_bytes: counts [8] int64 | loss_sum fp64 | confusion [C][C] int64 | wrong [cap][3] int32, padded to 8."""
    b = N_COUNTS * 8 + 8 + n_classes * n_classes * 8 + wrong_capacity * 12
    return (b + 7) // 8 * 8


def xent(logits, labels, pred_in=None, grad_out=1.0):
    """-> namespace(nll [B] fp64, loss fp64 (NaN with nothing scored), pred [B] int64, prob [B, C] fp64, dlogits [B, C] fp64,
    scored [B] bool, scored_label [B] int64, n_scored).  ``logits`` are taken as given (pass fp32 values promoted to fp64)."""
    x = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    B, C = x.shape
    mx = x.max(axis=1)
    e = np.exp(x - mx[:, None])
    s = e.sum(axis=1)
    prob = e / s[:, None]
    pred = np.argmax(x == mx[:, None], axis=1).astype(np.int64)         # the lowest index among the largest logits
    scored = (y >= 0) & (y < C)
    ys = np.where(scored, y, 0)
    nll = np.where(scored, (np.log(s) + mx) - x[np.arange(B), ys], 0.0)
    n = int(scored.sum())
    with np.errstate(invalid='ignore', divide='ignore'):
        loss = np.float64(nll[scored].sum()) / np.float64(n)
    onehot = np.zeros((B, C))
    onehot[np.arange(B), ys] = 1.0
    dlogits = np.zeros((B, C))
    if n:
        dlogits[scored] = ((prob - onehot) * np.float64(grad_out) / np.float64(n))[scored]
    sl = pred if pred_in is None else np.asarray(pred_in, dtype=np.int64)
    return types.SimpleNamespace(nll=nll, loss=loss, pred=pred, prob=prob, dlogits=dlogits, scored=scored, scored_label=sl,
                                 n_scored=n)


class State:
    """The epoch state as the device holds it."""

    def __init__(self, n_classes, wrong_capacity):
        self.C, self.cap = int(n_classes), int(wrong_capacity)
        self.reset()

    def reset(self):
        self.counts = np.zeros(N_COUNTS, dtype=np.int64)
        self.loss_sum = np.float64(0.0)
        self.confusion = np.zeros((self.C, self.C), dtype=np.int64)
        self.wrong = np.zeros((self.cap, 3), dtype=np.int32)

    def update(self, logits, labels, pred_in=None):
        o = xent(logits, labels, pred_in)
        y = np.asarray(labels, dtype=np.int64)
        B = len(y)
        seen0 = int(self.counts[SEEN])
        sc = o.scored
        sl = o.scored_label
        wrong = sc & (sl != y)
        cell = sc & (sl >= 0) & (sl < self.C)
        np.add.at(self.confusion, (y[cell], sl[cell]), 1)
        slot = int(self.counts[WRONG_TOTAL])
        for b in np.nonzero(wrong)[0]:                     # clip order; entries behind the capacity are counted only
            if slot < self.cap:
                self.wrong[slot] = (seen0 + b, sl[b], y[b])
            slot += 1
        self.counts[SEEN] += B
        self.counts[SCORED] += int(sc.sum())
        self.counts[CORRECT] += int((sc & ~wrong).sum())
        self.counts[IGNORED] += int((~sc).sum())
        self.counts[BAD_LABEL] += int((~sc & (y != IGNORE_INDEX)).sum())
        self.counts[WRONG_TOTAL] = slot
        self.counts[CALLS] += 1
        self.loss_sum = self.loss_sum + np.float64(o.nll[sc].sum())
        return o

    def result(self):
        return result_from(self.counts, self.loss_sum, self.confusion, self.wrong)


def confusion_present(confusion):
    """The matrix without the rows and columns of labels that occur neither as a true nor as a scored label: what
    ``sklearn.metrics.confusion_matrix(y, pred)`` returns without ``labels=``."""
    c = np.asarray(confusion)
    keep = (c.sum(axis=0) + c.sum(axis=1)) > 0
    return c[np.ix_(keep, keep)]


def result_from(counts, loss_sum, confusion, wrong):
    counts = np.asarray(counts, dtype=np.int64)
    scored = int(counts[SCORED])
    total = int(counts[WRONG_TOTAL])
    conf = np.array(confusion, dtype=np.int64)
    return types.SimpleNamespace(
        seen=int(counts[SEEN]), scored=scored, correct=int(counts[CORRECT]), ignored=int(counts[IGNORED]),
        bad_label=int(counts[BAD_LABEL]), wrong_total=total, calls=int(counts[CALLS]), loss_sum=float(loss_sum),
        accuracy=float(counts[CORRECT]) / scored if scored else float('nan'),
        loss=float(loss_sum) / scored if scored else float('nan'),
        confusion=conf, confusion_present=lambda: confusion_present(conf),
        wrong=np.array(wrong[:min(total, len(wrong))], dtype=np.int32).reshape(-1, 3))
