"""The scoring of the reference on the device (csrc/kernels_loss.h, ``dsp_xent_metrics_batch``).

* ``Metrics`` owns the epoch state -- the counters, the loss sum, the confusion matrix and the list of wrong clips that
  ``RNNModel.test`` / ``EnsembleModel.test`` collect on the host batch by batch (model.py:162-187, ensemble.py:44-64) -- as ONE
  device block.  ``update`` is a launch on torch's current stream, ``result()`` the one download of an epoch.
* ``cross_entropy`` is ``F.cross_entropy(logits, labels)`` at its defaults as an autograd function whose forward is one native
  call (loss and gradient together, the metrics too when asked) and whose backward launches nothing of its own when the
  upstream gradient is ``unit_grad`` (``backward(loss)`` passes it).

There is no fallback: without the library or a GPU every call raises.
"""
from __future__ import annotations

import types

import numpy as np

from . import _native as nat

IGNORE_INDEX = -100
MAX_UTT, MAX_CLASSES = 16384, 64
N_COUNTS = 8
_COUNT_NAMES = ('seen', 'scored', 'correct', 'ignored', 'bad_label', 'wrong_total', 'calls')


def state_bytes(n_classes, wrong_capacity):
    """``dsp_metrics_bytes``; ValueError for sizes the library refuses.  Needs no device."""
    out = nat.c_i64(0)
    nat.check_value(nat.load().dsp_metrics_bytes(int(n_classes), int(wrong_capacity), nat.C.byref(out)), 'invalid sizes')
    return out.value


def _check_logits(logits):
    import torch
    if not torch.is_tensor(logits) or logits.dtype != torch.float32:
        raise TypeError(f'logits must be a float32 tensor, got {getattr(logits, "dtype", type(logits).__name__)}')
    if logits.dim() != 2:
        raise ValueError(f'logits must be [B, C], got {tuple(logits.shape)}')
    if not logits.is_cuda:
        raise TypeError('logits must be a device tensor')


def _check_labels(labels, B, dev, what='labels', dtype=None):
    import torch
    dtype = torch.int64 if dtype is None else dtype
    if not torch.is_tensor(labels) or labels.dtype != dtype or tuple(labels.shape) != (B,) or labels.device != dev:
        raise TypeError(f'{what} must be a [{B}] {dtype} tensor on {dev}')
    return labels if labels.is_contiguous() else labels.contiguous()


def xent(logits, labels, pred_in=None, grad_out=None, want=('loss',), metrics=None):
    """One ``dsp_xent_metrics_batch`` on torch's current stream; nothing is synchronised.  ``logits`` [B, C] fp32 device tensor
    (any row stride), ``labels`` int64 [B], ``pred_in`` int32 [B] or None, ``grad_out`` fp32 [1] / 0-dim or None (= 1).
    ``want``: which of 'nll', 'loss', 'pred', 'prob', 'dlogits' to allocate and fill -> a namespace of them (loss is 0-dim);
    ``metrics``: a ``Metrics`` to update."""
    import torch
    _check_logits(logits)
    nat.require_device()
    dev = logits.device
    if logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        logits = logits.contiguous()
    B, C = logits.shape
    labels = _check_labels(labels, B, dev)
    if pred_in is not None:
        pred_in = _check_labels(pred_in, B, dev, 'pred', torch.int32)
    if grad_out is not None and not (torch.is_tensor(grad_out) and grad_out.dtype == torch.float32 and grad_out.numel() == 1
                                     and grad_out.device == dev):
        raise TypeError('grad_out must be a float32 device tensor of one element')
    if metrics is not None:
        if not isinstance(metrics, Metrics):
            raise TypeError(f'metrics must be a features.metrics.Metrics, not {type(metrics).__name__}')
        if metrics.n_classes != C or metrics.device != dev:
            raise ValueError(f'metrics is for {metrics.n_classes} classes on {metrics.device}; the logits have {C} on {dev}')
    bad = set(want) - {'nll', 'loss', 'pred', 'prob', 'dlogits'}
    if bad:
        raise ValueError(f'unknown outputs {sorted(bad)}')
    ns = types.SimpleNamespace(
        nll=torch.empty(B, dtype=torch.float32, device=dev) if 'nll' in want else None,
        loss=torch.empty((), dtype=torch.float32, device=dev) if 'loss' in want else None,
        pred=torch.empty(B, dtype=torch.int32, device=dev) if 'pred' in want else None,
        prob=torch.empty((B, C), dtype=torch.float32, device=dev) if 'prob' in want else None,
        dlogits=torch.empty((B, C), dtype=torch.float32, device=dev) if 'dlogits' in want else None)

    def ptr(t):
        return None if t is None else t.data_ptr()
    with torch.cuda.device(dev):                           # (the pointers carry no device: the launch goes to the tensors')
        rc = nat.load().dsp_xent_metrics_batch(
            logits.data_ptr(), logits.stride(0), B, C, labels.data_ptr(), ptr(pred_in), ptr(grad_out), ptr(ns.nll), ptr(ns.loss),
            ptr(ns.pred), ptr(ns.prob), ptr(ns.dlogits), C, None if metrics is None else metrics.state.data_ptr(),
            0 if metrics is None else metrics.wrong_capacity, torch.cuda.current_stream(dev).cuda_stream)
    nat.check_value(rc, 'invalid argument')
    return ns


def confusion_present(confusion):
    """The matrix without the rows and columns of labels that occur neither as a true nor as a scored label: what
    ``sklearn.metrics.confusion_matrix(y, pred)`` returns without ``labels=``."""
    c = np.asarray(confusion)
    keep = (c.sum(axis=0) + c.sum(axis=1)) > 0
    return c[np.ix_(keep, keep)]


def parse_state(words, n_classes, wrong_capacity):
    """The block as int64 words (host array) -> the namespace of ``Metrics.result``.  Needs no device."""
    a = np.ascontiguousarray(words, dtype=np.int64)
    C, cap = int(n_classes), int(wrong_capacity)
    counts = a[:N_COUNTS]
    loss_sum = float(a[N_COUNTS:N_COUNTS + 1].view(np.float64)[0])
    conf = a[N_COUNTS + 1:N_COUNTS + 1 + C * C].reshape(C, C).copy()
    wrong = a[N_COUNTS + 1 + C * C:].view(np.int32)[:3 * cap].reshape(cap, 3)
    ns = types.SimpleNamespace(**{k: int(v) for k, v in zip(_COUNT_NAMES, counts)})
    ns.loss_sum = loss_sum
    ns.accuracy = ns.correct / ns.scored if ns.scored else float('nan')
    ns.loss = loss_sum / ns.scored if ns.scored else float('nan')
    ns.confusion = conf
    ns.confusion_present = lambda: confusion_present(conf)
    ns.wrong = wrong[:min(max(ns.wrong_total, 0), cap)].copy()
    return ns


class Metrics:
    """``Metrics(n_classes, wrong_capacity=4096, device=None)``: the epoch state of include/dsp_frontend.h as one torch tensor
    (``state``, int64 words), zeroed by a launch.  Pass it as ``metrics=`` to ``cross_entropy``, ``TrainBatch.run`` /
    ``capture`` (with ``loss='native'``) and ``EnsembleBatch.run`` / ``capture`` (with ``labels=``); a recorded step updates it on
    every replay."""

    def __init__(self, n_classes, wrong_capacity=4096, device=None):
        import torch
        self.n_classes, self.wrong_capacity = int(n_classes), int(wrong_capacity)
        nbytes = state_bytes(self.n_classes, self.wrong_capacity)          # ValueError for sizes out of range, before any device work
        nat.require_device()
        self.device = torch.device('cuda', nat.current_device()) if device is None else torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError(f'Metrics lives on a GPU, not on {self.device}')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.state = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        self.reset()

    def reset(self):
        """Every field to zero: one launch on the current stream."""
        import torch
        with torch.cuda.device(self.device):
            nat.check_value(nat.load().dsp_metrics_reset(self.state.data_ptr(), self.n_classes, self.wrong_capacity,
                                                         torch.cuda.current_stream(self.device).cuda_stream), 'dsp_metrics_reset')

    def update(self, logits, labels, pred=None):
        """Score a batch: the arg-max of ``logits`` against ``labels``, or ``pred`` (int32 [B], e.g. the ensemble's) where
        given; the loss sum is taken from ``logits`` either way.  One launch, nothing returned, nothing synchronised."""
        xent(logits, labels, pred_in=pred, want=(), metrics=self)

    def result(self):
        """THE download and synchronisation of an epoch -> a namespace: seen, scored, correct, ignored, bad_label, wrong_total,
        calls (ints), accuracy = correct / scored and loss = loss_sum / scored (Python floats, NaN with nothing scored), loss_sum,
        confusion [C, C] int64 (rows the true label), confusion_present(), wrong [min(wrong_total, cap), 3] int32 rows of
        (index in the epoch, scored label, true label)."""
        return parse_state(self.state.cpu().numpy(), self.n_classes, self.wrong_capacity)


_UNIT = {}


def unit_grad(device):
    """The constant 1 that ``backward`` hands to autograd: a 0-dim fp32 tensor per device that nothing writes.  The backward of
    ``cross_entropy`` recognises it by its address and returns the stored gradient as it is (x * 1 = x in every bit, without
    the launch)."""
    import torch
    device = torch.device(device)
    u = _UNIT.get(device)
    if u is None:
        u = _UNIT[device] = torch.ones((), dtype=torch.float32, device=device)
    return u


def backward(loss):
    """``loss.backward()`` with ``unit_grad`` as the upstream gradient: for a loss from ``cross_entropy`` the step from the loss to
    the logits launches nothing."""
    import torch
    torch.autograd.backward(loss, grad_tensors=unit_grad(loss.device))


def _function():
    import torch

    class _CrossEntropy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, labels, metrics):
            ns = xent(logits, labels, want=('loss', 'dlogits'), metrics=metrics)
            ctx.save_for_backward(ns.dlogits)
            return ns.loss

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, g):
            dlogits, = ctx.saved_tensors
            u = _UNIT.get(g.device)
            if u is not None and g.data_ptr() == u.data_ptr():
                return dlogits, None, None
            return dlogits * g, None, None

    return _CrossEntropy


_FN = None


def cross_entropy(logits, labels, metrics=None):
    """``F.cross_entropy(logits, labels)`` at its defaults (mean over the labels in [0, C); -100 ignored) for fp32 [B, C] device
    logits, 2 <= C <= 64, B <= 16384: a 0-dim fp32 loss attached to the autograd graph.  The forward is one native call that
    also forms the gradient (upstream taken as 1); the backward is ``dlogits * grad_out`` -- one torch multiply, none for
    ``unit_grad``.  ``metrics``: a ``Metrics`` the same call updates.  ``labels`` are never differentiated.  Anything but fp32
    logits raises TypeError."""
    global _FN
    _check_logits(logits)
    if _FN is None:
        _FN = _function()
    return _FN.apply(logits, labels, metrics)
