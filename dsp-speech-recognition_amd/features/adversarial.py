"""The sixth model of the reference: ``adv_clf.AdvHRNN`` / ``adv_model.AdvModel``, its answer to the person-held-out split.

An ``HRNN`` whose pooled feature [B, 400] also feeds a speaker discriminator -- a gradient reversal (gamma = 0.01),
``Linear(400, 200)``, ``tanh``, ``Linear(200, 35)`` (adv_clf.py:24-38) -- trained with ``CE(labels) + CE(speakers)``
(adv_model.py:45-47).

* ``gradient_reverse`` is the reversal as a new-style autograd function (the reference's is a legacy one that current torch
  refuses to run).
* ``AdvHRNNHead`` carries the reference's parameter names (``g.enc1.gru.*`` ... ``d2.bias``), so its checkpoints load.
* ``AdvHRNNHead.speaker_loss`` is the discriminator's loss.  Its torch route is the chain of adv_clf.py:35-38 under
  ``F.cross_entropy``; its native route is ONE autograd node over (feat, d1.weight, d1.bias, d2.weight, d2.bias) whose forward is
  ``dsp_adv_disc_train`` (csrc/kernels_adv.h: forward, loss and every gradient in at most eight launches) and whose backward
  launches nothing when the upstream gradient is ``features.metrics.unit_grad``.  ``native=None`` follows
  ``native_disc_default``.  There is no fallback: the native route without the library or a GPU raises.
"""
from __future__ import annotations

import types

import torch
from torch import nn

from .classifier import HRNNHead

MAX_B, MAX_F, MAX_H, MAX_S = 16384, 2048, 512, 64


class _GradientReverse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma):
        ctx.gamma = gamma
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad):
        return -grad * ctx.gamma, None


def gradient_reverse(x, gamma):
    """adv_clf.GradientReverse: the identity forward (``x.view_as(x)``), ``-grad * gamma`` backward.  ``gamma``: a Python number
    or a one-element tensor on x's device (read when the backward runs)."""
    return _GradientReverse.apply(x, gamma)


def work_bytes(B, F, H, S):
    """``dsp_adv_disc_work_bytes``; ValueError for sizes the library refuses.  Needs no device."""
    from . import _native as nat
    out = nat.c_i64(0)
    nat.check_value(nat.load().dsp_adv_disc_work_bytes(int(B), int(F), int(H), int(S), nat.C.byref(out)), 'invalid sizes')
    return out.value


def _ptr(t):
    return None if t is None else t.data_ptr()


def _check_feat(feat, W1, b1, W2, b2):
    """The operands of the native discriminator -> (feat with a unit column stride, B, F, H, S)."""
    if not torch.is_tensor(feat) or feat.dtype != torch.float32 or feat.dim() != 2:
        raise TypeError(f'feat must be a float32 [B, F] tensor, got {getattr(feat, "dtype", type(feat).__name__)}')
    if not feat.is_cuda:
        raise TypeError('the native discriminator needs device tensors (there is no CPU route)')
    B, F = feat.shape
    H, S = W1.shape[0], W2.shape[0]
    if tuple(W1.shape) != (H, F) or tuple(b1.shape) != (H,) or tuple(W2.shape) != (S, H) or tuple(b2.shape) != (S,):
        raise ValueError(f'parameter shapes {tuple(W1.shape)}, {tuple(b1.shape)}, {tuple(W2.shape)}, {tuple(b2.shape)} do not chain '
                         f'behind feat {tuple(feat.shape)}')
    for name, t in (('d1.weight', W1), ('d1.bias', b1), ('d2.weight', W2), ('d2.bias', b2)):
        if t.dtype != torch.float32 or t.device != feat.device or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous float32 tensor on feat's device")
    if feat.stride(1) != 1 or feat.stride(0) < F:
        feat = feat.contiguous()
    return feat, B, F, H, S


def _check_speakers(speakers, B, dev):
    if not torch.is_tensor(speakers) or speakers.dtype != torch.int64 or tuple(speakers.shape) != (B,) or speakers.device != dev:
        raise TypeError(f'speakers must be a [{B}] int64 tensor on {dev}')
    return speakers if speakers.is_contiguous() else speakers.contiguous()


def _check_gamma(d_gamma, dev):
    if d_gamma is not None and not (torch.is_tensor(d_gamma) and d_gamma.dtype == torch.float32 and d_gamma.numel() == 1
                                    and d_gamma.device == dev):
        raise TypeError('d_gamma must be a float32 device tensor of one element')


def disc_forward(feat, W1, b1, W2, b2, want_a=False):
    """One ``dsp_adv_disc_forward`` on torch's current stream: -> logits2 [B, S] (and a = tanh(feat W1^T + b1) [B, H] with
    ``want_a``).  Nothing is synchronised, nothing is differentiated."""
    from . import _native as nat
    feat, B, F, H, S = _check_feat(feat.detach(), W1.detach(), b1.detach(), W2.detach(), b2.detach())
    nat.require_device()
    dev = feat.device
    logits2 = torch.empty((B, S), dtype=torch.float32, device=dev)
    a = torch.empty((B, H), dtype=torch.float32, device=dev) if want_a else None
    with torch.cuda.device(dev):
        rc = nat.load().dsp_adv_disc_forward(feat.data_ptr(), feat.stride(0), B, F, H, S, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                                             b2.data_ptr(), _ptr(a), logits2.data_ptr(), S, torch.cuda.current_stream(dev).cuda_stream)
    nat.check_value(rc, 'invalid argument')
    return (logits2, a) if want_a else logits2


def disc_train(feat, W1, b1, W2, b2, speakers, gamma=0.01, d_gamma=None, grad_out=None, metrics=None,
               want=('logits2', 'dfeat', 'dW1', 'db1', 'dW2', 'db2')):
    """One ``dsp_adv_disc_train`` on torch's current stream; nothing is synchronised.  ``feat`` [B, F] fp32 device tensor (any row
    stride), the parameters dense, ``speakers`` int64 [B], ``gamma`` a number or -- ``d_gamma`` -- an fp32 device tensor of one
    element, ``grad_out`` fp32 [1] / 0-dim or None (= 1), ``metrics`` a ``features.metrics.Metrics`` over S classes to update.
    ``want``: which of the optional outputs to allocate and fill.  -> a namespace: loss (0-dim), a [B, H], dz [B, S] and the
    wanted ones (None otherwise)."""
    from . import _native as nat
    from .metrics import Metrics
    feat, B, F, H, S = _check_feat(feat, W1, b1, W2, b2)
    nat.require_device()
    dev = feat.device
    speakers = _check_speakers(speakers, B, dev)
    _check_gamma(d_gamma, dev)
    if grad_out is not None and not (torch.is_tensor(grad_out) and grad_out.dtype == torch.float32 and grad_out.numel() == 1
                                     and grad_out.device == dev):
        raise TypeError('grad_out must be a float32 device tensor of one element')
    if metrics is not None:
        if not isinstance(metrics, Metrics):
            raise TypeError(f'metrics must be a features.metrics.Metrics, not {type(metrics).__name__}')
        if metrics.n_classes != S or metrics.device != dev:
            raise ValueError(f'metrics is for {metrics.n_classes} classes on {metrics.device}; the discriminator has {S} on {dev}')
    bad = set(want) - {'logits2', 'dfeat', 'dW1', 'db1', 'dW2', 'db2'}
    if bad:
        raise ValueError(f'unknown outputs {sorted(bad)}')
    nbytes = work_bytes(B, F, H, S)

    def new(name, *shape):
        return torch.empty(shape, dtype=torch.float32, device=dev) if name is None or name in want else None
    ns = types.SimpleNamespace(loss=new(None), a=new(None, B, H), dz=new(None, B, S), logits2=new('logits2', B, S),
                               dfeat=new('dfeat', B, F), dW1=new('dW1', H, F), db1=new('db1', H), dW2=new('dW2', S, H), db2=new('db2', S))
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = nat.load().dsp_adv_disc_train(
            feat.data_ptr(), feat.stride(0), B, F, H, S, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), speakers.data_ptr(),
            _ptr(grad_out), float(gamma), _ptr(d_gamma), ns.a.data_ptr(), _ptr(ns.logits2), S, ns.loss.data_ptr(), ns.dz.data_ptr(),
            _ptr(ns.dfeat), F, _ptr(ns.dW1), _ptr(ns.db1), _ptr(ns.dW2), _ptr(ns.db2),
            None if metrics is None else metrics.state.data_ptr(), 0 if metrics is None else metrics.wrong_capacity, work.data_ptr(),
            nbytes, torch.cuda.current_stream(dev).cuda_stream)
    nat.check_value(rc, 'invalid argument')
    return ns


class _DiscTrain(torch.autograd.Function):
    """The native route of ``speaker_loss``: ONE node.  forward: ``dsp_adv_disc_train`` (only the gradients some input needs are
    formed); backward: the stored gradients as they are for ``unit_grad``, times the upstream gradient otherwise."""

    @staticmethod
    def forward(ctx, feat, W1, b1, W2, b2, speakers, gamma, d_gamma, metrics):
        need = ctx.needs_input_grad
        want = ['logits2'] + [n for n, k in zip(('dfeat', 'dW1', 'db1', 'dW2', 'db2'), need[:5]) if k]
        ns = disc_train(feat.detach(), W1.detach(), b1.detach(), W2.detach(), b2.detach(), speakers, gamma, d_gamma, None, metrics, want)
        ctx.grads = (ns.dfeat, ns.dW1, ns.db1, ns.dW2, ns.db2)
        ctx.mark_non_differentiable(ns.logits2)
        return ns.loss, ns.logits2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_logits2):
        from .metrics import _UNIT
        u = _UNIT.get(g.device)
        grads = ctx.grads
        if not (u is not None and g.data_ptr() == u.data_ptr()):
            grads = tuple(None if t is None else t * g for t in grads)
        return grads + (None, None, None, None)


class AdvHRNNHead(nn.Module):
    """adv_clf.AdvHRNN (adv_clf.py:24-38) with the reference's parameter names: ``g`` an ``HRNNHead``, ``d1 = Linear(400, 200)``,
    ``d2 = Linear(200, n_speakers)``; the reversal's factor is ``gamma`` (a number) or, once ``device_gamma()`` was called, the
    one-element device tensor ``d_gamma`` that a schedule may rewrite between the replays of a recorded step.

    ``forward(inp, len0, **kw)`` -> (logits, logits2) as adv_clf.py:33-38; every keyword ``HRNNHead.forward`` takes goes to ``g``.
    With ``speakers=`` (int64 [B]) it returns (logits, logits2, loss_speaker) -- ``speaker_loss`` on g's feature, which is how
    ``features.train.AdvTrainBatch`` calls it; ``native_disc`` / ``speaker_metrics`` are ``speaker_loss``'s ``native`` / ``metrics``.
    ``native_sums=True`` (``HRNNHead.forward``) goes to ``g`` and needs the native discriminator."""
    native_disc_default = False    # what ``native=None`` picks: the torch chain, until profiles/adv_kbench.json decides otherwise

    def __init__(self, feat_size=39, n_speakers=35, gamma=0.01):
        super().__init__()
        self.g = HRNNHead(feat_size)
        self.gamma = float(gamma)
        self.d_gamma = None
        self.d1 = nn.Linear(400, 200)
        self.d2 = nn.Linear(200, n_speakers)

    def device_gamma(self, value=None):
        """Keep gamma in device memory from now on (an fp32 tensor of one element on d1's device, not part of the state dict) and
        return it; ``value`` overwrites it in place (a copy on the current stream: replays behind it read the new value)."""
        if self.d_gamma is None or self.d_gamma.device != self.d1.weight.device:
            self.d_gamma = torch.full((1,), self.gamma, dtype=torch.float32, device=self.d1.weight.device)
        if value is not None:
            self.gamma = float(value)
            self.d_gamma.fill_(self.gamma)
        return self.d_gamma

    def _native(self, native):
        return self.native_disc_default if native is None else bool(native)

    def _gamma(self, feat):
        return self.d_gamma if self.d_gamma is not None and self.d_gamma.device == feat.device else self.gamma

    def _params(self):
        return self.d1.weight, self.d1.bias, self.d2.weight, self.d2.bias

    def discriminate(self, feat, native=None):
        """adv_clf.py:35-38: logits2 = d2(tanh(d1(rev(feat)))).  The native route (one ``dsp_adv_disc_forward``) serves calls
        that need no gradient; with one required, ``native=True`` raises (the native training route is ``speaker_loss``)."""
        needs_grad = torch.is_grad_enabled() and self.training and (feat.requires_grad or any(p.requires_grad for p in self._params()))
        if self._native(native):
            if needs_grad:
                if native:
                    raise RuntimeError('AdvHRNNHead: native_disc=True cannot return differentiable logits2: the native training route '
                                       'is speaker_loss (one node for the loss and every gradient)')
            else:
                return disc_forward(feat, *self._params())
        return self.d2(torch.tanh(self.d1(gradient_reverse(feat, self._gamma(feat)))))

    def speaker_loss(self, feat, speakers, native=None, metrics=None):
        """The discriminator's loss on the pooled feature [B, 400] -> a namespace (loss: 0-dim, logits2 [B, n_speakers]).
        ``native=None`` follows ``native_disc_default``.  torch route: ``F.cross_entropy(d2(tanh(d1(gradient_reverse(feat, gamma)))),
        speakers)``.  Native route: one autograd node whose forward is ``dsp_adv_disc_train``; under ``no_grad`` or ``eval()`` it is
        ``dsp_adv_disc_forward`` and the loss call alone.  ``metrics`` (a ``features.metrics.Metrics`` over n_speakers classes) is
        updated by the native call and needs the native route."""
        if not self._native(native):
            if metrics is not None:
                raise ValueError('speaker metrics need the native discriminator: they are updated by its loss call')
            logits2 = self.d2(torch.tanh(self.d1(gradient_reverse(feat, self._gamma(feat)))))
            return types.SimpleNamespace(loss=torch.nn.functional.cross_entropy(logits2, speakers), logits2=logits2)
        if not (torch.is_grad_enabled() and self.training):
            from .metrics import xent
            logits2 = disc_forward(feat, *self._params())
            return types.SimpleNamespace(loss=xent(logits2, speakers, want=('loss',), metrics=metrics).loss, logits2=logits2)
        g = self._gamma(feat)
        tensor = torch.is_tensor(g)
        loss, logits2 = _DiscTrain.apply(feat, *self._params(), speakers, self.gamma if tensor else g, g if tensor else None, metrics)
        return types.SimpleNamespace(loss=loss, logits2=logits2)

    def forward(self, inp, len0, speakers=None, native_disc=None, speaker_metrics=None, **kw):
        if kw.get('native_sums') and not (speakers is not None and self._native(native_disc)):
            raise RuntimeError('AdvHRNNHead: native_sums=True needs speakers= and native_disc=True: the torch discriminator forms its '
                               'bias gradients and its loss with reductions of torch\'s')
        logits, feat = self.g(inp, len0, **kw)
        if speakers is None:
            return logits, self.discriminate(feat, native_disc)
        r = self.speaker_loss(feat, speakers, native_disc, speaker_metrics)
        return logits, r.logits2, r.loss
