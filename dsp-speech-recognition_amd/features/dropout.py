"""Reproducible dropout on the device (csrc/kernels_dropout.h, ``dsp_rng_advance`` / ``dsp_dropout_*``): the ``F.dropout`` calls
and ``nn.GRU``'s inter-layer dropout of rnn_clf.py drawn by a counter-based generator whose whole state is ``{seed, step}``, two
int64 words in device memory.  A multiplier is a pure function of (seed, step, site, element index) -- Philox4x32-10, key =
seed, counter = (element_index // 4, step, site); kept iff (word >> 8) < llrint((1 - p) 2^24) -- so an eager step and a graph
replay draw the same bits, a backward regenerates its mask from 16 saved bytes instead of storing it, and a checkpoint holds the
generator as two integers.  tools/philox_emul.py restates all of it in NumPy.

The draw sites of the heads (features/classifier.py), fixed:

    site            draw
    0               logits (``F.dropout(out, 0.2)``, every head but RNNHead)
    1               HMRNNHead: the encoder output in front of the HM-LSTM (``F.dropout(enc_out, 0.2)``)
    2               TransformerHead: the attention output (``F.dropout(attn_out, 0.5)``)
    8 + 4 k + l     the inter-layer draw of the k-th ``_DynEnc`` of a head (in the order the head runs them), layer l: the
                    multipliers of the input of GRU layer l + 1

Everything here is opt-in through the heads' ``rng=`` keyword; there is no fallback: without the library or a GPU it raises.
"""
from __future__ import annotations

from . import _native as nat

SITE_LOGITS = 0
SITE_HM_ENC = 1
SITE_ATTN = 2
SITE_GRU = 8                 # + 4 k + l
GRU_SITES_PER_ENC = 4        # _DynEnc serves at most 4 layers: at most 3 inter-layer draws


def gru_site(k, l=0):
    """The site of the inter-layer draw ``l`` of the ``k``-th ``_DynEnc`` of a head."""
    return SITE_GRU + GRU_SITES_PER_ENC * k + l


def _stream(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


class DeviceRng:
    """``DeviceRng(seed, device)``: owns ``state``, the int64 [2] device tensor ``{seed, step}`` every draw reads when its launch
    RUNS.  ``seed`` in [0, 2^64); the step starts at 0.  ``advance()`` is one launch on torch's current stream (``step += 1``);
    nothing is synchronised, so it can be recorded: ``TrainBatch`` puts one in front of every step."""

    def __init__(self, seed, device=None):
        import torch
        nat.require_device()
        dev = torch.device('cuda', nat.current_device()) if device is None else torch.device(device)
        if dev.type != 'cuda':
            raise ValueError(f'DeviceRng: device {dev} is not a GPU')
        self.state = torch.tensor([self._wrap(seed), 0], dtype=torch.int64, device=dev)
        self.device = self.state.device

    @staticmethod
    def _wrap(seed):
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f'DeviceRng: seed {seed} must be in [0, 2^64)')
        return seed - (1 << 64) if seed >= 1 << 63 else seed

    def advance(self):
        import torch
        with torch.cuda.device(self.device):
            nat.check_value(nat.load().dsp_rng_advance(self.state.data_ptr(), _stream(self.device)), 'dsp_rng_advance')

    def set_step(self, k):
        """The step the next draws read (after ``k`` advances from 0): one fill on the current stream, nothing synchronised."""
        k = int(k)
        if not 0 <= k < 1 << 63:
            raise ValueError(f'DeviceRng.set_step: step {k} must be in [0, 2^63)')
        self.state[1:].fill_(k)

    def state_dict(self):
        """-> {'seed', 'step'} as two Python ints.  Synchronises (checkpoints and tests)."""
        seed, step = self.state.tolist()
        return {'seed': seed & ((1 << 64) - 1), 'step': step}

    def load_state_dict(self, sd):
        import torch
        step = int(sd['step'])
        if not 0 <= step < 1 << 63:
            raise ValueError(f'DeviceRng.load_state_dict: step {step} must be in [0, 2^63)')
        self.state.copy_(torch.tensor([self._wrap(sd['seed']), step], dtype=torch.int64))
        torch.cuda.current_stream(self.device).synchronize()

    def multipliers(self, L, T, B, C, p, site_base, d_rows=None):
        """``dsp_dropout_multipliers``: the fp32 multipliers [L, T, B, C] ``dsp_bigru_forward_train`` takes as ``d_drop``; layer l
        draws at ``site_base + l``.  ``d_rows``: a one-element int32 tensor on the device; rows behind clamp(d_rows[0], 1, T)
        are exact zeros (None: all T rows are drawn)."""
        import torch
        m = torch.empty(L, T, B, C, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check_value(nat.load().dsp_dropout_multipliers(m.data_ptr(), L, T, B, C, float(p), int(site_base), self.state.data_ptr(),
                                                               None if d_rows is None else d_rows.data_ptr(), _stream(self.device)),
                            'dsp_dropout_multipliers')
        return m


def _check_input(who, x, rng):
    import torch
    if not isinstance(rng, DeviceRng):
        raise TypeError(f'{who}: rng must be a features.dropout.DeviceRng, not {type(rng).__name__}')
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        raise ValueError(f'{who}: the input must be a float32 CUDA tensor (there is no CPU route)')
    if x.device != rng.device:
        raise ValueError(f'{who}: the input is on {x.device}, the generator on {rng.device}')


def _device_dropout_function():
    import torch

    class _DeviceDropout(torch.autograd.Function):
        """y = x * m with m drawn at (rng's state, site); the backward multiplies the incoming gradient by the same m,
        regenerated from the 16-byte key the forward saved.  Inputs: (x, p, rng, site)."""

        @staticmethod
        def forward(ctx, x, p, rng, site):
            dev = x.device
            xc = x.detach().contiguous()
            y = torch.empty_like(xc)
            key = torch.empty(2, dtype=torch.int64, device=dev)
            with torch.cuda.device(dev):
                nat.check_value(nat.load().dsp_dropout_apply(xc.data_ptr(), y.data_ptr(), xc.numel(), p, site, rng.state.data_ptr(),
                                                             key.data_ptr(), _stream(dev)), 'dsp_dropout_apply')
            ctx.p, ctx.site = p, site
            ctx.save_for_backward(key)
            return y

        @staticmethod
        def backward(ctx, g):
            key, = ctx.saved_tensors
            dev = g.device
            gc = g.contiguous()
            dx = torch.empty_like(gc)
            with torch.cuda.device(dev):
                nat.check_value(nat.load().dsp_dropout_apply_key(gc.data_ptr(), dx.data_ptr(), gc.numel(), ctx.p, ctx.site, key.data_ptr(),
                                                                 _stream(dev)), 'dsp_dropout_apply_key')
            return dx, None, None, None

    return _DeviceDropout


_FUNCTION = None


def device_dropout(x, p, rng, site):
    """``F.dropout(x, p)`` (training=True) with the draws of ``rng`` at ``site``: a ``torch.autograd.Function`` over
    ``dsp_dropout_apply`` / ``dsp_dropout_apply_key``.  No mask is stored.  A non-contiguous ``x`` is made contiguous; the draw of
    an element depends on its row-major index in ``x`` alone."""
    global _FUNCTION
    _check_input('device_dropout', x, rng)
    if _FUNCTION is None:
        _FUNCTION = _device_dropout_function()
    return _FUNCTION.apply(x, float(p), rng, int(site))
