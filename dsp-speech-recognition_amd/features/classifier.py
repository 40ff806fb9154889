"""PyTorch-ROCm stand-ins of the reference's recurrent classifiers (RNN, HRNN, HRNN_Att, Transformer, HMRNN), for SURVEY row f-3 (device-resident
features feed the RNN without a host round trip) and for the configs[4] throughput figure of bench.py.

The reference's own classes (rnn_clf.py, layers.py) run unchanged on PyTorch-ROCm; they are not part of this
package and do not travel to the GPU box.  This module restates the forward pass of ``rnn_clf.RNN``
(rnn_clf.py:12-34) over ``layers.DynamicEncoder`` (layers.py:42-76) so that the tests can pin it to logits the
REAL reference class produced (tests/golden/make_rnn_golden.py -> tests/golden/rnn_golden.npz):

    sort by length -> pack_padded_sequence -> 3-layer bidirectional GRU(39 -> 200) -> pad_packed_sequence
    -> forward + backward halves summed -> unsort -> sum over time / length  ||  max over time -> Linear(400 -> 20)

Two details of the reference that a "masked pooling" rewrite would get wrong, kept here on purpose:
the time axis of the GRU output is max(len0), not the padded 200, and the max pooling runs over the zero rows
``pad_packed_sequence`` leaves behind shorter utterances (an utterance whose activations are all negative pools to 0).

The encoder in front of every head (``_DynEnc``) has a native forward pass (csrc/kernels_bigru.h) beside the ``nn.GRU`` route;
both yield max(len0) rows with zero rows behind each end, so the pooling above is the same on either.  With a gradient
required, ``native_enc=True`` takes the native training path (``_DynEncTrain``, csrc/kernels_bigru_bwd.h).

The two attention blocks -- ``_TransformerEncoder`` in front of ``TransformerHead`` and ``_SelfAttn``, the pooling of
``HRNNAttHead`` -- have opt-in native forward passes as well (csrc/kernels_attn.h), reached through ``native_attn=True``.  With a
gradient required, ``native_attn=True`` takes their native training paths (``_AttnTrain`` / ``_SelfAttnTrain``,
csrc/kernels_attn_bwd.h): the forward saves a tape without any [B, T, T] tensor, the backward is four launches (one for the
pooling) and the parameter gradients are GEMMs over the rows it leaves (``attn_param_grads``).  ``native_attn=None`` keeps the
torch chains whenever a gradient is required, unless ``native_train_default`` is set.

``device_len=True`` on a head's forward keeps the lengths on the device (a [B] int32 tensor, e.g. the ``len0`` a captured front
end leaves there): the row counts come from ``dsp_head_lengths_batch``, the encoders run over all ``inp.shape[0]`` rows with the
lengths read in place, and the two places that need max(len0) -- the pooling and ``_SelfAttn``'s softmax -- read it from device
memory (``dsp_head_pool_batch``, ``dsp_selfattn_pool_rows_batch``; csrc/kernels_head.h).  Nothing reads device memory from the
host, so the call can be captured in a HIP graph.  Forward only, every stage native -- unless ``device_grad=True`` is given as
well: a required gradient is then served on the same path, still without a host round trip.  The encoders take their native
training paths over all ``inp.shape[0]`` rows with the lengths read in place, the pooling and ``_SelfAttn`` get their
backward from ``dsp_head_pool_train_batch`` / ``dsp_head_pool_backward_batch`` and the ``dsp_selfattn_pool_rows_*`` pair, and the
native handles are repacked in place after an optimiser step (``dsp_*_refresh``) instead of destroyed and rebuilt, so a whole
training step -- refresh, forward, loss, backward -- can be captured too (features/train.py: ``TrainBatch``).
"""
import numpy as np
import torch
from torch import nn

from .dropout import SITE_ATTN, SITE_GRU, SITE_HM_ENC, SITE_LOGITS, device_dropout, gru_site


def _lengths(len0):
    """Lengths as a list, a NumPy array or a tensor (any device, any integer dtype) -> an int64 NumPy array."""
    return np.asarray(len0.cpu() if torch.is_tensor(len0) else len0, dtype=np.int64)


def _ptr(t):
    return None if t is None else t.data_ptr()      # an optional tensor: None is a NULL argument


def _dropout(x, p, rng, site):
    """``F.dropout(x, p)`` in training mode: torch's draw, or with ``rng`` (a ``features.dropout.DeviceRng``) the device
    generator's at ``site`` (features/dropout.py holds the table of sites)."""
    if rng is None:
        return torch.nn.functional.dropout(x, p)
    return device_dropout(x, p, rng, site)


def _check_device_grad(who, device_len, device_grad):
    """``device_grad=True`` is the training form of ``device_len=True`` and means nothing without it."""
    if device_grad and not device_len:
        raise ValueError(f'{who}: device_grad=True needs device_len=True (it is the training form of the device-length path)')


def _want_wgrad(who, native_wgrad, default, train):
    """``native_wgrad`` resolved.  The switch is valid wherever the native training path runs (``train``); anywhere else an
    explicit True raises.  None takes the class default, which never raises."""
    if native_wgrad and not train:
        raise RuntimeError(f'{who}: native_wgrad=True cannot run: the native training path does not run here (no gradient is '
                           'required, or another route was chosen)')
    return bool(train and (default if native_wgrad is None else native_wgrad))


def _want_sums(who, native_sums, default, train):
    """``native_sums`` resolved, as ``_want_wgrad`` resolves its switch.  It is valid where the device-length training path runs
    (``device_len=True, device_grad=True`` under a required gradient: ``train``); anywhere else an explicit True raises."""
    if native_sums and not train:
        raise RuntimeError(f'{who}: native_sums=True cannot run: it serves the device-length training path (device_len=True, '
                           'device_grad=True with a gradient required)')
    return bool(train and (default if native_sums is None else native_sums))


class _LinearSums(torch.autograd.Function):
    """An output layer ``F.linear(feat, W, b)`` whose backward records no reduction of torch's (``native_sums=True``): the forward
    is the same addmm, so the logits keep their bits; backward: dfeat = g W as a GEMM, dW = g^T feat with db its column sums as
    the two launches of ``dsp_rows_wgrad`` with T = 1 (features/wgrad.py: ``rows_gemm``)."""

    @staticmethod
    def forward(ctx, feat, W, b):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(feat, W)
        return torch.nn.functional.linear(feat, W, b)

    @staticmethod
    def backward(ctx, g):
        from .wgrad import rows_gemm
        if g is None:
            return None, None, None
        feat, W = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        need = ctx.needs_input_grad
        d_feat = g @ W if need[0] else None
        dW = db = None
        if need[1] or need[2]:
            dW, db = rows_gemm(g.unsqueeze(0), feat.detach().unsqueeze(0), colsum=True)
        return d_feat, dW if need[1] else None, db if need[2] else None


def _out_layer(linear, feat, sums):
    """``linear(feat)``; with ``sums`` through ``_LinearSums``."""
    return _LinearSums.apply(feat, linear.weight, linear.bias) if sums else linear(feat)


def _check_rows_word(who, d_rows, x):
    if not (torch.is_tensor(d_rows) and d_rows.dtype == torch.int32 and d_rows.numel() == 1 and d_rows.device == x.device):
        raise TypeError(f"{who}: d_rows must be a one-element int32 tensor on the input's device")


def _check_device_len(who, inp, len0, module, device_grad=False):
    """The conditions of ``device_len=True``: lengths as a [B] int32 tensor on ``inp``'s device, and no gradient required
    unless ``device_grad`` is given.  -> whether a gradient is required."""
    if not torch.is_tensor(inp) or not inp.is_cuda:
        raise RuntimeError(f'{who}: device_len=True cannot run: the input is not on a GPU')
    if not (torch.is_tensor(len0) and len0.dtype == torch.int32 and len0.dim() == 1 and len0.shape[0] == inp.shape[1]
            and len0.device == inp.device):
        raise TypeError(f"{who}: device_len=True needs len0 as a [B] int32 tensor on the input's device")
    needs_grad = torch.is_grad_enabled() and (inp.requires_grad or any(p.requires_grad for p in module.parameters()))
    if needs_grad and not device_grad:
        raise RuntimeError(f'{who}: device_len=True cannot run: a gradient is required (the device-length path is forward only '
                           'unless device_grad=True is given)')
    return needs_grad


def head_length_info(len0, T, hir):
    """The row counts of a batch whose lengths are on the device (``dsp_head_lengths_batch``, one launch on the current
    stream): len0 [B] int32 device tensor -> (len0c [B] = clamp(len0, 1, T), len1 [B] = ceil(len0c / hir), info [4] =
    (max len0c, ceil(max len0c / hir), number of entries that had to be clamped, 0)), three int32 device tensors."""
    from . import _native as nat
    if not (torch.is_tensor(len0) and len0.is_cuda and len0.dtype == torch.int32 and len0.dim() == 1):
        raise TypeError('head_length_info needs a [B] int32 device tensor')
    dev, B = len0.device, len0.shape[0]
    len0 = len0.contiguous()
    with torch.cuda.device(dev):
        len0c = torch.empty(B, dtype=torch.int32, device=dev)
        len1 = torch.empty(B, dtype=torch.int32, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)
        nat.check(nat.load().dsp_head_lengths_batch(len0.data_ptr(), B, int(T), int(hir), len0c.data_ptr(), len1.data_ptr(),
                                                    info.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return len0c, len1, info


def _pool_native(y, d_len, d_rows, avg=True, grad=False):
    """``dsp_head_pool_batch`` over y [T, B, H] (fp32, on a GPU): -> [B, 2 H] = sum over t < len / len || max over the first
    *d_rows rows (zero rows included, unread), or the max half [B, H] alone with ``avg=False``.  ``grad=True``: where y requires a gradient the result carries it
    (``_PoolTrain``); otherwise y is read detached, as always."""
    from . import _native as nat
    if grad and torch.is_grad_enabled() and y.requires_grad:                  # ``grad``: the caller's device_grad=True
        return _PoolTrain.apply(y, d_len, d_rows, avg)
    T, B, H = y.shape
    dev = y.device
    yc = y.detach().to(torch.float32).contiguous()
    with torch.cuda.device(dev):
        feat = torch.empty(B, 2 * H if avg else H, dtype=torch.float32, device=dev)
        nat.check(nat.load().dsp_head_pool_batch(yc.data_ptr(), T, B, H, d_len.data_ptr(), d_rows.data_ptr(), feat.data_ptr(),
                                                 feat.stride(0), 0 if avg else -1, H if avg else 0,
                                                 torch.cuda.current_stream(dev).cuda_stream))
    return feat


class _PoolTrain(torch.autograd.Function):
    """``_pool_native`` with a gradient.  forward: dsp_head_pool_train_batch (the pooling kernel, which also saves the row each
    maximum came from, arg [B, H] int32); backward: dsp_head_pool_backward_batch, one streaming launch that writes every
    element of g_y [T, B, H] (zeros at t >= len; the gradient of a maximum the padding won is dropped).  The lengths and the
    row count are read on the device in both."""

    @staticmethod
    def forward(ctx, y, d_len, d_rows, avg):
        from . import _native as nat
        ctx.set_materialize_grads(False)
        T, B, H = y.shape
        dev = y.device
        yc = y.detach().to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            feat = torch.empty(B, 2 * H if avg else H, dtype=torch.float32, device=dev)
            arg = torch.empty(B, H, dtype=torch.int32, device=dev)
            nat.check(nat.load().dsp_head_pool_train_batch(yc.data_ptr(), T, B, H, d_len.data_ptr(), d_rows.data_ptr(), feat.data_ptr(),
                                                           feat.stride(0), 0 if avg else -1, H if avg else 0, arg.data_ptr(),
                                                           torch.cuda.current_stream(dev).cuda_stream))
        ctx.shape, ctx.avg = (T, B, H), avg
        ctx.save_for_backward(d_len, arg)
        return feat

    @staticmethod
    def backward(ctx, g_feat):
        from . import _native as nat
        if g_feat is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        d_len, arg = ctx.saved_tensors
        T, B, H = ctx.shape
        dev = arg.device
        g = g_feat.detach().to(torch.float32)
        if g.stride(1) != 1 or g.stride(0) < g.shape[1]:                        # (the call takes any row stride, not a column stride)
            g = g.contiguous()
        with torch.cuda.device(dev):
            g_y = torch.empty(T, B, H, dtype=torch.float32, device=dev)
            nat.check(nat.load().dsp_head_pool_backward_batch(g.data_ptr(), g.stride(0), 0 if ctx.avg else -1, H if ctx.avg else 0,
                                                              d_len.data_ptr(), arg.data_ptr(), T, B, H, g_y.data_ptr(),
                                                              torch.cuda.current_stream(dev).cuda_stream))
        return g_y, None, None, None


def _pack_state(hidden, H1, H2, B, **f32):
    """hidden = (h1, c1, z1, h2, c2, z2) as [H, B] / [1, B] -> the flat h1 | c1 | z1 | h2 | c2 | z2 buffer of the kernels."""
    state = torch.cat([v.detach().to(**f32).reshape(-1) for v in hidden])
    assert state.numel() == (2 * H1 + 2 * H2 + 2) * B, 'hidden does not fit (h1, c1, z1, h2, c2, z2) of this batch'
    return state


def _split_state(state, H1, H2, B):
    """The flat h1 | c1 | z1 | h2 | c2 | z2 buffer -> the six ``hidden`` views [H1, B], [H1, B], [1, B], [H2, B], [H2, B], [1, B]."""
    rows = (H1, H1, 1, H2, H2, 1)
    return tuple(v.view(n, B) for v, n in zip(torch.split(state, [n * B for n in rows]), rows))


class _NativeHandle:
    """The life cycle of a module's native handle (the packed copy of its parameters): built on first use, rebuilt when a
    parameter moved or was written (data_ptr / _version), destroyed with the module, never shared with a copy.  The module
    supplies ``_params()``, ``_descriptor(nat)`` -> the create function's descriptor of them, and ``_lib``, the prefix of the
    library's create / destroy functions."""
    _lib = _handle = _handle_key = None

    def _drop_handle(self):
        if self._handle is not None:
            try:                                    # (at interpreter shutdown even the import may fail)
                from . import _native as nat
                getattr(nat.load(), self._lib + '_destroy')(self._handle)
            except Exception:
                pass
            self._handle, self._handle_key = None, None

    __del__ = _drop_handle

    def __getstate__(self):
        """Copies (copy.deepcopy, pickling) do not share the native handle: each builds its own on first use."""
        d = self.__dict__.copy()
        d['_handle'], d['_handle_key'] = None, None
        return d

    def _param_key(self, dev_index):
        return (dev_index,) + tuple((p.data_ptr(), p._version) for p in self._params())

    def _native_handle(self, dev, refresh=False):
        """``refresh=True``: where the key differs from the handle's in ``_version``s only -- same device, same tensors,
        written in place, which is what an optimiser step leaves -- the handle is kept and its packed copy rewritten by
        launches on torch's current stream (``dsp_*_refresh``: nothing allocated or synchronised; the stream orders the
        repack behind the step that wrote the parameters and in front of the calls that follow).  ``refresh='always'`` repacks
        on an equal key as well, so that a recorded sequence carries the repack.  Anything else rebuilds as before."""
        key = self._param_key(dev.index)
        old = self._handle_key
        if refresh and self._handle is not None and key[0] == old[0] and [p for p, _ in key[1:]] == [p for p, _ in old[1:]]:
            if key != old or refresh == 'always':
                from . import _native as nat
                d = self._descriptor(nat)
                with torch.cuda.device(dev):
                    nat.check(getattr(nat.load(), self._lib + '_refresh')(self._handle, nat.C.byref(d),
                                                                         torch.cuda.current_stream(dev).cuda_stream))
                self._handle_key = key
            return self._handle
        if self._handle is None or key != self._handle_key:
            from . import _native as nat
            self._drop_handle()
            d, h = self._descriptor(nat), nat.c_vp(0)
            nat.check(getattr(nat.load(), self._lib + '_create')(nat.C.byref(d), nat.C.byref(h)))
            self._handle, self._handle_key = h.value, key
        return self._handle

    def _check_unmodified(self, key):
        """``key``: the ``_handle_key`` a forward ran with."""
        if self._handle is None or self._handle_key != key or self._param_key(key[0]) != key:
            raise RuntimeError(f'{type(self).__name__}: a parameter was modified between the native forward and its backward')


class _DynEnc(_NativeHandle, nn.Module):
    """layers.DynamicEncoder (layers.py:42-76): bidirectional GRU over ragged lengths, output padded to max(lens) rows (zeros
    behind each end), forward + backward halves SUMMED.  Parameter names ``gru.*``.

    Two paths compute the same thing:
      * the ``nn.GRU`` one -- the reference's own route: sort by length (np.argsort(-lens): stable), pack, GRU, pad back,
        unsort; on any device, with gradients, with inter-layer dropout in training mode;
      * the native one -- ``dsp_bigru_forward`` (csrc/kernels_bigru.h), forward only, fp32, on the tensors in place on the
        current stream.  Nothing is sorted or packed: a column depends on no other column, so the kernel masks on
        ``t < len``.  Runs for CUDA/ROCm tensors when no gradient is required and inter-layer dropout is inactive;
        ``native=None`` picks it only where ``native_default`` says so.
        ``native=True`` insists on it (and raises where it cannot run), ``native=False`` keeps ``nn.GRU``.
        With a gradient required, ``native=True`` takes the native TRAINING path (``_DynEncTrain``): the forward saves a tape
        (``dsp_bigru_forward_train``), the backward recurrence is one launch per layer (``dsp_bigru_backward``,
        csrc/kernels_bigru_bwd.h) and the gradients of the parameters and of x are GEMMs over what it leaves
        (``gru_param_grads``).  y and h_n both carry the gradient; inter-layer dropout in training mode is drawn with torch
        and handed to the kernel as multipliers.  The training path serves modules in TRAINING mode (``.train()``): in eval
        mode a required gradient stays a reason the native path cannot run, as it was before that path existed.
        ``native=None`` keeps ``nn.GRU`` whenever a gradient is required, unless ``native_train_default`` is set."""
    native_default = False         # what ``native=None`` picks where the native path can run: opt-in until DESIGN 7.3's timing shows it ahead
    native_train_default = False   # what ``native=None`` picks when a gradient is required: nn.GRU, until DESIGN 7.5's timing decides
    native_wgrad_default = False   # what ``native_wgrad=None`` picks on the native training path: torch's GEMMs
    _lib = 'dsp_bigru'

    def __init__(self, input_size, hidden_size, n_layers, dropout=0.0):
        super().__init__()
        self.hidden_size = hidden_size
        self.gru = nn.GRU(input_size, hidden_size, n_layers, dropout=dropout, bidirectional=True)

    # ---- native path ------------------------------------------------------------------------------------------------
    def _params(self):
        """nn.GRU's order: per layer weight_ih, weight_hh, bias_ih, bias_hh, then the same four of the reverse direction."""
        g = self.gru
        return [getattr(g, f'{n}_l{l}{sfx}') for l in range(g.num_layers) for sfx in ('', '_reverse')
                for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]

    def native_supported(self, x, train=False):
        """Why the native path cannot serve ``x`` (a string), or None when it can.  ``train``: the training path, which
        applies inter-layer dropout itself."""
        from . import _native as nat
        import os
        g = self.gru
        if not x.is_cuda:
            return 'the input is not on a GPU'
        if x.dtype != torch.float32 or any(p.dtype != torch.float32 or p.device != x.device for p in self._params()):
            return 'input and parameters must be float32 on one device'
        if any(not p.is_contiguous() for p in self._params()):
            return 'parameters must be contiguous'
        if not (1 <= g.input_size <= 512 and 4 <= g.hidden_size <= 256 and g.hidden_size % 4 == 0 and 1 <= g.num_layers <= 4):
            return 'sizes out of range: input_size in [1, 512], hidden a multiple of 4 in [4, 256], 1 to 4 layers'
        if not train and self.training and g.dropout > 0 and g.num_layers > 1:
            return 'inter-layer dropout is active (training mode)'
        if not os.path.exists(nat.LIB_PATH):
            return f'{nat.LIB_PATH} is not built'
        return None

    def _descriptor(self, nat):
        d = nat.BigruDesc(self.gru.input_size, self.gru.hidden_size, self.gru.num_layers, 0)
        d.d_params[:8 * self.gru.num_layers] = [p.data_ptr() for p in self._params()]
        return d

    def _run_native(self, x, lens):
        B, dev = x.shape[1], x.device
        T = int(lens.max())
        assert lens.numel() == B and int(lens.min()) >= 1 and T <= x.shape[0], 'lengths do not fit the input'
        with torch.cuda.device(dev):
            return self._launch_native(x, T, lens.to(torch.int32).to(dev))

    def _launch_native(self, x, T, d_len):
        """The forward over the first ``T`` rows of x with the lengths ``d_len`` ([B] int32, in [1, T]) read on the device."""
        from . import _native as nat
        B, H, dev = x.shape[1], self.hidden_size, x.device
        x = x.detach().contiguous()
        with torch.cuda.device(dev):
            handle = self._native_handle(dev)
            lib = nat.load()
            nbytes = nat.c_i64(0)
            nat.check(lib.dsp_bigru_workspace_bytes(handle, T, B, nat.C.byref(nbytes)))
            work = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
            y = torch.empty(T, B, H, dtype=torch.float32, device=dev)
            hn = torch.empty(2 * self.gru.num_layers, B, H, dtype=torch.float32, device=dev)
            nat.check(lib.dsp_bigru_forward(handle, x.data_ptr(), T, B, d_len.data_ptr(), y.data_ptr(), hn.data_ptr(),
                                            work.data_ptr(), nbytes.value, torch.cuda.current_stream(dev).cuda_stream))
        return y, hn

    def _run_native_train(self, x, lens, drop=None, wgrad=False, rng=None, rng_site=SITE_GRU):
        """The native training path: y and h_n attached to the autograd graph.  ``drop``: the inter-layer multipliers
        [n_layers - 1, max(lens), B, 2 H] (0 or 1 / (1 - p)); drawn here in training mode when None -- with torch, or, with
        ``rng`` (a ``features.dropout.DeviceRng``), by ``dsp_dropout_multipliers`` at the sites ``rng_site + l``.  ``wgrad``: the
        products behind the backward recurrence as native launches (features/wgrad.py) over the max(lens) rows."""
        B, H, dev, g = x.shape[1], self.hidden_size, x.device, self.gru
        T = int(lens.max())
        assert lens.numel() == B and int(lens.min()) >= 1 and T <= x.shape[0], 'lengths do not fit the input'
        x = x[:T]                                                               # (autograd pads the gradient of the rows behind)
        with torch.cuda.device(dev):
            self._native_handle(dev)
            d_len = lens.to(torch.int32).to(dev)
            if drop is None and self.training and g.dropout > 0 and g.num_layers > 1:
                if rng is not None:
                    drop = rng.multipliers(g.num_layers - 1, T, B, 2 * H, g.dropout, rng_site)
                else:
                    keep = 1.0 - g.dropout
                    drop = (torch.rand(g.num_layers - 1, T, B, 2 * H, device=dev) < keep).to(torch.float32) / keep
            if drop is not None:
                drop = drop.detach().to(torch.float32).contiguous()
                assert tuple(drop.shape) == (g.num_layers - 1, T, B, 2 * H), 'drop does not fit [n_layers - 1, T, B, 2 H]'
            if wgrad:
                return _DynEncWgradTrain.apply(self, T, d_len, drop, x, None, *self._params())
            return _DynEncTrain.apply(self, T, d_len, drop, x, *self._params())

    def _run_device_train(self, x, d_len, drop=None, wgrad=False, d_rows=None, rng=None, rng_site=SITE_GRU):
        """The native training path with the lengths on the device (``device_grad=True``): all x.shape[0] rows of the buffer
        are used -- max(len0) is not known here --, so the multipliers are drawn as [n_layers - 1, x.shape[0], B, 2 H].  The
        handle survives an optimiser step (``refresh=True``).  ``wgrad``: the products behind the backward recurrence as
        native launches that stop at clamp(d_rows[0], 1, T) rows, read on the device (all T rows without ``d_rows``).
        ``rng``: the multipliers come from ``dsp_dropout_multipliers`` at the sites ``rng_site + l``, drawn for the rows below
        the same ``d_rows`` bound and exact zeros behind it (all rows without ``d_rows``)."""
        B, H, dev, g = x.shape[1], self.hidden_size, x.device, self.gru
        T = x.shape[0]
        with torch.cuda.device(dev):
            self._native_handle(dev, refresh=True)
            if drop is None and self.training and g.dropout > 0 and g.num_layers > 1:
                if rng is not None:
                    drop = rng.multipliers(g.num_layers - 1, T, B, 2 * H, g.dropout, rng_site, d_rows)
                else:
                    keep = 1.0 - g.dropout
                    drop = (torch.rand(g.num_layers - 1, T, B, 2 * H, device=dev) < keep).to(torch.float32) / keep
            if drop is not None:
                drop = drop.detach().to(torch.float32).contiguous()
                assert tuple(drop.shape) == (g.num_layers - 1, T, B, 2 * H), 'drop does not fit [n_layers - 1, T, B, 2 H]'
            if wgrad:
                return _DynEncWgradTrain.apply(self, T, d_len, drop, x, d_rows, *self._params())
            return _DynEncDeviceTrain.apply(self, T, d_len, drop, x, *self._params())

    # ---- nn.GRU path (layers.py:63-76) -----------------------------------------------------------------------------------
    def _run_torch(self, x, lens, rng=None):
        if rng is not None and self.training and self.gru.dropout > 0 and self.gru.num_layers > 1:
            raise RuntimeError('_DynEnc: rng= needs the native training path (native=True or device_grad=True): nn.GRU draws its '
                               'inter-layer dropout itself')
        order = torch.argsort(lens, descending=True, stable=True)
        unsort = torch.argsort(order).to(x.device)
        packed = nn.utils.rnn.pack_padded_sequence(x[:, order.to(x.device)], lens[order])
        y, hn = self.gru(packed)
        y, _ = nn.utils.rnn.pad_packed_sequence(y)
        h = self.hidden_size
        return (y[:, :, :h] + y[:, :, h:])[:, unsort].contiguous(), hn[:, unsort].contiguous()

    def run(self, x, lens, native=None, device_len=False, device_grad=False, native_wgrad=None, d_rows=None, rng=None, rng_site=SITE_GRU):
        """-> (y [max(lens), B, H], h_n [2 n_layers, B, H]), the reference's return value (layers.py:76).
        ``rng`` (a ``features.dropout.DeviceRng``): the native training path draws its inter-layer multipliers with
        ``dsp_dropout_multipliers`` at the sites ``rng_site + l`` instead of with torch; where inter-layer dropout is active and
        the route is nn.GRU's it raises.  ``rng=None`` changes nothing.
        ``native_wgrad=True``: on the native training path -- either route -- the products behind the backward recurrence
        (``gru_param_grads``) run as native launches (features/wgrad.py) instead of torch's GEMMs, sums and ``cat`` copies;
        anywhere else it raises.  ``native_wgrad=None`` takes ``native_wgrad_default``.  ``d_rows`` (with ``device_grad=True``): a
        one-element int32 tensor on x's device holding a row count no smaller than the longest length, such as
        ``head_length_info(...)[2][0:1]``: those launches stop at clamp(d_rows[0], 1, x.shape[0]) rows, read on the device.  It
        is read on the device when the kernels run and must hold the same value at the backward call.  On the host-length
        route the buffers already end at max(lens) rows and no bound is needed.
        ``device_len=True``: ``lens`` is a [B] int32 tensor on x's device with entries in [1, x.shape[0]] and stays there; the
        native forward runs over all x.shape[0] rows (y has that many, exact zero rows behind each end) and nothing is read
        back.  Forward only: a required gradient, or anything else the native path cannot serve, raises --
        unless ``device_grad=True`` is given as well: a required gradient then takes the native training path over all
        x.shape[0] rows (``_run_device_train``; training mode, as ``native=True``), and the handle is refreshed in place
        after an optimiser step instead of rebuilt."""
        _check_device_grad('_DynEnc', device_len, device_grad)
        draw = {} if rng is None else {'rng': rng, 'rng_site': rng_site}        # (without rng= the training paths are called as before)
        if d_rows is not None:
            if not device_grad:
                raise ValueError('_DynEnc: d_rows needs device_len=True, device_grad=True (it bounds the native training path)')
            _check_rows_word('_DynEnc', d_rows, x)
        if device_len:
            needs_grad = _check_device_len('_DynEnc', x, lens, self, device_grad)
            if needs_grad and not self.training:
                why = 'a gradient is required and the module is in eval mode (the native training path serves training mode)'
            else:
                why = self.native_supported(x, train=needs_grad)
            if why is not None:
                raise RuntimeError(f'_DynEnc: the native path cannot run: {why}')
            wgrad = _want_wgrad('_DynEnc', native_wgrad, self.native_wgrad_default, needs_grad)
            if needs_grad:
                return self._run_device_train(x, lens.contiguous(), wgrad=wgrad, d_rows=d_rows, **draw)
            if device_grad:
                self._native_handle(x.device, refresh=True)
            return self._launch_native(x, x.shape[0], lens.contiguous())
        lens = torch.as_tensor(_lengths(lens))
        if native is False:
            _want_wgrad('_DynEnc', native_wgrad, False, False)
            return self._run_torch(x, lens, rng)
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if native is None and not (self.native_train_default if needs_grad else self.native_default):
            _want_wgrad('_DynEnc', native_wgrad, False, False)
            return self._run_torch(x, lens, rng)                                # (nothing to find out about the native path)
        if needs_grad and not self.training:                                    # eval mode keeps what it always did: no native gradient
            why = 'a gradient is required and the module is in eval mode (the native training path serves training mode)'
        else:
            why = self.native_supported(x, train=needs_grad)
        if native is None:
            native = why is None
        if native:
            if why is not None:
                raise RuntimeError(f"_DynEnc: the native {'training path (a gradient is required)' if needs_grad else 'path'} cannot run: {why}")
            wgrad = _want_wgrad('_DynEnc', native_wgrad, self.native_wgrad_default, needs_grad)
            return self._run_native_train(x, lens, wgrad=wgrad, **draw) if needs_grad else self._run_native(x, lens)
        _want_wgrad('_DynEnc', native_wgrad, False, False)
        return self._run_torch(x, lens, rng)

    def forward(self, x, lens, native=None, device_len=False, device_grad=False, native_wgrad=None, d_rows=None, rng=None, rng_site=SITE_GRU):
        return self.run(x, lens, native, device_len, device_grad, native_wgrad, d_rows, rng, rng_site)[0]


def _ones_col_sum(a):
    """a [n, m] -> the column sums [m] as a product with a row of ones.  The device-length training path forms the GRU bias
    gradients with it in place of ``a.sum(0)``: recorded in a HIP graph inside a whole training step, that reduction
    (T B = 1000 rows of a strided view into 600 columns) gave seven of the eight bias gradients wrong by up to 0.1 max |ref|
    from the SECOND replay on, while every product replayed bit for bit.  torch's split reductions zero their counters with
    a memset, and a recorded memset of more than 4 bytes is not replayed faithfully on this stack (DESIGN 7.12,
    tools/probes/graph_memset_replay.py).  The host-length routes keep ``a.sum(0)`` and their bits."""
    return (a.new_ones(1, a.shape[0]) @ a).reshape(-1)


def gru_param_grads(params, x, out, da, drop=None, need=None, col_sum=None):
    """The GEMMs behind one layer of the backward recurrence (include/dsp_frontend.h: dsp_bigru_backward).  params: the
    layer's weight_ih, weight_hh, bias_ih, bias_hh of the forward direction, then of the reverse one; x [T, B, in]: the
    layer's input as the kernel read it (dropout multipliers applied); out [T, B, 2 H]: the layer's output rows, forward |
    reverse, zero rows behind each column's end; da [T, B, 2, 4 H]: the gradients of the pre-activations, n_x | r | z | n_h;
    drop [T, B, in]: the multipliers of x, or None.  -> (dx -- the gradient of the layer's input in front of the
    multipliers -- then the eight parameter gradients in the order of ``params``); ``need`` (9 booleans) leaves out what is
    not wanted.  ``col_sum``: what forms the bias gradients' column sums (default ``a.sum(0)``)."""
    T, B, I = x.shape
    H = out.shape[2] // 2
    need = [True] * 9 if need is None else need
    col_sum = (lambda a: a.sum(0)) if col_sum is None else col_sum
    d2, x2 = da.reshape(T * B, 2, 4 * H), x.reshape(T * B, I)
    rzn = lambda v: torch.cat([v[H:], v[:H]], 0)            # rows n | r | z -> nn.GRU's r | z | n
    res = [None] * 9
    dx = None
    zero = out.new_zeros(1, B, H)
    for d in (0, 1):
        w_ih = params[4 * d]
        a_ih, a_hh = d2[:, d, :3 * H], d2[:, d, H:]          # [T B, 3 H]: (n_x | r | z) and (r | z | n_h)
        if need[0]:
            part = a_ih @ torch.cat([w_ih[2 * H:], w_ih[:2 * H]], 0)
            dx = part if dx is None else dx + part
        if need[1 + 4 * d]: res[1 + 4 * d] = rzn(a_ih.t() @ x2)
        if need[2 + 4 * d]:
            hp = torch.cat([zero, out[:-1, :, :H]], 0) if d == 0 else torch.cat([out[1:, :, H:], zero], 0)
            res[2 + 4 * d] = a_hh.t() @ hp.reshape(T * B, H)
        if need[3 + 4 * d]: res[3 + 4 * d] = rzn(col_sum(a_ih))
        if need[4 + 4 * d]: res[4 + 4 * d] = col_sum(a_hh)
    if need[0]:
        dx = dx.view(T, B, I)
        res[0] = dx * drop if drop is not None else dx
    return tuple(res)


class _DynEncTrain(torch.autograd.Function):
    """_DynEnc's native training path.  forward: dsp_bigru_forward_train (the forward kernels, which also save the tape and keep
    every layer's output rows); backward: per layer, top down, dsp_bigru_backward (the recurrence, one launch) and
    ``gru_param_grads``, whose dx is the next layer's incoming gradient.  Inputs: (module, T, d_len int32 [B], drop or None, x,
    the 8 n_layers parameters in nn.GRU's order); outputs: y [T, B, H] and h_n [2 n_layers, B, H], both differentiable."""

    @staticmethod
    def forward(ctx, mod, T, d_len, drop, x, *params):
        return _dynenc_train_forward(ctx, None, mod, T, d_len, drop, x, *params)

    @staticmethod
    def backward(ctx, g_y, g_hn):
        return _dynenc_train_backward(ctx, g_y, g_hn)


class _DynEncDeviceTrain(torch.autograd.Function):
    """``_DynEncTrain`` as the device-length path calls it (``_DynEnc._run_device_train``): the same kernels and products, the
    bias gradients' column sums formed by ``_ones_col_sum``."""

    @staticmethod
    def forward(ctx, mod, T, d_len, drop, x, *params):
        return _dynenc_train_forward(ctx, _ones_col_sum, mod, T, d_len, drop, x, *params)

    @staticmethod
    def backward(ctx, g_y, g_hn):
        return _dynenc_train_backward(ctx, g_y, g_hn)


class _DynEncWgradTrain(torch.autograd.Function):
    """``_DynEncTrain`` with the products behind the backward recurrence as native launches (``native_wgrad=True``;
    features/wgrad.py: ``gru_param_grads_native``) on either route.  Inputs: (module, T, d_len, drop or None, x, d_rows or None,
    the parameters).  ``d_rows``: a one-element int32 tensor on x's device, the row bound of those launches: they stop at
    clamp(d_rows[0], 1, T) rows.  It is read on the device when the kernels run and must hold the same value at the backward
    call.  None (the host-length route, whose T is max(lens) already): all T rows."""

    @staticmethod
    def forward(ctx, mod, T, d_len, drop, x, d_rows, *params):
        return _dynenc_train_forward(ctx, None, mod, T, d_len, drop, x, *params, wgrad=True, d_rows=d_rows)

    @staticmethod
    def backward(ctx, g_y, g_hn):
        return _dynenc_train_backward(ctx, g_y, g_hn)


def _dynenc_train_forward(ctx, col_sum, mod, T, d_len, drop, x, *params, wgrad=False, d_rows=None):
    from . import _native as nat
    ctx.set_materialize_grads(False)                     # an unused output hands None to backward, not a tensor of zeros
    B, H, L, dev = x.shape[1], mod.hidden_size, mod.gru.num_layers, x.device
    f32 = dict(dtype=torch.float32, device=dev)
    xc = x.detach().contiguous()
    handle, lib = mod._native_handle(dev), nat.load()
    nbytes = nat.c_i64(0)
    nat.check(lib.dsp_bigru_tape_bytes(handle, T, B, nat.C.byref(nbytes)))
    tape = torch.empty(nbytes.value // 4, **f32)
    y, hn = torch.empty(T, B, H, **f32), torch.empty(2 * L, B, H, **f32)
    nat.check(lib.dsp_bigru_forward_train(handle, xc.data_ptr(), T, B, d_len.data_ptr(), _ptr(drop),
                                          y.data_ptr(), hn.data_ptr(), tape.data_ptr(), nbytes.value,
                                          torch.cuda.current_stream(dev).cuda_stream))
    ctx.mod, ctx.tape_bytes, ctx.handle_key, ctx.has_drop = mod, nbytes.value, mod._handle_key, drop is not None
    ctx.col_sum = col_sum
    ctx.wgrad, ctx.has_rows = wgrad, d_rows is not None                   # (wgrad: one more input, d_rows, in front of the parameters)
    ctx.save_for_backward(xc, d_len, tape, *([drop] if drop is not None else []), *([d_rows] if ctx.has_rows else []), *params)
    return y, hn

def _dynenc_train_backward(ctx, g_y, g_hn):
    from . import _native as nat
    mod = ctx.mod
    mod._check_unmodified(ctx.handle_key)
    saved = ctx.saved_tensors
    xc, d_len, tape = saved[:3]
    drop = saved[3] if ctx.has_drop else None
    k = 4 if ctx.has_drop else 3
    d_rows = saved[k] if ctx.has_rows else None
    params = [p.detach() for p in saved[k + (1 if ctx.has_rows else 0):]]
    T, B, _ = xc.shape
    H, L, dev = mod.hidden_size, mod.gru.num_layers, xc.device
    grads = [None] * (1 + 8 * L)
    p0 = 6 if ctx.wgrad else 5                                               # the first parameter among the inputs
    pack = lambda: (None,) * 4 + (grads[0],) + (None,) * (p0 - 5) + tuple(grads[1:])
    if g_y is None and g_hn is None:
        return pack()
    gp = lambda g: None if g is None else g.to(torch.float32).contiguous()
    g, g_hn = gp(g_y), gp(g_hn)
    lib = nat.load()
    with torch.cuda.device(dev):
        off = nat.c_i64(0)
        rows = []
        for l in range(L):
            nat.check(lib.dsp_bigru_tape_rows(mod._handle, l, T, B, nat.C.byref(off)))
            rows.append(tape[off.value // 4:off.value // 4 + T * B * 2 * H].view(T, B, 2 * H))
        for l in range(L - 1, -1, -1):
            da = torch.empty(T, B, 2, 4 * H, dtype=torch.float32, device=dev)
            nat.check(lib.dsp_bigru_backward(mod._handle, l, T, B, d_len.data_ptr(), tape.data_ptr(), ctx.tape_bytes, _ptr(g),
                                             None if g_hn is None else g_hn[2 * l:].data_ptr(), da.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream))
            dl = drop[l - 1] if (drop is not None and l > 0) else None
            x_l = xc if l == 0 else (rows[l - 1] if dl is None else rows[l - 1] * dl)
            need = [l > 0 or ctx.needs_input_grad[4]] + list(ctx.needs_input_grad[p0 + 8 * l:p0 + 8 + 8 * l])
            if ctx.wgrad:
                from .wgrad import gru_param_grads_native
                res = gru_param_grads_native(params[8 * l:8 * l + 8], x_l, rows[l], da, dl, need, d_rows)
            else:
                res = gru_param_grads(params[8 * l:8 * l + 8], x_l, rows[l], da, dl, need, ctx.col_sum)
            grads[1 + 8 * l:9 + 8 * l] = res[1:]
            g = res[0]
        grads[0] = g
    return pack()


class RNNHead(nn.Module):
    """Same parameter names, shapes and forward pass as the reference's ``RNN`` (``enc.gru.*``, ``out.*``)."""

    def __init__(self, feat_size=39, hidden=200, layers=3, classes=20):
        super().__init__()
        self.enc = _DynEnc(feat_size, hidden, layers)
        self.out = nn.Linear(2 * hidden, classes)

    native_sums_default = False    # what ``native_sums=None`` picks on the device-length training path

    def forward(self, inp, len0, native_enc=None, device_len=False, device_grad=False, native_wgrad=None, rng=None, native_sums=None):
        """inp: [T, B, 39] (zero beyond each utterance's length), len0: lengths (numpy / list / tensor) -> [B, 20].
        ``rng`` is accepted and ignored: this head has no draw site.
        ``device_len=True``: len0 is a [B] int32 tensor on inp's device and is never read from the host (module docstring);
        ``device_grad=True`` with it serves a required gradient on that path.
        ``native_sums=True`` (with ``device_len=True, device_grad=True`` under a required gradient; it raises elsewhere): the
        whole backward off torch's reduction kernels -- ``native_wgrad`` on, the output layer's dW / db as native launches --
        so that a recorded step holds none.  The logits keep their bits."""
        _check_device_grad('RNNHead', device_len, device_grad)
        if device_len:
            needs_grad = _check_device_len('RNNHead', inp, len0, self, device_grad)
            sums = _want_sums('RNNHead', native_sums, self.native_sums_default, device_grad and needs_grad)
            native_wgrad = True if sums else native_wgrad
            d_len, _, info = head_length_info(len0, inp.shape[0], 1)
            y = self.enc(inp, d_len, device_len=True, device_grad=device_grad, native_wgrad=native_wgrad,
                         d_rows=info[0:1] if device_grad else None)             # [T, B, H], zeros behind each end
            return _out_layer(self.out, _pool_native(y, d_len, info[0:1], grad=device_grad), sums)
        _want_sums('RNNHead', native_sums, False, False)
        lens = torch.as_tensor(_lengths(len0))
        y = self.enc(inp, lens, native=native_enc, native_wgrad=native_wgrad)    # [max(len0), B, H], zeros behind each end
        avg = y.sum(0) / lens.to(inp.device, inp.dtype).unsqueeze(1)        # rnn_clf.py:29-30
        mx = y.max(0).values                                                # rnn_clf.py:31 (over the padded rows too)
        return self.out(torch.cat([avg, mx], dim=1))


def _pool_head(y, lens, out, attn=None, native_attn=None):
    """The pooled features of rnn_clf.py:68-72 / 107-115: sum over time / length (or the self-attention vector) || max over
    time -- both over the zero rows pad_packed_sequence leaves behind shorter utterances -- and the pre-dropout logits."""
    n = torch.as_tensor(np.asarray(lens), dtype=y.dtype, device=y.device)
    first = attn(y, native=native_attn) if attn is not None else y.sum(0) / n.unsqueeze(1)
    feat = torch.cat([first, y.max(0).values], dim=1)
    return out(feat), feat


class HRNNHead(nn.Module):
    """rnn_clf.HRNN (rnn_clf.py:36-77): 2-layer bidirectional GRU at the frame rate, every ``hir``-th output row
    (t = 0, hir, 2 hir, .. of max(len0) rows) into a 1-layer bidirectional GRU with lengths ceil(len0 / hir), pooled.
    The reference applies F.dropout(out, 0.2) to the logits in EVERY mode (training=True is F.dropout's default,
    rnn_clf.py:73): ``dropout=True`` does the same, ``False`` returns the logits in front of it.  forward -> (logits, feat).
    ``rng`` (a ``features.dropout.DeviceRng``): every draw -- the logits' and enc1's inter-layer one -- comes from the device
    generator at its site (features/dropout.py) instead of from torch; enc1 then needs its native training path."""
    hir = 10
    native_sums_default = False    # what ``native_sums=None`` picks on the device-length training path (``RNNHead.forward``)

    def __init__(self, feat_size=39):
        super().__init__()
        self.hidden_size = 200
        self.enc1 = _DynEnc(feat_size, 200, 2, dropout=0.2)
        self.enc2 = _DynEnc(200, 200, 1)
        self.out = nn.Linear(400, 20)

    def _levels(self, inp, len0, native_enc=None, native_wgrad=None, rng=None):
        len0 = _lengths(len0)
        len1 = (len0 + self.hir - 1) // self.hir                      # rnn_clf.py:52
        y = self.enc1(inp, len0, native=native_enc, native_wgrad=native_wgrad, rng=rng, rng_site=gru_site(0))[:, :, -self.hidden_size:]   # rnn_clf.py:58
        return self.enc2(y[0::self.hir], len1, native=native_enc, native_wgrad=native_wgrad, rng=rng, rng_site=gru_site(1)), len1         # rnn_clf.py:61-65

    def _levels_device(self, inp, len0, device_grad=False, native_wgrad=None, rng=None):
        """``_levels`` with the lengths on the device: all ceil(T / hir) picked rows go into enc2 -> (y2, len1, info)."""
        d_len, d_len1, info = head_length_info(len0, inp.shape[0], self.hir)
        rows0, rows1 = (info[0:1], info[1:2]) if device_grad else (None, None)   # max(len0) and ceil(max(len0) / hir), on the device
        y = self.enc1(inp, d_len, device_len=True, device_grad=device_grad, native_wgrad=native_wgrad, d_rows=rows0, rng=rng,
                      rng_site=gru_site(0))[:, :, -self.hidden_size:]
        return self.enc2(y[0::self.hir], d_len1, device_len=True, device_grad=device_grad, native_wgrad=native_wgrad, d_rows=rows1, rng=rng,
                         rng_site=gru_site(1)), d_len1, info

    def _forward_device(self, inp, len0, dropout, attn=None, device_grad=False, native_wgrad=None, rng=None, native_sums=None):
        needs_grad = _check_device_len(type(self).__name__, inp, len0, self, device_grad)
        sums = _want_sums(type(self).__name__, native_sums, self.native_sums_default, device_grad and needs_grad)
        native_wgrad = True if sums else native_wgrad
        y2, d_len1, info = self._levels_device(inp, len0, device_grad, native_wgrad, rng)
        rows = info[1:2]                                                        # ceil(max(len0) / hir), on the device
        if attn is None:
            feat = _pool_native(y2, d_len1, rows, grad=device_grad)
        else:
            feat = torch.cat([attn(y2, native=True, d_rows=rows, device_grad=device_grad, native_sums=sums),
                              _pool_native(y2, d_len1, rows, avg=False, grad=device_grad)], dim=1)
        out = _out_layer(self.out, feat, sums)
        return (_dropout(out, 0.2, rng, SITE_LOGITS) if dropout else out), feat

    def forward(self, inp, len0, dropout=True, native_enc=None, device_len=False, device_grad=False, native_wgrad=None, rng=None,
                native_sums=None):
        _check_device_grad(type(self).__name__, device_len, device_grad)
        if device_len:
            return self._forward_device(inp, len0, dropout, device_grad=device_grad, native_wgrad=native_wgrad, rng=rng,
                                        native_sums=native_sums)
        _want_sums(type(self).__name__, native_sums, False, False)
        y2, len1 = self._levels(inp, len0, native_enc, native_wgrad, rng)
        out, feat = _pool_head(y2, len1, self.out)
        return (_dropout(out, 0.2, rng, SITE_LOGITS) if dropout else out), feat


def _attn_needs_grad(x, module):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


def _attn_input_reason(x, params):
    """The reasons common to both attention blocks' native paths: device, dtype, parameter layout, library."""
    from . import _native as nat
    import os
    if x.dtype != torch.float32 or any(p.dtype != torch.float32 or p.device != x.device for p in params):
        return 'input and parameters must be float32 on one device'
    if not x.is_cuda:
        return 'the input is not on a GPU'
    if any(not p.is_contiguous() for p in params):
        return 'parameters must be contiguous'
    if not os.path.exists(nat.LIB_PATH):
        return f'{nat.LIB_PATH} is not built'
    return None


def _aligned16(t):
    """A dense fp32 tensor whose first element is 16-byte aligned (a copy where ``t`` is a view that is not)."""
    t = t.detach().to(torch.float32).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _SelfAttnTrain(torch.autograd.Function):
    """_SelfAttn's native training path.  forward: dsp_selfattn_pool_train_batch (the forward kernel, which also saves the weights
    w [T, B]); backward: dsp_selfattn_pool_backward_batch (one launch) and the sums over what it wrote.  Inputs: (y, attn.weight,
    attn.bias, v.weight, v.bias), read in place: autograd's version check on the saved tensors is what guards against a
    parameter written between forward and backward."""

    @staticmethod
    def forward(ctx, y, W, bW, v, c):
        return _selfattn_train_forward(ctx, y, W, bW, v, c, None)

    @staticmethod
    def backward(ctx, g_out):
        return _selfattn_train_backward(ctx, g_out, ctx.needs_input_grad, None)


def _selfattn_train_forward(ctx, y, W, bW, v, c, d_rows):
    """The forward of ``_SelfAttnTrain`` (d_rows None) and ``_SelfAttnRowsTrain``."""
    from . import _native as nat
    ctx.set_materialize_grads(False)
    T, B, H = y.shape
    dev = y.device
    yc = _aligned16(y)
    with torch.cuda.device(dev):
        out = torch.empty(B, H, dtype=torch.float32, device=dev)
        w = torch.empty(T, B, dtype=torch.float32, device=dev)
        lib, args = nat.load(), (yc.data_ptr(), T, B, H, W.data_ptr(), bW.data_ptr(), v.data_ptr(), c.data_ptr(), out.data_ptr(), w.data_ptr())
        st = torch.cuda.current_stream(dev).cuda_stream
        if d_rows is None:
            nat.check(lib.dsp_selfattn_pool_train_batch(*args, st))
        else:
            nat.check(lib.dsp_selfattn_pool_rows_train_batch(*args, d_rows.data_ptr(), st))
    ctx.save_for_backward(yc, w, W, bW, v)
    return out


def _selfattn_train_backward(ctx, g_out, need, d_rows, sums=False):
    """The backward of both: -> the gradients of (y, W, bW, v, c); ``need``: which of the five are wanted.  With ``d_rows`` the
    kernel leaves exact zeros behind the row count, so the sums over all T rows below are the sums over the block.  ``sums``:
    the four sums as native launches bounded by ``d_rows`` (features/wgrad.py) in place of torch's."""
    from . import _native as nat
    if g_out is None or not any(need):
        return (None,) * 5
    yc, w, W, bW, v = ctx.saved_tensors
    T, B, H = yc.shape
    dev = yc.device
    f32 = dict(dtype=torch.float32, device=dev)
    g = _aligned16(g_out)
    with torch.cuda.device(dev):
        g_y = torch.empty(T, B, H, **f32) if need[0] else None
        g_pre, g_e, gv = torch.empty(T, B, H, **f32), torch.empty(T, B, **f32), torch.empty(B, H, **f32)
        lib = nat.load()
        args = (yc.data_ptr(), T, B, H, W.data_ptr(), bW.data_ptr(), v.data_ptr(), w.data_ptr(), g.data_ptr(), _ptr(g_y), g_pre.data_ptr(),
                g_e.data_ptr(), gv.data_ptr())
        st = torch.cuda.current_stream(dev).cuda_stream
        if d_rows is None:
            nat.check(lib.dsp_selfattn_pool_backward_batch(*args, st))
        else:
            nat.check(lib.dsp_selfattn_pool_rows_backward_batch(*args, d_rows.data_ptr(), st))
        if sums:
            from .wgrad import rows_colsum, rows_gemm
            g_W = g_bW = None
            if need[1]:
                g_W, g_bW = rows_gemm(g_pre, yc, d_rows, colsum=True)
            elif need[2]:
                g_bW = rows_colsum(g_pre, None, d_rows)
            return (g_y, g_W, g_bW if need[2] else None,
                    rows_colsum(gv.unsqueeze(0)).reshape(1, H) if need[3] else None,
                    rows_colsum(g_e.unsqueeze(2), None, d_rows) if need[4] else None)
        return (g_y,
                _rows_gemm(g_pre, yc) if need[1] else None,
                _rows_sum(g_pre) if need[2] else None,
                gv.sum(0, keepdim=True) if need[3] else None,
                g_e.sum().reshape(1) if need[4] else None)


class _SelfAttnRowsTrain(torch.autograd.Function):
    """``_SelfAttnTrain`` over the first clamp(*d_rows, 1, T) rows of y, the count read on the device
    (dsp_selfattn_pool_rows_train_batch / dsp_selfattn_pool_rows_backward_batch).  Inputs: (y, d_rows, attn.weight, attn.bias,
    v.weight, v.bias); the parameter gradients are computed as ``_SelfAttnTrain`` computes them."""
    sums = False                   # ``_SelfAttnRowsSumsTrain``: the four sums of the backward as native launches

    @staticmethod
    def forward(ctx, y, d_rows, W, bW, v, c):
        ctx.d_rows = d_rows
        return _selfattn_train_forward(ctx, y, W, bW, v, c, d_rows)

    @staticmethod
    def backward(ctx, g_out):
        need = ctx.needs_input_grad
        res = _selfattn_train_backward(ctx, g_out, (need[0],) + tuple(need[2:]), ctx.d_rows, ctx._forward_cls.sums)
        return (res[0], None) + tuple(res[1:])


class _SelfAttnRowsSumsTrain(_SelfAttnRowsTrain):
    """``_SelfAttnRowsTrain`` whose backward records no reduction of torch's (``native_sums=True``)."""
    sums = True


class _SelfAttn(nn.Module):
    """layers.SelfAttn (layers.py:78-95): softmax over ALL rows of the padded output, zero rows included.

    Two paths compute the same thing: the torch chain below, and ``dsp_selfattn_pool_batch`` (csrc/kernels_attn.h: one launch,
    fp32, on the parameter tensors in place on the current stream).  ``native=True`` insists on the native one (and raises
    where it cannot run), ``native=False`` keeps torch, ``native=None`` picks native only where ``native_default`` says so.
    With a gradient required, ``native=True`` takes the native TRAINING path (``_SelfAttnTrain``: the forward kernel saves
    the weights, the backward is one launch, csrc/kernels_attn_bwd.h) in either mode -- the module has no mode-dependent
    behaviour --, and ``native=None`` keeps torch unless ``native_train_default`` is set."""
    native_default = False         # opt-in until DESIGN 7.9's timing shows it ahead at every size
    native_train_default = False   # what ``native=None`` picks when a gradient is required: torch, until DESIGN 7.10's timing decides

    def __init__(self, hidden_size):
        super().__init__()
        self.attn = nn.Linear(hidden_size, hidden_size)
        self.v = nn.Linear(hidden_size, 1)

    def native_supported(self, y, train=False):
        """Why the native path cannot serve ``y`` [T, B, H] (a string), or None when it can.  ``train``: the training path,
        for which a required gradient is no reason."""
        if not train and _attn_needs_grad(y, self):
            return 'a gradient is required (the native path is forward only)'
        why = _attn_input_reason(y, list(self.parameters()))
        if why is not None:
            return why
        T, H = y.shape[0], y.shape[2]
        if not (1 <= T <= 1024 and 4 <= H <= 256 and H % 4 == 0 and H == self.attn.in_features):
            return 'sizes out of range: T in [1, 1024], H a multiple of 4 in [4, 256]'
        return None

    def _run_native(self, y, d_rows=None):
        from . import _native as nat
        T, B, H = y.shape
        dev = y.device
        yc = y.detach().contiguous()                                            # (a copy of a view is held until the call returns)
        with torch.cuda.device(dev):
            out = torch.empty(B, H, dtype=torch.float32, device=dev)
            params = (self.attn.weight.data_ptr(), self.attn.bias.data_ptr(), self.v.weight.data_ptr(), self.v.bias.data_ptr())
            st = torch.cuda.current_stream(dev).cuda_stream
            if d_rows is None:
                nat.check(nat.load().dsp_selfattn_pool_batch(yc.data_ptr(), T, B, H, *params, out.data_ptr(), st))
            else:
                nat.check(nat.load().dsp_selfattn_pool_rows_batch(yc.data_ptr(), T, B, H, *params, out.data_ptr(), d_rows.data_ptr(), st))
        return out

    def _run_native_train(self, y):
        return _SelfAttnTrain.apply(y, self.attn.weight, self.attn.bias, self.v.weight, self.v.bias)

    def _run_torch(self, y):
        y = y.transpose(0, 1)                                                   # [B, T, H]
        w = torch.softmax(self.v(torch.tanh(self.attn(y))).squeeze(2), 1)       # [B, T]
        return torch.bmm(w.unsqueeze(1), y).squeeze(1)

    def forward(self, y, native=None, d_rows=None, device_grad=False, native_sums=False):
        """``d_rows``: a one-element int32 device tensor -- the softmax runs over the first min(*d_rows, T) rows of y only,
        the count read on the device (``dsp_selfattn_pool_rows_batch``); native, and forward only unless
        ``device_grad=True`` is given: a required gradient then takes ``_SelfAttnRowsTrain``.  ``native_sums=True``: that
        backward forms its four sums with native launches; it raises where that path does not run."""
        if device_grad and d_rows is None:
            raise ValueError('_SelfAttn: device_grad=True needs d_rows (it is the training form of the device-length path)')
        if native_sums and not (d_rows is not None and device_grad and _attn_needs_grad(y, self)):
            raise RuntimeError('_SelfAttn: native_sums=True cannot run: it serves the device-length training path (d_rows and '
                               'device_grad=True with a gradient required)')
        if d_rows is not None:
            needs_grad = device_grad and _attn_needs_grad(y, self)
            why = self.native_supported(y, train=needs_grad)
            if why is not None:
                raise RuntimeError(f'_SelfAttn: the native path cannot run: {why}')
            if needs_grad:
                fn = _SelfAttnRowsSumsTrain if native_sums else _SelfAttnRowsTrain
                return fn.apply(y, d_rows, self.attn.weight, self.attn.bias, self.v.weight, self.v.bias)
            return self._run_native(y, d_rows)
        if native is False:
            return self._run_torch(y)
        needs_grad = _attn_needs_grad(y, self)
        if native is None and not (self.native_train_default if needs_grad else self.native_default):
            return self._run_torch(y)                                           # (nothing to find out about the native path)
        why = self.native_supported(y, train=needs_grad)
        if why is None:
            return self._run_native_train(y) if needs_grad else self._run_native(y)
        if native:
            raise RuntimeError(f"_SelfAttn: the native {'training path (a gradient is required)' if needs_grad else 'path'} cannot run: {why}")
        return self._run_torch(y)


class HRNNAttHead(HRNNHead):
    """rnn_clf.HRNN_Att (rnn_clf.py:79-120): hir = 5, the attention vector in place of the average pool.  Parameter order
    as in the reference, whose __init__ re-assigns enc1 / enc2 / out created by HRNN.__init__ and appends attn."""
    hir = 5

    def __init__(self, feat_size=39):
        super().__init__(feat_size)
        self.attn = _SelfAttn(200)

    def forward(self, inp, len0, dropout=True, native_enc=None, native_attn=None, device_len=False, device_grad=False, native_wgrad=None,
                rng=None, native_sums=None):
        _check_device_grad('HRNNAttHead', device_len, device_grad)
        if device_len:
            return self._forward_device(inp, len0, dropout, self.attn, device_grad, native_wgrad, rng, native_sums)
        _want_sums('HRNNAttHead', native_sums, False, False)
        y2, len1 = self._levels(inp, len0, native_enc, native_wgrad, rng)
        out, feat = _pool_head(y2, len1, self.out, self.attn, native_attn)
        return (_dropout(out, 0.2, rng, SITE_LOGITS) if dropout else out), feat


class _LayerNorm(nn.Module):
    """layers.LayerNormalization (layers.py:125-143): unbiased std, eps added to sigma, and NO normalisation at all when
    the SECOND axis has one element."""

    def __init__(self, d, eps=1e-3):
        super().__init__()
        self.eps = eps
        self.a_2 = nn.Parameter(torch.ones(d))
        self.b_2 = nn.Parameter(torch.zeros(d))

    def forward(self, z):
        if z.size(1) == 1:
            return z
        mu, sigma = z.mean(-1, keepdim=True), z.std(-1, keepdim=True)
        return (z - mu) / (sigma + self.eps) * self.a_2 + self.b_2


class _MHA(nn.Module):
    """transformer.MultiHeadAttention + ScaledDotProductAttention (transformer.py:32-121) with the reference's quirks:
    tanh on the queries, temperature sqrt(d_model), and ``nn.Softmax()`` WITHOUT a dim on a 3-D tensor, i.e. a softmax over
    axis 0 -- across the (head x utterance) axis, not over the keys."""

    def __init__(self, n_head, d_model, d_k, d_v):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.w_qs = nn.Parameter(torch.empty(n_head, d_model, d_k))
        self.w_ks = nn.Parameter(torch.empty(n_head, d_model, d_k))
        self.w_vs = nn.Parameter(torch.empty(n_head, d_model, d_v))
        self.layer_norm = _LayerNorm(d_model)
        self.proj = nn.Linear(n_head * d_v, d_model)
        for w in (self.w_qs, self.w_ks, self.w_vs):
            nn.init.xavier_normal_(w)

    def forward(self, x):                                       # x: [T, B, d_model]
        q = x.transpose(0, 1)                                   # [B, T, d]
        B, T, d = q.shape
        rep = q.repeat(self.n_head, 1, 1).view(self.n_head, -1, d)
        qs = torch.bmm(rep, self.w_qs).view(-1, T, self.d_k)
        ks = torch.bmm(rep, self.w_ks).view(-1, T, self.d_k)
        vs = torch.bmm(rep, self.w_vs).view(-1, T, self.d_v)
        att = torch.bmm(torch.tanh(qs), ks.transpose(1, 2)) / float(np.power(d, 0.5))
        att = torch.softmax(att, 0)                             # transformer.py:40,58: implicit dim of a 3-D input is 0
        o = torch.bmm(att, vs)
        o = torch.cat(torch.split(o, B, dim=0), dim=-1)
        return self.layer_norm(self.proj(o) + q).transpose(0, 1)


class _PosFFN(nn.Module):
    """transformer.PositionwiseFeedForward (transformer.py:123-139): two 1 x 1 convolutions = two per-position linear maps."""

    def __init__(self, d, d_inner):
        super().__init__()
        self.w_1 = nn.Conv1d(d, d_inner, 1)
        self.w_2 = nn.Conv1d(d_inner, d, 1)
        self.layer_norm = _LayerNorm(d)

    def forward(self, x):
        o = self.w_2(torch.relu(self.w_1(x.transpose(1, 2)))).transpose(2, 1)
        return self.layer_norm(o + x)


def _ln_unit(r, eps):
    """The rows of layers.LayerNormalization in front of the gain: (r - mean) / (std_unbiased + eps)."""
    return (r - r.mean(-1, keepdim=True)) / (r.std(-1, keepdim=True) + eps)


def _ln_unit_ones(r, eps):
    """``_ln_unit`` with the two per-row statistics as products with a column of ones (library GEMMs) in place of torch's
    reductions, which ``native_sums=True`` keeps out of a recorded step whatever their shape.  The same formula:
    the mean, the unbiased variance of the centred row."""
    d = r.shape[-1]
    ones = r.new_ones(d, 1)
    c = r - (r @ ones) / d
    return c / (((c * c) @ ones / (d - 1)).sqrt() + eps)


def _rows_gemm(a, b):
    """a [T, B, m], b [T, B, n] -> a^T b [m, n] over all T B rows.  With a wide batch the product is one GEMM per time step,
    summed over t afterwards: a single [m, T B] x [T B, n] product has m n / tile outputs and runs on a handful of workgroups
    however long T B is.  The rule depends on the shapes alone: the same arguments give the same bits."""
    T, B, m = a.shape
    if B >= 64 and T > 1:
        return torch.bmm(a.transpose(1, 2), b).sum(0)
    return a.reshape(T * B, m).t() @ b.reshape(T * B, -1)


def _rows_sum(a):
    """a [T, B, n] -> the column sums [n], over t first: B n outputs keep the reduction parallel, n alone do not."""
    return a.sum(0).sum(0)


def _rows_sum_torch(a, x=None):
    """``_rows_sum`` of a, or of a * x."""
    return _rows_sum(a if x is None else a * x)


def _rows_gemm_native(a, b):
    from .wgrad import rows_gemm
    return rows_gemm(a, b)


def _rows_sum_native(a, x=None):
    from .wgrad import rows_colsum
    return rows_colsum(a, x)


def attn_param_grads(params, x, M, g_y, da, need=None, eps=1e-3, native=False):
    """The GEMMs and column sums behind the encoder layer's backward (include/dsp_frontend.h: dsp_attn_backward).  params: the
    13 tensors of ``_TransformerEncoder._params()``; x [T, B, d]: the layer's input; M [T, B, d]: the weighted sums
    sum_u A x_b[u] of the tape; g_y [T, B, d]: the gradient of the output; da: the seven row tensors g_r2, g_pre1, g_z1,
    g_r1, g_o, g_q', g_preQ, each [T, B, .].  The row-wise forward values (o, z1, h and the normalised rows) are recomputed
    from M and x; the B T T part is never run.  -> the 13 gradients in the order of ``params``; ``need`` (13 booleans) leaves
    out what is not wanted.  The gain and shift of a skipped LayerNorm (T == 1: the first, B == 1: the second) get None, as
    they get no gradient from autograd.  ``native``: every sum over the rows -- the products and the column sums -- as the native
    launches of features/wgrad.py (``rows_gemm``, ``rows_colsum``) in place of torch's GEMMs and reductions, and the row
    statistics of the two LayerNorms as products with ones (``_ln_unit_ones``); the recomputed forward values stay."""
    T, B, d = x.shape
    gemm, rsum, ln_unit = (_rows_gemm_native, _rows_sum_native, _ln_unit_ones) if native else (_rows_gemm, _rows_sum_torch, _ln_unit)
    need = [True] * 13 if need is None else list(need)
    res = [None] * 13
    if not any(need):
        return tuple(res)
    wq, wk, wv, a1, b1, wp, bp, w1, c1, w2, c2, a2, b2 = params
    g_r2, g_pre1, g_z1, g_r1, g_o, g_q, g_preq = da
    ln1, ln2 = T > 1, B > 1
    if need[0]: res[0] = gemm(x, g_preq).unsqueeze(0)
    if need[1]: res[1] = (gemm(g_q, torch.tanh(x @ wq[0])) / float(np.power(d, 0.5))).unsqueeze(0)
    if need[2]: res[2] = gemm(M, g_o).unsqueeze(0)
    if need[4] and ln1: res[4] = rsum(g_z1)
    if need[6]: res[6] = rsum(g_r1)
    if need[8]: res[8] = rsum(g_pre1)
    if need[10]: res[10] = rsum(g_r2)
    if need[12] and ln2: res[12] = rsum(g_y)
    if not (need[5] or need[7] or need[9] or (need[3] and ln1) or (need[11] and ln2)):
        return tuple(res)
    o = M @ wv[0]
    if need[5]: res[5] = gemm(g_r1, o)
    if not (need[7] or need[9] or (need[3] and ln1) or (need[11] and ln2)):
        return tuple(res)
    z1 = o @ wp.t() + bp + x
    if ln1:
        n1 = ln_unit(z1, eps)
        if need[3]: res[3] = rsum(g_z1, n1)
        z1 = n1 * a1 + b1
    if need[7]: res[7] = gemm(g_pre1, z1).unsqueeze(2)
    if need[9] or (need[11] and ln2):
        h = torch.relu(z1 @ w1[:, :, 0].t() + c1)
        if need[9]: res[9] = gemm(g_r2, h).unsqueeze(2)
        if need[11] and ln2:
            res[11] = rsum(g_y, ln_unit(h @ w2[:, :, 0].t() + c2 + z1, eps))
    return tuple(res)


def attn_tape_views(tape, T, B, d):
    """The tape of dsp_attn_forward_train (include/dsp_frontend.h) -> M [T, B, d], a view."""
    TP, DP = (T + 15) // 16 * 16, (d + 15) // 16 * 16
    off = 2 * B * TP * DP + 2 * TP * TP
    return tape[off:off + B * TP * DP].view(B, TP, DP)[:, :T, :d].transpose(0, 1)


class _AttnTrain(torch.autograd.Function):
    """_TransformerEncoder's native training path.  forward: dsp_attn_forward_train (the forward's three launches, which also
    save the tape); backward: dsp_attn_backward (four launches, three when x needs no gradient) and ``attn_param_grads``.
    Inputs: (module, x, the 13 parameters in module order); output: y [T, B, d_model]."""
    sums = False                   # ``_AttnSumsTrain``: the sums of ``attn_param_grads`` as native launches

    @staticmethod
    def forward(ctx, mod, x, *params):
        from . import _native as nat
        ctx.set_materialize_grads(False)                     # an unused output hands None to backward, not a tensor of zeros
        T, B, d = x.shape
        dev = x.device
        xc = x.detach().contiguous()
        with torch.cuda.device(dev):
            handle, lib = mod._native_handle(dev), nat.load()
            nbytes = nat.c_i64(0)
            nat.check(lib.dsp_attn_tape_bytes(handle, T, B, nat.C.byref(nbytes)))
            tape = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
            y = torch.empty(T, B, d, dtype=torch.float32, device=dev)
            nat.check(lib.dsp_attn_forward_train(handle, xc.data_ptr(), T, B, y.data_ptr(), tape.data_ptr(), nbytes.value,
                                                 torch.cuda.current_stream(dev).cuda_stream))
        ctx.mod, ctx.tape_bytes, ctx.handle_key = mod, nbytes.value, mod._handle_key
        ctx.save_for_backward(xc, tape, *params)
        return y

    @staticmethod
    def backward(ctx, g_y):
        from . import _native as nat
        mod = ctx.mod
        need_x, need = ctx.needs_input_grad[1], list(ctx.needs_input_grad[2:])
        if g_y is None or not (need_x or any(need)):
            return (None,) * 15
        mod._check_unmodified(ctx.handle_key)
        saved = ctx.saved_tensors
        xc, tape = saved[:2]
        params = [p.detach() for p in saved[2:]]
        T, B, d = xc.shape
        dev = xc.device
        f32 = dict(dtype=torch.float32, device=dev)
        g = g_y.detach().to(torch.float32).contiguous()
        lib = nat.load()
        with torch.cuda.device(dev):
            wb, db = nat.c_i64(0), nat.c_i64(0)
            nat.check(lib.dsp_attn_backward_bytes(mod._handle, T, B, nat.C.byref(wb), nat.C.byref(db)))
            work, da = torch.empty(wb.value // 4, **f32), torch.empty(db.value // 4, **f32)
            g_x = torch.empty(T, B, d, **f32) if need_x else None
            nat.check(lib.dsp_attn_backward(mod._handle, T, B, tape.data_ptr(), ctx.tape_bytes, g.data_ptr(), _ptr(g_x),
                                            da.data_ptr(), db.value, work.data_ptr(), wb.value,
                                            torch.cuda.current_stream(dev).cuda_stream))
            a = mod.slf_attn
            rows = [v.view(T, B, n) for v, n in zip(torch.split(da, [T * B * n for n in mod._da_widths()]), mod._da_widths())]
            grads = attn_param_grads(params, xc, attn_tape_views(tape, T, B, d), g, rows, need, a.layer_norm.eps, ctx._forward_cls.sums)
        return (None, g_x) + tuple(grads)


class _AttnSumsTrain(_AttnTrain):
    """``_AttnTrain`` whose backward records no reduction of torch's over the rows (``native_sums=True``)."""
    sums = True


class _TransformerEncoder(_NativeHandle, nn.Module):
    """transformer.EncoderLayer (transformer.py:16-30): ``_MHA`` then ``_PosFFN`` over x [T, B, d_model], all T rows as given.

    Two paths compute the same thing: the torch chain (any device, with gradients), and ``dsp_attn_forward``
    (csrc/kernels_attn.h: three launches that never hold a [B, T, T] tensor; fp32, n_head = 1, on the current stream).
    ``native=True`` insists on the native one (and raises where it cannot run), ``native=False`` keeps torch,
    ``native=None`` picks native only where ``native_default`` says so.
    With a gradient required, ``native=True`` takes the native TRAINING path (``_AttnTrain``): the forward saves a tape
    (``dsp_attn_forward_train``), the backward is four launches without a [B, T, T] tensor (``dsp_attn_backward``,
    csrc/kernels_attn_bwd.h) and the parameter gradients are GEMMs over the rows it leaves (``attn_param_grads``).  The module
    has no mode-dependent behaviour, so ``.train()`` and ``.eval()`` are both served.  ``native=None`` keeps torch whenever
    a gradient is required, unless ``native_train_default`` is set."""
    native_default = False         # opt-in until DESIGN 7.9's timing shows it ahead at every size
    native_train_default = False   # what ``native=None`` picks when a gradient is required: torch, until DESIGN 7.10's timing decides
    _lib = 'dsp_attn'

    def __init__(self, d_model, d_inner, n_head, d_k, d_v):
        super().__init__()
        self.d_model, self.d_inner = d_model, d_inner
        self.slf_attn = _MHA(n_head, d_model, d_k, d_v)
        self.pos_ffn = _PosFFN(d_model, d_inner)

    def _params(self):
        """Module order: w_qs, w_ks, w_vs, LN1 a_2, b_2, proj weight, bias, w_1 weight, bias, w_2 weight, bias, LN2 a_2, b_2."""
        return list(self.parameters())

    def _da_widths(self):
        """The widths of dsp_attn_backward's seven row tensors: g_r2, g_pre1, g_z1, g_r1, g_o, g_q', g_preQ."""
        d, a = self.d_model, self.slf_attn
        return [d, self.d_inner, d, d, a.d_v, d, a.d_k]

    def native_supported(self, x, train=False):
        """Why the native path cannot serve ``x`` [T, B, d_model] (a string), or None when it can.  ``train``: the training
        path, for which a required gradient is no reason."""
        a = self.slf_attn
        if a.n_head != 1:
            return f'n_head is {a.n_head}: the native path serves n_head = 1'
        if not train and _attn_needs_grad(x, self):
            return 'a gradient is required (the native path is forward only)'
        why = _attn_input_reason(x, self._params())
        if why is not None:
            return why
        ok4 = lambda v, hi: 4 <= v <= hi and v % 4 == 0
        if not (1 <= self.d_model <= 64 and ok4(a.d_k, 128) and ok4(a.d_v, 128) and ok4(self.d_inner, 256)
                and 1 <= x.shape[0] <= 1024 and x.shape[2] == self.d_model):
            return 'sizes out of range: d_model in [1, 64], d_k and d_v multiples of 4 in [4, 128], d_inner a multiple of 4 in [4, 256], T in [1, 1024]'
        if train and self.d_model < 2:
            return 'd_model is 1: training needs d_model in [2, 64] (the unbiased std of one element is not a number)'
        if a.layer_norm.eps != self.pos_ffn.layer_norm.eps:
            return 'the two layer norms differ in eps'
        return None

    def _descriptor(self, nat):
        a = self.slf_attn
        d = nat.AttnDesc(self.d_model, self.d_inner, a.n_head, a.d_k, a.d_v, a.layer_norm.eps)
        ps = self._params()
        d.d_params[:len(ps)] = [p.data_ptr() for p in ps]
        return d

    def _run_native(self, x):
        from . import _native as nat
        T, B, d = x.shape
        dev = x.device
        xc = x.detach().contiguous()                                            # (a copy of a view is held until the call returns)
        with torch.cuda.device(dev):
            handle = self._native_handle(dev)
            lib = nat.load()
            nbytes = nat.c_i64(0)
            nat.check(lib.dsp_attn_workspace_bytes(handle, T, B, nat.C.byref(nbytes)))
            work = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
            y = torch.empty(T, B, d, dtype=torch.float32, device=dev)
            nat.check(lib.dsp_attn_forward(handle, xc.data_ptr(), T, B, y.data_ptr(), work.data_ptr(), nbytes.value,
                                           torch.cuda.current_stream(dev).cuda_stream))
        return y

    def _run_native_train(self, x, sums=False):
        """The native training path: y attached to the autograd graph.  (The handle is created here, outside any capture.)"""
        return (_AttnSumsTrain if sums else _AttnTrain).apply(self, x, *self._params())

    def _run_torch(self, x):
        return self.pos_ffn(self.slf_attn(x))

    def run(self, x, native=None, refresh=False, native_sums=False):
        """``refresh``: what ``_native_handle`` is told on the native paths -- True keeps the handle across an optimiser step and
        repacks it in place (the ``device_grad=True`` path of ``TransformerHead``), 'always' repacks in any case.
        ``native_sums=True``: the native training path forms the sums of ``attn_param_grads`` with native launches; it raises
        where that path does not run."""
        needs_grad = _attn_needs_grad(x, self)
        if native_sums and not (native and needs_grad):
            raise RuntimeError('_TransformerEncoder: native_sums=True cannot run: it serves the native training path '
                               '(native=True with a gradient required)')
        if native is False:
            return self._run_torch(x)
        if native is None and not (self.native_train_default if needs_grad else self.native_default):
            return self._run_torch(x)                                           # (nothing to find out about the native path)
        why = self.native_supported(x, train=needs_grad)
        if why is None:
            if refresh:
                self._native_handle(x.device, refresh=refresh)                  # (the paths' own call then finds an equal key)
            return self._run_native_train(x, native_sums) if needs_grad else self._run_native(x)
        if native:
            raise RuntimeError(f"_TransformerEncoder: the native {'training path (a gradient is required)' if needs_grad else 'path'} cannot run: {why}")
        return self._run_torch(x)

    def forward(self, x, native=None, refresh=False, native_sums=False):
        return self.run(x, native, refresh, native_sums)


class TransformerHead(nn.Module):
    """rnn_clf.Transformer (rnn_clf.py:166-203): one self-attention block over the [T, B, 39] input, its output -- behind an
    F.dropout(.., 0.5) that is active in every mode (rnn_clf.py:184) -- concatenated with the input into a bidirectional GRU,
    every 5th row into a second one, pooled.  ``dropout=False`` leaves both F.dropout calls out.  -> (logits, feat, attn_out).
    ``rng`` (a ``features.dropout.DeviceRng``): both draws come from the device generator (sites 2 and 0, features/dropout.py)."""
    hir = 5
    native_sums_default = False    # what ``native_sums=None`` picks on the device-length training path (``RNNHead.forward``)

    def __init__(self):
        super().__init__()
        self.attn_enc = _TransformerEncoder(39, 200, 1, 100, 100)
        self.rnn_enc_1 = _DynEnc(78, 200, 1, dropout=0.2)
        self.rnn_enc_2 = _DynEnc(200, 200, 1)
        self.out = nn.Linear(400, 20)
        self.hidden_size = 200

    def forward(self, inp, len0, dropout=True, native_enc=None, native_attn=None, device_len=False, device_grad=False, native_wgrad=None,
                rng=None, native_sums=None):
        _check_device_grad('TransformerHead', device_len, device_grad)
        if device_len:
            needs_grad = _check_device_len('TransformerHead', inp, len0, self, device_grad)
            sums = _want_sums('TransformerHead', native_sums, self.native_sums_default, device_grad and needs_grad)
            native_wgrad = True if sums else native_wgrad
            d_len, d_len1, info = head_length_info(len0, inp.shape[0], self.hir)
            attn_out = self.attn_enc(inp, native=True, refresh=device_grad, native_sums=sums)
            a = _dropout(attn_out, 0.5, rng, SITE_ATTN) if dropout else attn_out
            rows0, rows1 = (info[0:1], info[1:2]) if device_grad else (None, None)
            y = self.rnn_enc_1(torch.cat([inp, a], 2), d_len, device_len=True, device_grad=device_grad, native_wgrad=native_wgrad,
                               d_rows=rows0, rng=rng, rng_site=gru_site(0))[:, :, -self.hidden_size:]
            y2 = self.rnn_enc_2(y[0::self.hir], d_len1, device_len=True, device_grad=device_grad, native_wgrad=native_wgrad, d_rows=rows1,
                                rng=rng, rng_site=gru_site(1))
            feat = _pool_native(y2, d_len1, info[1:2], grad=device_grad)
            out = _out_layer(self.out, feat, sums)
            return (_dropout(out, 0.2, rng, SITE_LOGITS) if dropout else out), feat, attn_out
        _want_sums('TransformerHead', native_sums, False, False)
        len0 = _lengths(len0)
        len1 = (len0 + self.hir - 1) // self.hir
        attn_out = self.attn_enc(inp, native=native_attn)
        a = _dropout(attn_out, 0.5, rng, SITE_ATTN) if dropout else attn_out
        # (the reference concatenates all 200 padded rows; the packed GRU then reads max(len0) of them)
        y = self.rnn_enc_1(torch.cat([inp, a], 2), len0, native=native_enc, native_wgrad=native_wgrad, rng=rng,
                           rng_site=gru_site(0))[:, :, -self.hidden_size:]
        y2 = self.rnn_enc_2(y[0::self.hir], len1, native=native_enc, native_wgrad=native_wgrad, rng=rng, rng_site=gru_site(1))
        out, feat = _pool_head(y2, len1, self.out)
        return (_dropout(out, 0.2, rng, SITE_LOGITS) if dropout else out), feat, attn_out


class _HMCell(nn.Module):
    """The parameters of hmrnn.HM_LSTMCell (hmrnn.py:60-71), same names, shapes, order and initial distribution."""

    def __init__(self, bottom_size, hidden_size, top_size, last_layer):
        super().__init__()
        self.hidden_size, self.last_layer = hidden_size, last_layer
        rows = 4 * hidden_size + 1
        self.U_11 = nn.Parameter(torch.empty(rows, hidden_size))
        if not last_layer:
            self.U_21 = nn.Parameter(torch.empty(rows, top_size))
        self.W_01 = nn.Parameter(torch.empty(rows, bottom_size))
        self.bias = nn.Parameter(torch.empty(rows))
        stdv = 1.0 / float(np.sqrt(hidden_size))
        for p in self.parameters():
            nn.init.uniform_(p, -stdv, stdv)

    def forward(self, a, c, h_bottom, h, h_top, z, z_bottom):
        """hmrnn.py:73-111, everything [rows, B].  Returns (h_new, c_new, z_new, z_hat); z_new carries the reference's
        straight-through gradient (``bound.backward`` hands the gradient on unchanged, hmrnn.py:37-45)."""
        H = self.hidden_size
        f_s = torch.mm(self.W_01, h_bottom)
        if not self.last_layer:
            f_s = f_s + z * torch.mm(self.U_21, h_top)
        else:
            f_s = f_s + torch.zeros_like(f_s)
        f_s = f_s + z_bottom * torch.mm(self.U_11, h) + self.bias.unsqueeze(1)
        f, i, o = torch.sigmoid(f_s[0:H]), torch.sigmoid(f_s[H:2 * H]), torch.sigmoid(f_s[2 * H:3 * H])
        g = torch.tanh(f_s[3 * H:4 * H])
        z_hat = torch.clamp((f_s[4 * H:4 * H + 1] * a + 1) / 2.0, min=0, max=1)                    # hard_sigm, hmrnn.py:25-28
        c_new = z * (i * g) + (1 - z) * (1 - z_bottom) * c + (1 - z) * z_bottom * (f * c + i * g)
        t = torch.tanh(c_new)
        h_new = z * o * t + (1 - z) * (1 - z_bottom) * h + (1 - z) * z_bottom * o * t
        z_new = (z_hat > 0.5).to(z_hat.dtype) + (z_hat - z_hat.detach())
        return h_new, c_new, z_new, z_hat


def hm_param_grads(params, x, state_in, h_1, h_2, z_1, dfs1, dfs2, need=None):
    """The GEMMs behind the backward recurrence (include/dsp_frontend.h: dsp_hmlstm_backward).  params: (U_11, U_21, W_01,
    bias of cell 1, U_11, W_01, bias of cell 2); x [T, B, I]; state_in: the flat h1 | c1 | z1 | h2 | c2 | z2 buffer or
    None (zeros); h_1 [B, T, H1], h_2 [B, T, H2], z_1 [B, T] (0 / 1, any dtype); dfs1 [T, B, 4 H1 + 1] and dfs2
    [T, B, 4 H2 + 1]: the gradients of the pre-activations f_s of every step.  -> (dx, then the seven parameter gradients
    in the order of ``params``); ``need`` (8 booleans) leaves out what is not wanted."""
    T, B, _ = x.shape
    H1, H2 = h_1.shape[2], h_2.shape[2]
    need = [True] * 8 if need is None else need
    dt = dfs1.dtype
    z1 = z_1.to(dt).t()                                                          # [T, B]
    if state_in is None:
        h1_0, h2_0, z1_0 = dfs1.new_zeros(1, B, H1), dfs1.new_zeros(1, B, H2), dfs1.new_zeros(1, B)
    else:
        h1_0 = state_in[:H1 * B].view(H1, B).t().unsqueeze(0)
        z1_0 = state_in[2 * H1 * B:(2 * H1 + 1) * B].view(1, B)
        h2_0 = state_in[(2 * H1 + 1) * B:(2 * H1 + 1 + H2) * B].view(H2, B).t().unsqueeze(0)
    h1t, h2t = h_1.transpose(0, 1), h_2.transpose(0, 1)                          # [T, B, H]
    h1p = torch.cat([h1_0.to(dt), h1t[:-1]], 0).reshape(T * B, H1)
    h2p = torch.cat([h2_0.to(dt), h2t[:-1]], 0).reshape(T * B, H2)
    z1p = torch.cat([z1_0.to(dt), z1[:-1]], 0).reshape(T * B, 1)
    d1, d2 = dfs1.reshape(T * B, -1), dfs2.reshape(T * B, -1)
    U11_1, U21, W01_1, _, U11_2, W01_2, _ = params
    out = [None] * 8
    if need[0]: out[0] = torch.matmul(dfs1, W01_1)
    if need[1]: out[1] = d1.t() @ h1p
    if need[2]: out[2] = (d1 * z1p).t() @ h2p
    if need[3]: out[3] = d1.t() @ x.reshape(T * B, -1)
    if need[4]: out[4] = d1.sum(0)
    if need[5]: out[5] = (d2 * z1.reshape(T * B, 1)).t() @ h2p
    if need[6]: out[6] = d2.t() @ h1t.reshape(T * B, H1)
    if need[7]: out[7] = d2.sum(0)
    return tuple(out)


class _HMLSTMTrain(torch.autograd.Function):
    """HMLSTM's native training path.  forward: dsp_hmlstm_forward_train (the forward kernel, which also saves the tape);
    backward: dsp_hmlstm_backward (the recurrence, one launch) and ``hm_param_grads``.  Inputs: (module, a, d_len int32 [B],
    d_rows or None, state_in or None, x, the seven parameters); outputs: h_1, h_2, last_h2 (differentiable) and z_1, z_2
    (uint8 [B, T]), z_hat, state_out (marked non-differentiable).
    ``d_rows``: a one-element int32 tensor on x's device, the row bound of both passes (dsp_hmlstm_forward_train_rows /
    dsp_hmlstm_backward_rows): the kernels stop at clamp(d_rows[0], 1, T) rows and leave exact zeros behind.  It is read on
    the device when the kernels run and must hold the same value at the backward call."""

    wgrad = False

    @staticmethod
    def forward(ctx, mod, a, d_len, d_rows, state_in, x, *params):
        from . import _native as nat
        ctx.set_materialize_grads(False)                     # an unused output hands None to backward, not a tensor of zeros
        T, B, _ = x.shape
        H1, H2 = mod.size_list
        dev = x.device
        f32 = dict(dtype=torch.float32, device=dev)
        xc = x.detach().contiguous()
        handle, lib = mod._native_handle(dev), nat.load()
        nbytes = nat.c_i64(0)
        nat.check(lib.dsp_hmlstm_tape_bytes(handle, T, B, nat.C.byref(nbytes)))
        tape = torch.empty(nbytes.value // 4, **f32)
        state_out = torch.empty((2 * H1 + 2 * H2 + 2) * B, **f32)
        h_1, h_2 = torch.empty(B, T, H1, **f32), torch.empty(B, T, H2, **f32)
        z_1, z_2 = torch.empty(B, T, dtype=torch.uint8, device=dev), torch.empty(B, T, dtype=torch.uint8, device=dev)
        z_hat, last = torch.empty(T, 2, B, **f32), torch.empty(B, H2, **f32)
        call = lib.dsp_hmlstm_forward_train if d_rows is None else lib.dsp_hmlstm_forward_train_rows
        rows = () if d_rows is None else (d_rows.data_ptr(),)
        nat.check(call(handle, xc.data_ptr(), T, B, a, d_len.data_ptr(), *rows, _ptr(state_in), state_out.data_ptr(),
                       h_1.data_ptr(), h_2.data_ptr(), z_1.data_ptr(), z_2.data_ptr(), z_hat.data_ptr(),
                       last.data_ptr(), tape.data_ptr(), nbytes.value, torch.cuda.current_stream(dev).cuda_stream))
        ctx.mod, ctx.a, ctx.tape_bytes, ctx.handle_key = mod, a, nbytes.value, mod._handle_key
        ctx.has_rows, ctx.has_state = d_rows is not None, state_in is not None
        ctx.save_for_backward(xc, d_len, tape, h_1, h_2, z_1, z_2, *([d_rows] if ctx.has_rows else []),
                              *([state_in] if ctx.has_state else []), *params)
        ctx.mark_non_differentiable(z_1, z_2, z_hat, state_out)
        return h_1, h_2, last, z_1, z_2, z_hat, state_out

    @staticmethod
    def backward(ctx, g_h1, g_h2, g_last, *_):
        from . import _native as nat
        saved = ctx.saved_tensors
        xc, d_len, tape, h_1, h_2, z_1, z_2 = saved[:7]
        k = 7
        d_rows = state_in = None
        if ctx.has_rows:
            d_rows, k = saved[k], k + 1
        if ctx.has_state:
            state_in, k = saved[k], k + 1
        params = saved[k:]
        mod = ctx.mod
        T, B, _ = xc.shape
        H1, H2 = mod.size_list
        dev = xc.device
        mod._check_unmodified(ctx.handle_key)
        need = [ctx.needs_input_grad[5]] + list(ctx.needs_input_grad[6:13])
        if g_h1 is None and g_h2 is None and g_last is None:
            return (None,) * 13
        gp = lambda g: None if g is None else g.to(torch.float32).contiguous()
        g_h1, g_h2, g_last = gp(g_h1), gp(g_h2), gp(g_last)
        with torch.cuda.device(dev):
            dfs1 = torch.empty(T, B, 4 * H1 + 1, dtype=torch.float32, device=dev)
            dfs2 = torch.empty(T, B, 4 * H2 + 1, dtype=torch.float32, device=dev)
            lib = nat.load()
            call = lib.dsp_hmlstm_backward if d_rows is None else lib.dsp_hmlstm_backward_rows
            rows = () if d_rows is None else (d_rows.data_ptr(),)
            nat.check(call(mod._handle, T, B, ctx.a, d_len.data_ptr(), *rows, _ptr(state_in), tape.data_ptr(),
                           ctx.tape_bytes, h_1.data_ptr(), h_2.data_ptr(), z_1.data_ptr(), z_2.data_ptr(),
                           _ptr(g_h1), _ptr(g_h2), _ptr(g_last), dfs1.data_ptr(), dfs2.data_ptr(),
                           torch.cuda.current_stream(dev).cuda_stream))
            if ctx._forward_cls.wgrad:
                from .wgrad import hm_param_grads_native
                grads = hm_param_grads_native([p.detach() for p in params], xc, state_in, h_1, h_2, z_1, dfs1, dfs2, need, d_rows)
            else:
                grads = hm_param_grads([p.detach() for p in params], xc, state_in, h_1, h_2, z_1, dfs1, dfs2, need)
        return (None, None, None, None, None) + grads


class _HMLSTMWgradTrain(_HMLSTMTrain):
    """``_HMLSTMTrain`` with the products behind the backward recurrence as native launches (``native_wgrad=True``;
    features/wgrad.py: ``hm_param_grads_native``).  With ``d_rows`` they stop at the same clamp(d_rows[0], 1, T) rows as the two
    passes: it is read on the device when the kernels run and must hold the same value at the backward call."""
    wgrad = True


class HMLSTMResult:
    """h_1 [B, T, H1], h_2 [B, T, H2], z_1 / z_2 [B, T, 1] (0. / 1.), hidden = (h1, c1, z1, h2, c2, z2) as [H, B] / [1, B]
    (hmrnn.py:153-154), z_hat [T, 2, B] (hard_sigm in front of the threshold: cell 1, cell 2) and, when lengths were given,
    last_h2 [B, H2] = h_2[b, len[b] - 1] (rnn_clf.py:140-143)."""
    __slots__ = ('h_1', 'h_2', 'z_1', 'z_2', 'hidden', 'z_hat', 'last_h2')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class HMLSTM(_NativeHandle, nn.Module):
    """hmrnn.HM_LSTM (hmrnn.py:114-154): two hierarchical-multiscale LSTM cells over a [T, B, input_size] sequence.
    Parameter names, shapes and order equal the reference's (``cell_1.U_11, cell_1.U_21, cell_1.W_01, cell_1.bias,
    cell_2.U_11, cell_2.W_01, cell_2.bias``): its state_dict loads.

    Two paths compute the same thing:
      * the torch step loop -- the restatement, on any device, with the reference's straight-through gradient; what
        ``native=None`` takes when a gradient is required (unless ``native_train_default`` is set);
      * the native one -- ``dsp_hmlstm_forward`` (csrc/kernels_hmlstm.h: one persistent HIP launch), on the tensors in
        place on the current stream; the default for CUDA/ROCm tensors when no gradient is required.  ``native=True``
        insists on it (and raises where it cannot run), ``native=False`` keeps the loop.
        With a gradient required, ``native=True`` takes the native TRAINING path (``_HMLSTMTrain``): the forward saves a
        tape (``dsp_hmlstm_forward_train``), the backward recurrence is one more persistent launch
        (``dsp_hmlstm_backward``, csrc/kernels_hmlstm_bwd.h) and the parameter gradients are GEMMs over what it leaves
        (``hm_param_grads``).  On that path h_1, h_2 and last_h2 carry the gradient to x and the seven parameters;
        z_1, z_2, z_hat and the final ``hidden`` are NOT differentiable (the loop's z carries the straight-through gradient
        to its consumers; nothing in this package consumes it), and an initial ``hidden`` that requires a gradient is a
        reason the native path cannot run.

    ``a`` is the slope of hard_sigm and is read at every call.  (The reference's cells copy ``a`` at construction,
    hmrnn.py:53,121-122, so its ``HMRNN.adjust_param`` -- which adds to ``HM_LSTM.a`` only -- never reaches them; here the
    one attribute is what both cells use.)"""
    native_train_default = False   # what ``native=None`` picks when a gradient is required: the loop, until DESIGN 7.4's timing shows the native path ahead
    native_wgrad_default = False   # what ``native_wgrad=None`` picks on the native training path: torch's GEMMs
    _lib = 'dsp_hmlstm'

    def __init__(self, a, input_size, size_list):
        super().__init__()
        self.a, self.input_size, self.size_list = float(a), int(input_size), [int(v) for v in size_list]
        self.cell_1 = _HMCell(self.input_size, self.size_list[0], self.size_list[1], False)
        self.cell_2 = _HMCell(self.size_list[0], self.size_list[1], None, True)

    # ---- native path ------------------------------------------------------------------------------------------------
    def _params(self):
        c1, c2 = self.cell_1, self.cell_2
        return [c1.U_11, c1.U_21, c1.W_01, c1.bias, c2.U_11, c2.W_01, c2.bias]

    def native_supported(self, x):
        """Why the native path cannot serve ``x`` (a string), or None when it can."""
        from . import _native as nat
        import os
        if not x.is_cuda:
            return 'the input is not on a GPU'
        if x.dtype != torch.float32 or any(p.dtype != torch.float32 or p.device != x.device for p in self._params()):
            return 'input and parameters must be float32 on one device'
        if any(v < 4 or v > 256 or v % 4 for v in [self.input_size] + self.size_list):
            return 'sizes must be multiples of 4 in [4, 256]'
        if not os.path.exists(nat.LIB_PATH):
            return f'{nat.LIB_PATH} is not built'
        return None

    def _descriptor(self, nat):
        return nat.HmlstmDesc(self.input_size, self.size_list[0], self.size_list[1], 0, *[p.data_ptr() for p in self._params()])

    def _native_handle(self, dev, refresh=False):
        if any(not p.is_contiguous() for p in self._params()):
            from . import _native as nat
            raise nat.DspError('HMLSTM: parameters must be contiguous')
        return super()._native_handle(dev, refresh)

    def _run_native(self, x, hidden, lens, want_seq=True, d_len=None, last_only=False):
        """``d_len``: the lengths as a [B] int32 tensor on x's device, read in place (``lens`` is then ignored).
        ``last_only``: ``last_h2`` is the one output asked for -- the kernel then stops every 16-column slice at its longest
        length instead of running all T rows."""
        from . import _native as nat
        T, B, _ = x.shape
        H1, H2 = self.size_list
        dev = x.device
        x = x.detach().contiguous()
        with torch.cuda.device(dev):
            handle = self._native_handle(dev)
            f32 = dict(dtype=torch.float32, device=dev)
            state_in = None if hidden is None else _pack_state(hidden, H1, H2, B, **f32)
            want_seq = want_seq and not last_only
            state_out = None if last_only else torch.empty((2 * H1 + 2 * H2 + 2) * B, **f32)
            h_1 = torch.empty(B, T, H1, **f32) if want_seq else None
            h_2 = torch.empty(B, T, H2, **f32) if want_seq else None
            z_1 = torch.empty(B, T, dtype=torch.uint8, device=dev) if want_seq else None
            z_2 = torch.empty(B, T, dtype=torch.uint8, device=dev) if want_seq else None
            z_hat = None if last_only else torch.empty(T, 2, B, **f32)
            last = None
            if d_len is None and lens is not None:
                d_len = torch.as_tensor(_lengths(lens), dtype=torch.int32).to(dev)
            if d_len is not None:
                last = torch.empty(B, H2, **f32)
            nat.check(nat.load().dsp_hmlstm_forward(handle, x.data_ptr(), T, B, float(self.a), _ptr(d_len), _ptr(state_in),
                                                    _ptr(state_out), _ptr(h_1), _ptr(h_2), _ptr(z_1), _ptr(z_2), _ptr(z_hat),
                                                    _ptr(last), torch.cuda.current_stream(dev).cuda_stream))
        hid = None if last_only else _split_state(state_out, H1, H2, B)
        zf = lambda z: None if z is None else z.to(torch.float32).unsqueeze(2)
        return HMLSTMResult(h_1=h_1, h_2=h_2, z_1=zf(z_1), z_2=zf(z_2), hidden=hid, z_hat=z_hat, last_h2=last)

    def _run_native_train(self, x, hidden, lens, d_len=None, d_rows=None, wgrad=False):
        """The native training path: the same HMLSTMResult, h_1 / h_2 / last_h2 attached to the autograd graph.
        ``d_len`` (``device_grad=True``): the lengths as a [B] int32 tensor on x's device, read in place; ``last_h2`` is then
        the only field returned, and the handle survives an optimiser step (``refresh=True``).  All T rows run on this path
        -- the forward-only ``last_only`` shortcut does not apply: the backward recurrence reads the tape of every row it
        runs -- unless ``d_rows`` (with ``d_len``) gives both passes one row bound to stop at (``_HMLSTMTrain``)."""
        T, B, _ = x.shape
        H1, H2 = self.size_list
        dev = x.device
        with torch.cuda.device(dev):
            self._native_handle(dev, refresh=d_len is not None)
            f32 = dict(dtype=torch.float32, device=dev)
            state_in = None if hidden is None else _pack_state(hidden, H1, H2, B, **f32)
            train = _HMLSTMWgradTrain if wgrad else _HMLSTMTrain          # (``wgrad``: the products as native launches)
            if d_len is not None:
                last = train.apply(self, float(self.a), d_len, d_rows, state_in, x, *self._params())[2]
                return HMLSTMResult(last_h2=last)
            if lens is not None:
                d_len = torch.as_tensor(_lengths(lens), dtype=torch.int32).to(dev)
            else:
                d_len = torch.full((B,), T, dtype=torch.int32, device=dev)
            h_1, h_2, last, z_1, z_2, z_hat, state_out = train.apply(self, float(self.a), d_len, None, state_in, x, *self._params())
        hid = _split_state(state_out, H1, H2, B)
        zf = lambda z: z.to(torch.float32).unsqueeze(2)
        return HMLSTMResult(h_1=h_1, h_2=h_2, z_1=zf(z_1), z_2=zf(z_2), hidden=hid, z_hat=z_hat, last_h2=last if lens is not None else None)

    # ---- torch step loop (hmrnn.py:124-154) -------------------------------------------------------------------------------
    def _run_torch(self, x, hidden, lens):
        T, B, _ = x.shape
        H1, H2 = self.size_list
        zeros = lambda n: torch.zeros(n, B, dtype=x.dtype, device=x.device)
        if hidden is None:
            h1, c1, z1, h2, c2, z2 = zeros(H1), zeros(H1), zeros(1), zeros(H2), zeros(H2), zeros(1)
        else:
            h1, c1, z1, h2, c2, z2 = hidden
        one = torch.ones(1, B, dtype=x.dtype, device=x.device)
        hs1, hs2, zs1, zs2, zh = [], [], [], [], []
        for t in range(T):
            h1, c1, z1, zh1 = self.cell_1(self.a, c1, x[t].t(), h1, h2, z1, one)
            h2, c2, z2, zh2 = self.cell_2(self.a, c2, h1, h2, None, z2, z1)
            hs1.append(h1.t()); hs2.append(h2.t()); zs1.append(z1.t()); zs2.append(z2.t())
            zh.append(torch.cat([zh1, zh2], 0))
        h_2 = torch.stack(hs2, dim=1)
        last = None
        if lens is not None:
            idx = torch.as_tensor(_lengths(lens)).clamp(1, T) - 1
            last = h_2[torch.arange(B, device=x.device), idx.to(x.device)]
        return HMLSTMResult(h_1=torch.stack(hs1, dim=1), h_2=h_2, z_1=torch.stack(zs1, dim=1), z_2=torch.stack(zs2, dim=1),
                            hidden=(h1, c1, z1, h2, c2, z2), z_hat=torch.stack(zh).detach(), last_h2=last)

    def run(self, x, hidden=None, lens=None, native=None, device_len=False, device_grad=False, d_rows=None, native_wgrad=None):
        """Everything the forward pass yields, as an HMLSTMResult.  x: [T, B, input_size].
        ``device_len=True``: ``lens`` is a [B] int32 tensor on x's device with entries in [1, T] and stays there; the native
        forward yields ``last_h2`` alone (every other field is None), which lets each 16-column slice stop at its longest
        length instead of running all T rows.
        Forward only: a required gradient, or anything else the native path cannot serve, raises -- unless
        ``device_grad=True`` is given as well: a required gradient then takes the native training path with the lengths read
        on the device.  ``last_h2`` is still the only field returned; the handle is refreshed in place after an optimiser
        step instead of rebuilt.  The per-slice stop does not apply there, because the forward and the backward recurrence
        must agree on the rows the tape holds: without ``d_rows`` all T rows run, and with it -- a one-element int32 tensor on
        x's device holding a row count no smaller than the longest length, such as ``head_length_info(...)[2][0:1]`` -- both
        passes stop at clamp(d_rows[0], 1, T) rows, read on the device, with the same ``last_h2`` and the same gradients (a
        smaller count cuts the lengths to it).  ``d_rows`` serves the training path only and needs ``device_grad=True``.
        ``native_wgrad=True``: on the native training path -- either route -- the products behind the backward recurrence
        (``hm_param_grads``) run as native launches (features/wgrad.py), bounded by ``d_rows`` where it is given; anywhere else
        it raises.  ``native_wgrad=None`` takes ``native_wgrad_default``."""
        _check_device_grad('HMLSTM', device_len, device_grad)
        if d_rows is not None:
            if not device_grad:
                raise ValueError('HMLSTM: d_rows needs device_len=True, device_grad=True (it bounds the native training path)')
            _check_rows_word('HMLSTM', d_rows, x)
        if device_len:
            needs_grad = _check_device_len('HMLSTM', x, lens, self, device_grad)
            if torch.is_grad_enabled() and hidden is not None and any(v.requires_grad for v in hidden):
                raise RuntimeError('HMLSTM: device_len=True cannot run: the initial hidden requires a gradient')
            why = self.native_supported(x)
            if why is not None:
                raise RuntimeError(f'HMLSTM: the native path cannot run: {why}')
            wgrad = _want_wgrad('HMLSTM', native_wgrad, self.native_wgrad_default, needs_grad)
            if needs_grad:
                return self._run_native_train(x, hidden, None, d_len=lens.contiguous(), d_rows=d_rows, wgrad=wgrad)
            if device_grad:
                self._native_handle(x.device, refresh=True)
            return self._run_native(x, hidden, None, d_len=lens.contiguous(), last_only=True)
        hidden_grad = torch.is_grad_enabled() and hidden is not None and any(v.requires_grad for v in hidden)
        needs_grad = hidden_grad or (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())))
        if needs_grad and native is None and not self.native_train_default:
            _want_wgrad('HMLSTM', native_wgrad, False, False)
            return self._run_torch(x, hidden, lens)
        why = 'the initial hidden requires a gradient' if hidden_grad else self.native_supported(x)
        if native is None:
            native = why is None
        if native:
            if why is not None:
                raise RuntimeError(f'HMLSTM: the native path cannot run: {why}')
            wgrad = _want_wgrad('HMLSTM', native_wgrad, self.native_wgrad_default, needs_grad)
            return self._run_native_train(x, hidden, lens, wgrad=wgrad) if needs_grad else self._run_native(x, hidden, lens)
        _want_wgrad('HMLSTM', native_wgrad, False, False)
        return self._run_torch(x, hidden, lens)

    def forward(self, x, hidden=None, lens=None, native=None):
        """-> (h_1, h_2, z_1, z_2, hidden), the reference's return value (hmrnn.py:154)."""
        r = self.run(x, hidden, lens, native)
        return r.h_1, r.h_2, r.z_1, r.z_2, r.hidden


class HMRNNHead(nn.Module):
    """rnn_clf.HMRNN (rnn_clf.py:122-164), the classifier model.py:110 ships: a 2-layer bidirectional GRU (halves summed, 200
    wide), F.dropout(.., 0.2) on its output in EVERY mode (rnn_clf.py:138), the HM-LSTM over the max(len0) rows of it, and
    feat = [sum / len | max over those rows, zero rows included | h_2 at len - 1] -> Linear(600, 20) -> F.dropout(.., 0.2).
    ``dropout=False`` returns the values in front of both dropouts.  forward -> (logits, feat).  Parameter names and order
    equal the real class's ``named_parameters()``.  ``rng`` (a ``features.dropout.DeviceRng``): both draws come from the device
    generator (sites 1 and 0, features/dropout.py)."""
    hir = 5
    native_sums_default = False    # what ``native_sums=None`` picks on the device-length training path (``RNNHead.forward``)

    def __init__(self, feat_size=39):
        super().__init__()
        self.hidden_size = 200
        self.enc1 = _DynEnc(feat_size, 200, 2)
        self.enc2 = HMLSTM(1.0, 200, [200, 200])
        self.out = nn.Linear(600, 20)

    def forward(self, inp, len0, dropout=True, native=None, native_enc=None, device_len=False, device_grad=False, native_wgrad=None,
                rng=None, native_sums=None):
        _check_device_grad('HMRNNHead', device_len, device_grad)
        if device_len:
            needs_grad = _check_device_len('HMRNNHead', inp, len0, self, device_grad)
            sums = _want_sums('HMRNNHead', native_sums, self.native_sums_default, device_grad and needs_grad)
            native_wgrad = True if sums else native_wgrad
            d_len, _, info = head_length_info(len0, inp.shape[0], 1)
            enc = self.enc1(inp, d_len, device_len=True, device_grad=device_grad, native_wgrad=native_wgrad,
                            d_rows=info[0:1] if device_grad else None, rng=rng, rng_site=gru_site(0))   # [T, B, 200], zeros behind each end
            if dropout:
                enc = _dropout(enc, 0.2, rng, SITE_HM_ENC)
            last = self.enc2.run(enc, None, lens=d_len, device_len=True, device_grad=device_grad, native_wgrad=native_wgrad,
                                 d_rows=info[0:1] if device_grad else None).last_h2      # both passes stop at max(len0)
            feat = torch.cat([_pool_native(enc, d_len, info[0:1], grad=device_grad), last], dim=1)
            out = _out_layer(self.out, feat, sums)
            return (_dropout(out, 0.2, rng, SITE_LOGITS) if dropout else out), feat
        _want_sums('HMRNNHead', native_sums, False, False)
        len0 = _lengths(len0)
        enc = self.enc1(inp, len0, native=native_enc, native_wgrad=native_wgrad, rng=rng, rng_site=gru_site(0))   # [max(len0), B, 200]
        if dropout:
            enc = _dropout(enc, 0.2, rng, SITE_HM_ENC)
        last = self.enc2.run(enc, None, lens=len0, native=native, native_wgrad=native_wgrad).last_h2     # rnn_clf.py:139-143
        n = torch.as_tensor(len0, dtype=enc.dtype, device=enc.device)
        feat = torch.cat([enc.sum(0) / n.unsqueeze(1), enc.max(0).values, last], dim=1)
        out = self.out(feat)
        return (_dropout(out, 0.2, rng, SITE_LOGITS) if dropout else out), feat

    def adjust_param(self):
        """rnn_clf.py:163-164: the slope schedule, +0.5 per call (see HMLSTM on what the reference's own cells read)."""
        self.enc2.a += 0.5


def fill_parameters(module, seed):
    """Deterministic weights for parity fixtures: every parameter, in ``named_parameters()`` order, drawn from
    numpy's ``default_rng(seed)`` as uniform(-0.08, 0.08) float32 -- the same call fills the reference class in
    tests/golden/make_rnn_golden.py, so both sides hold identical weights without a multi-megabyte fixture."""
    rng = np.random.default_rng(seed)
    names = []
    with torch.no_grad():
        for name, p in module.named_parameters():
            v = rng.uniform(-0.08, 0.08, size=tuple(p.shape)).astype(np.float32)
            p.copy_(torch.from_numpy(v))
            names.append(name)
    return names


def __getattr__(name):
    """``AdvHRNNHead`` and ``gradient_reverse`` live in features/adversarial.py (which builds on ``HRNNHead`` above) and are
    re-exported from here, resolved on first use so that either module may be imported first."""
    if name in ('AdvHRNNHead', 'gradient_reverse'):
        from . import adversarial
        return getattr(adversarial, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
