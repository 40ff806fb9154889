"""One training step of a classifier head on raw clips without a host round trip: the training twin of
``ensemble.EnsembleBatch`` for one sample rate (model.py:137-147: ``get_batch_full(feat, augment=True)``, the classifier,
``F.cross_entropy``, ``backward``).

* ``TrainBatch.run`` queues the augmented front end (``ModelFeatureBatch.enqueue`` with the endpoint jitter of model.py:54-60
  read from device memory), the head with ``device_len=True, device_grad=True`` and the loss on torch's current stream.
  ``len0`` never leaves the device and nothing is synchronised; the caller calls ``loss.backward()``.
* ``TrainBatch.capture`` records a refresh of every native handle of the head, the front end, the forward, the loss and the
  backward into ONE HIP graph.  ``replay()`` serves new clips, labels and jitter written into the captured buffers and leaves
  the gradients in ``.grad`` tensors the graph owns.  Without ``optimizer=`` the optimiser step stays the caller's, eager,
  after ``replay()``: it writes the parameters in place, and the refresh at the head of the next replay repacks them.  With
  ``optimizer=`` a ``features.optim.DeviceAdam`` over the head's trainable parameters, its step is recorded behind the backward:
  the whole of model.py:137-149 is one replay.
* ``AdvTrainBatch`` is the same step for ``features.adversarial.AdvHRNNHead`` (adv_model.py:33-48): speakers beside the labels,
  ``loss = CE(labels) + CE(speakers)``, the discriminator optionally as one native call (``native_disc=True``).
* With ``rng=`` a ``features.dropout.DeviceRng`` among the head's keywords the dropouts are drawn by the device generator, and
  the chain begins with ``rng.advance()`` -- recorded too, so every replay draws a new step's multipliers, the ones an eager
  ``run`` from the same state draws.  ``capture`` leaves the generator's state as it found it.
"""
from __future__ import annotations

import types

import numpy as np

from . import _native as nat
from .batch import _is_device_tensor, _wave_dtype_of


# Where ``TrainBatch.capture`` records: head class -> batch sizes at which tests/test_gpu_train_capture.py (B >= 32) and
# tests/test_gpu_device_train.py (B = 5) compare a second replay with the eager step, bit for bit.
CAPTURE_VERIFIED = {'RNNHead': (32, 512), 'HRNNHead': (32, 512), 'HRNNAttHead': (32, 512), 'TransformerHead': (32, 512),
                    'HMRNNHead': (5, 32, 512)}
# The same for ``AdvTrainBatch.capture``: the sizes at which tests/test_gpu_adv.py compares three replays with three eager steps.
# A table of its own: every entry of CAPTURE_VERIFIED is a head that the label-only ``TrainBatch`` trains (and
# tests/test_gpu_train_capture.py runs each of them through it), and under a label-only loss the discriminator's parameters
# receive no gradient, so a ``TrainBatch`` over an ``AdvHRNNHead`` is refused by ``capture`` like any other unverified pair.
ADV_CAPTURE_VERIFIED = {'AdvHRNNHead': (32, 512)}


def _advance_rng(head_kwargs):
    """The head of every chain: with an ``rng`` among the head's keywords, one step of the generator (a launch, recordable)."""
    rng = head_kwargs.get('rng')
    if rng is not None:
        rng.advance()


def _logits_of(out):
    return out[0] if isinstance(out, (tuple, list)) else out


def _loss_spec(loss, metrics):
    """The ``loss=`` / ``metrics=`` keywords of ``run`` and ``capture`` -> (native?, metrics); refusals need no device."""
    if loss not in ('torch', 'native'):
        raise ValueError(f"loss must be 'torch' or 'native', got {loss!r}")
    if metrics is not None:
        if loss != 'native':
            raise ValueError("metrics= needs loss='native': the device metrics are updated by the native loss call")
        from .metrics import Metrics
        if not isinstance(metrics, Metrics):
            raise TypeError(f'metrics must be a features.metrics.Metrics, not {type(metrics).__name__}')
    return loss == 'native', metrics


class _CapturedStep:
    """What ``TrainBatch.capture`` returns.  ``replay()`` re-runs the recorded step on whatever the captured buffers hold now
    and returns ``result`` (loss, logits, inp, len0, n_clamped: device tensors, valid after the current stream's work; nothing
    is synchronised).  ``grads``: the gradient tensors the graph owns, in the order of ``params``; every replay OVERWRITES
    them (it does not accumulate) and makes them the parameters' ``.grad`` again, so an ``optimizer.zero_grad()`` between
    replays -- which drops ``.grad`` -- costs nothing and loses nothing.  ``hold``: every buffer the graph's kernels touch
    that the result does not already keep alive.  ``optimizer``: the ``DeviceAdam`` whose step the graph carries, or None; with
    one, a replay also binds the optimiser to ``grads`` (a recorded launch in front of the step, so an eager ``step()`` on other
    gradients in between does not mislead it), updates the parameters and the optimiser's state, and ``replay()`` bumps the
    parameters' version counters afterwards.  ``rng``: the ``DeviceRng`` whose state the recorded draws read (and whose
    ``advance`` the graph carries), or None; kept alive here."""

    def __init__(self, graph, result, params, grads, hold, optimizer=None, rng=None):
        self.graph, self.result, self.params, self.grads, self.hold, self.optimizer = graph, result, params, grads, hold, optimizer
        self.rng = rng
        # a capture with ``capacity=``: where the next batch's offsets go before a replay, and the offsets kernel's status word
        self.sample_offsets = self.status = None
        self.census = None         # ``capture(..., census=True)`` or a capture outside the table: the recorded graph's census

    def replay(self):
        self.graph.replay()
        for p, g in zip(self.params, self.grads):
            p.grad = g
        if self.optimizer is not None:
            self.optimizer._after_replay(self.grads)
        return self.result


class TrainBatch:
    """model.py:137-147 for a batch of raw clips of one sample rate, device-resident.

    ``head``: one of features/classifier.py's heads in training mode (it is called with ``device_len=True,
    device_grad=True``; further keywords -- ``dropout=False`` and the like -- go through ``run`` / ``capture``)."""

    _verified = CAPTURE_VERIFIED       # what ``capture`` serves: head class -> batch sizes

    def __init__(self, rate, head, frame=0.03, step=0.01):
        from .model_glue import ModelFeatureBatch
        self.rate, self.head = rate, head
        self.features = ModelFeatureBatch(rate, frame=frame, step=step)
        self._layouts = {}

    def draw_jitter(self, n_utt, rng):
        """The endpoint offsets of model.py:54-60 for a batch (``ModelFeatureBatch.draw_jitter``): int64 [B, 2]."""
        return self.features.draw_jitter(n_utt, rng)

    def _layout(self, so):
        """The pipeline layout of this batch shape, owned by this object (a few shapes are kept, the most recently used last)."""
        key = (nat.current_device(), so.tobytes())
        lay = self._layouts.pop(key, None)
        if lay is None:
            lay = self.features.pipe.prepare(so, 0)
            while len(self._layouts) >= 4:
                self._layouts.pop(next(iter(self._layouts)))
        self._layouts[key] = lay
        return lay

    def _m0(self, lay, dev):
        import torch
        return torch.empty((max(lay.frames_bound, 1), self.features.pipe.features.C), dtype=torch.float32, device=dev)

    @staticmethod
    def _labels(labels, B, dev):
        import torch
        if not torch.is_tensor(labels):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64))
        labels = labels.to(device=dev, dtype=torch.int64)
        if tuple(labels.shape) != (B,):
            raise ValueError(f'labels must be [B] = [{B}], got {tuple(labels.shape)}')
        return labels

    @staticmethod
    def _jitter(jitter, B, dev):
        import torch
        if jitter is None:
            return None
        if not torch.is_tensor(jitter):
            jitter = torch.from_numpy(np.ascontiguousarray(jitter, dtype=np.int64))
        jitter = jitter.to(device=dev, dtype=torch.int64).contiguous()
        if tuple(jitter.shape) != (B, 2):
            raise ValueError(f'jitter must be [B, 2] = [{B}, 2], got {tuple(jitter.shape)}')
        return jitter

    def _chain(self, clips, lay, m0, labels, d_jit, head_kwargs, alias=None, spec=(False, None)):
        """Front end, head, loss: launches on torch's current stream, nothing synchronised, no device memory read from the
        host.  ``alias``: name -> tensor to stand in for the head's parameters during the call (``capture``)."""
        import torch
        _advance_rng(head_kwargs)
        mfb, dev, B = self.features, clips.device, lay.n_utt
        inp = torch.empty((mfb.max_len, B, 3 * mfb.pipe.features.C), dtype=torch.float32, device=dev)
        len0 = torch.empty(B, dtype=torch.int32, device=dev)
        mfb.enqueue(clips.data_ptr(), _wave_dtype_of(clips), lay, m0.data_ptr(), inp.data_ptr(), len0.data_ptr(),
                    torch.cuda.current_stream(dev), d_jitter=None if d_jit is None else d_jit.data_ptr())
        return self._head_loss(inp, len0, labels, head_kwargs, alias, [clips, lay, m0, labels, d_jit], spec)

    def _head_loss(self, inp, len0, labels, head_kwargs, alias, hold, spec=(False, None)):
        """The chain from ``inp`` / ``len0`` on: head, loss, the count of clamped lengths.  ``spec``: ``_loss_spec``'s pair."""
        import torch
        from .classifier import head_length_info
        kw = dict(device_len=True, device_grad=True, **head_kwargs)
        if alias is None:
            out = self.head(inp, len0, **kw)
        else:
            out = torch.func.functional_call(self.head, alias, (inp, len0), kw)
        logits = _logits_of(out)
        if spec[0]:                                                                     # one native call, the metrics with it
            from .metrics import cross_entropy
            loss = cross_entropy(logits, labels, spec[1])
        else:
            loss = torch.nn.functional.cross_entropy(logits, labels)                    # model.py:141-147
        n_clamped = head_length_info(len0, inp.shape[0], 1)[2][2:3]
        return types.SimpleNamespace(loss=loss, logits=logits, inp=inp, len0=len0, n_clamped=n_clamped, _hold=hold)

    def run(self, waves, sample_offsets, labels, jitter=None, capacity=None, loss='torch', metrics=None, **head_kwargs):
        """``loss='native'``: the loss is ``features.metrics.cross_entropy`` -- one native call for the loss and its gradient -- in
        place of ``F.cross_entropy``; ``metrics=`` (a ``features.metrics.Metrics``, with ``loss='native'`` only) is updated by the
        same call.  ``loss='torch'``, the default, launches what it launched.
        ``capacity=N``: the same chain on a capacity layout cached per (B, N) -- the launches ``capture(..., capacity=N)``
        records: ``waves`` is a contiguous device tensor of exactly N samples (ValueError otherwise), ``sample_offsets``
        ([B + 1], host array or device tensor) any B lengths >= 1 that sum to at most N; no layout is built or uploaded per
        batch shape.  ``status`` (int32 [1]) is added to the namespace.
        ``waves``: concatenated clips, a 1-D host array (int16 or float) or device tensor (int16 / float32);
        ``sample_offsets`` [B + 1]; ``labels`` [B] class indices; ``jitter``: int [B, 2] endpoint offsets (``draw_jitter``;
        model.py:144 trains with augment=True) or None.  Device tensors are read where they lie; host arrays are uploaded
        first.  -> a namespace (loss: the scalar ``F.cross_entropy(logits, labels)``, attached to the autograd graph; logits
        [B, C]; inp [200, B, 39]; len0 int32 [B]; n_clamped int32 [1]: the lengths the head had to clamp), all on the device.
        Nothing is synchronised and no device memory is read from the host: the caller calls ``loss.backward()`` and then
        its optimiser -- the head's native handles survive the step (they are repacked in place by the next call)."""
        import torch
        spec = _loss_spec(loss, metrics)
        nat.require_device()
        if capacity is not None:
            from .pipeline import check_capacity_wave
            check_capacity_wave(waves, capacity)
            _wave_dtype_of(waves)
            dev = waves.device
            B = int(sample_offsets.shape[0] if torch.is_tensor(sample_offsets) else len(sample_offsets)) - 1
            lay = self.features.pipe._capacity_layout(B, capacity, 0)
            lay.write_offsets(sample_offsets)
            ns = self._chain(waves, lay, self._m0(lay, dev), self._labels(labels, B, dev), self._jitter(jitter, B, dev), head_kwargs,
                             spec=spec)
            ns.status = lay.status
            return ns
        so = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        if _is_device_tensor(waves):
            clips = waves.reshape(-1).contiguous()
        else:
            host, _ = nat.as_wave(np.asarray(waves).reshape(-1))
            clips = torch.from_numpy(host).to(torch.device('cuda', nat.current_device()))
        _wave_dtype_of(clips)                              # TypeError for anything but int16 / float32
        dev, B = clips.device, len(so) - 1
        lay = self._layout(so)
        return self._chain(clips, lay, self._m0(lay, dev), self._labels(labels, B, dev), self._jitter(jitter, B, dev), head_kwargs,
                           spec=spec)

    def capture(self, waves, sample_offsets, labels, jitter=None, optimizer=None, capacity=None, loss='torch', metrics=None,
                census=False, **head_kwargs):
        """``census=True``: the graph is recorded with ``keep_graph=True`` and ``g.census`` is its node census
        (features/graphcheck.py); the default records exactly as before.
        ``loss='native'`` / ``metrics=`` as ``run``: the recorded loss is the native call, its backward launches nothing of its
        own, and every replay updates ``metrics`` (``capture`` itself leaves the block as it found it).
        ONE HIP graph of a whole step; without ``optimizer`` all of it but the optimiser: ``g = tb.capture(waves, so, labels, jitter, dropout=False)``;
        ``g.replay()`` does, in order, (1) a refresh of every native handle of the head -- the repack of whatever the
        optimiser wrote since the last replay --, (2) the front end, (3) the forward, (4) the loss and (5) the backward into
        ``.grad`` tensors the graph owns (``g.grads``), which every replay overwrites.  It returns the namespace of ``run``.
        ``waves`` (contiguous device tensor, int16 / float32), ``labels`` (int64 [B] device tensor) and ``jitter`` (int64
        [B, 2] device tensor, or None) are read at their addresses on every replay: write the next batch into them -- clips of
        the same lengths, unless the step was recorded with ``capacity=``.  With ``optimizer=None`` the optimiser step stays
        the caller's, eager, after ``replay()``.

        ``capacity=N``: ``waves`` is a contiguous 1-D tensor of exactly N samples (ValueError otherwise) and ``sample_offsets``
        the offsets of the batch it holds now.  The recorded step then serves ANY B clips whose lengths are >= 1 and sum to at
        most N: write the clips, their [B + 1] offsets into ``g.sample_offsets`` (int64 device tensor), the labels and the
        jitter, and replay; samples behind ``offsets[B]`` are ignored and ``g.status`` (int32 [1]) is 0 for a valid table.  The
        batch layout is rebuilt by two launches at the head of the front end (``features.pipeline.CapacityLayout``).
        ``CAPTURE_VERIFIED`` governs the head / B pairs as before; without ``capacity=`` exactly the same launches are
        recorded as before.

        ``optimizer``: a ``features.optim.DeviceAdam`` over exactly the head's trainable parameters, in their order.  The
        recorded sequence then ends in (6) the binding of the optimiser to ``g.grads`` and its step -- three launches of the
        library's, nothing of torch's -- and ``replay()`` bumps the parameters' version counters.  ``capture()`` itself changes
        neither the parameters nor the optimiser's state (the warm-up steps do not step), and ``optimizer.set_lr`` between
        replays takes effect without a new capture.  ``optimizer=None`` records exactly what it recorded before.

        The recipe is torch's for a whole network: warm-up steps on a side stream (they build the native handles and the
        layout's tables), then forward and backward recorded under ``torch.cuda.graph``.  Whatever ``.grad`` the parameters
        held before is dropped.  Recording raises on anything that synchronises or reads device memory from the host.

        The recorded step does not differentiate with respect to the module's own parameter objects but with respect to
        private leaf aliases of them (same storage, same version counter, made here on the capture stream and kept by the
        returned object).  A gradient accumulator is bound to the stream it was created on, and an autograd graph of an
        earlier eager step that is still alive keeps the parameters' accumulators, bound to the default stream; a recorded
        backward through those would pull that stream into the capture as a second branch.  The aliases' accumulators are
        created by the warm-up on the capture stream whatever the caller still holds.  The returned ``loss`` and ``logits``
        are detached.

        A head / size pair of ``CAPTURE_VERIFIED`` is served as it always was: a recorded multi-workgroup reduction of torch's
        has been seen to go wrong on replay on this stack, so those pairs are the ones where
        tests/test_gpu_train_capture.py has compared a second replay with the eager step bit for bit.  ANY OTHER batch size of
        the library's heads is served with ``native_sums=True`` among the head's keywords and ``loss='native'``: the step then
        launches no reduction of torch's, and ``capture`` looks instead of trusting -- it records with ``keep_graph=True``, takes
        the census, and raises RuntimeError carrying it (the graph is dropped) if the graph holds a memset node of more than 4
        bytes or one of torch's reductions (``at::native::reduce_kernel``).  Without those keywords anything outside the
        table raises NotImplementedError; ``run`` serves every head and size."""
        spec = _loss_spec(loss, metrics)
        so = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        B = len(so) - 1
        clips, check = self._check_capture(waves, B, labels, jitter, head_kwargs, loss)
        dev = waves.device
        if capacity is None:
            lay = self.features.pipe.prepare(so, 0)            # the graph's own: nothing else launches on its tables
        else:
            from .pipeline import check_capacity_wave
            check_capacity_wave(waves, capacity)
            lay = self.features.pipe.prepare_capacity(B, capacity, 0)
            lay.write_offsets(so)
        m0 = self._m0(lay, dev)
        g = self._record(dev, lambda alias: self._chain(clips, lay, m0, labels, jitter, head_kwargs, alias, spec), optimizer,
                         [lay, m0, clips, labels, jitter], head_kwargs.get('rng'), spec, census, check)
        if capacity is not None:
            g.sample_offsets, g.status = lay.sample_offsets_in, lay.status
        return g

    def _check_capture(self, waves, B, labels, jitter, head_kwargs=None, loss='torch'):
        """The refusals of ``capture`` in front of its layout -> (the clips as a flat view of ``waves``, whether the recorded
        graph has to pass the census: a pair outside the table, served because of ``native_sums=True`` and ``loss='native'``)."""
        import torch
        if not _is_device_tensor(waves):
            raise TypeError('capture needs a device tensor')
        if not waves.is_contiguous():
            raise ValueError('capture needs a contiguous waves tensor: the graph reads it in place on every replay')
        nat.require_device()
        clips = waves.reshape(-1)                              # a view: the same memory
        _wave_dtype_of(clips)
        kind = type(self.head).__name__
        check = False
        if B not in self._verified.get(kind, ()):
            check = kind in self._verified and (head_kwargs or {}).get('native_sums') is True and loss == 'native'
        if B not in self._verified.get(kind, ()) and not check:
            raise NotImplementedError(f'capture: {kind} at B = {B} is not in CAPTURE_VERIFIED ({self._verified}): a replay of this head '
                                      'and size has not been compared with the eager step; use run()')
        if not (_is_device_tensor(labels) and labels.dtype == torch.int64 and tuple(labels.shape) == (B,) and labels.is_contiguous()):
            raise TypeError('capture needs labels as a contiguous [B] int64 device tensor: the graph reads it in place')
        if jitter is not None and not (_is_device_tensor(jitter) and jitter.dtype == torch.int64 and tuple(jitter.shape) == (B, 2)
                                       and jitter.is_contiguous()):
            raise TypeError('capture needs jitter as a contiguous [B, 2] int64 device tensor (or None): the graph reads it in place')
        return clips, check

    @staticmethod
    def _backward(out, native):
        """The backward of a recorded step: a native loss is differentiated from ``features.metrics.unit_grad``."""
        if native:
            from .metrics import backward as native_backward
            native_backward(out.loss)
        else:
            out.loss.backward()

    def _record(self, dev, chain, optimizer, hold, rng=None, spec=(False, None), census=False, check=False):
        """The check of ``optimizer`` and the recipe of ``capture``: ``chain(alias)`` queues front end, head and loss on torch's current
        stream with the parameter aliases standing in, and returns the namespace of ``run``.  ``rng``: the generator the chain
        advances; the warm-up steps move it, so its state is put back behind them (recording runs nothing).  ``spec``:
        ``_loss_spec``'s pair; the metrics block is put back like the generator, and a native loss is differentiated from
        ``features.metrics.unit_grad``.  ``census``: record with ``keep_graph=True`` and attach the census; ``check``: the same, and
        a graph with a memset node of more than 4 bytes or a reduction kernel of torch's is refused (``capture``)."""
        import torch
        from .classifier import _NativeHandle
        names = [n for n, p in self.head.named_parameters() if p.requires_grad]
        params = [p for p in self.head.parameters() if p.requires_grad]
        if optimizer is not None:
            from .optim import DeviceAdam
            if not isinstance(optimizer, DeviceAdam):
                raise TypeError(f'capture: optimizer must be a features.optim.DeviceAdam or None, not {type(optimizer).__name__}: only its '
                                'step can be recorded')
            if len(optimizer.params) != len(params) or any(a is not b for a, b in zip(optimizer.params, params)):
                raise ValueError("capture: the optimizer's parameters must be the head's trainable parameters, in their order")
        handles = [m for m in self.head.modules() if isinstance(m, _NativeHandle)]
        bound = None if optimizer is None else optimizer._bound
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            leaves = [p.detach().requires_grad_(True) for p in params]      # aliases: the optimiser's writes to p are theirs
            rng_state = None if rng is None else rng.state.clone()
            native, metrics = spec
            metrics_state = None if metrics is None else metrics.state.clone()
            if native:
                from .metrics import unit_grad
                unit_grad(dev)                                 # (made here, not while recording)
        alias = dict(zip(names, leaves))

        def step(record):
            if record:                                         # the recorded sequence carries the repack
                for m in handles:
                    if m._handle is not None:
                        m._native_handle(dev, refresh='always')
            out = chain(alias)
            with torch.autograd.set_multithreading_enabled(False):      # every recorded launch comes from the capturing thread
                self._backward(out, native)
            if record and optimizer is not None:               # the graph's own gradients: their addresses are known from here on
                optimizer._launch([v.grad for v in leaves], False, rebind='always')
            out.loss, out.logits = out.loss.detach(), out.logits.detach()
            return out

        with torch.enable_grad():
            with torch.cuda.stream(side):
                for _ in range(2):
                    for v in leaves:
                        v.grad = None
                    warm = step(False)
                if rng is not None:
                    rng.state.copy_(rng_state)
                if metrics is not None:
                    metrics.state.copy_(metrics_state)
            side.synchronize()
            del warm
            for v in leaves:
                v.grad = None
            graph = torch.cuda.CUDAGraph(keep_graph=True) if (census or check) else torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                result = step(True)
        grads = [v.grad for v in leaves]
        for p in params:
            p.grad = None
        if optimizer is not None:
            optimizer._bound = bound                           # the recorded binding has not run yet
        found = None
        if census or check:
            from .graphcheck import census as graph_census
            found = graph_census(graph)
            bad = found.torch_reductions()                 # (a '?' is a library GEMM launched from a code object: the runtime names none)
            if check and (found.wide_memsets or bad):
                del graph, result, grads                       # the recording is dropped: nothing of it ever runs
                raise RuntimeError(f'capture: the recorded step holds {found.wide_memsets} memset node(s) of more than 4 bytes (the widest '
                                   f'{found.widest_memset_bytes}) and {len(bad)} reduction kernel(s) of torch\'s {sorted(set(bad))[:4]}: such a '
                                   f'graph has been seen to replay wrong here (DESIGN 7.12) and is not served.  Census: {found}')
            graph.instantiate()
        # (the head too: its modules own the native handles whose packed weights the recorded kernels read, and a module's
        # ``__del__`` destroys its handle -- a step that outlived its head would replay on freed memory)
        g = _CapturedStep(graph, result, params, grads, list(hold) + [leaves, metrics, self.head], optimizer, rng)
        g.census = found
        return g


class MixedRateTrainBatch(TrainBatch):
    """model.py:137-147 for batches that mix the sample rates of a fixed table (reader.py:80 yields 44.1 and 48 kHz files in
    shuffled order): ``TrainBatch``'s capacity routes over ``model_glue.MixedRateCapacityBatch``, whose front end groups the
    clips by rate on the device.  From ``inp`` / ``len0`` on the chain is ``TrainBatch``'s.  Capacity routes only: ``run`` and
    ``capture`` need ``capacity=N``; one recorded step then serves an epoch whose lengths AND rate assignments change from
    batch to batch."""

    def __init__(self, rates, head, frame=0.03, step=0.01):
        from .model_glue import MixedRateCapacityBatch
        self.features = MixedRateCapacityBatch(rates, frame=frame, step=step)     # ValueError for a bad table, before any device work
        self.rates, self.head = self.features.rates, head

    def draw_jitter(self, rates, rng):
        """The endpoint offsets of model.py:54-60 for a batch with these [B] rates, in the reference's order: int64 [B, 2]."""
        return self.features.draw_jitter(rates, rng)

    def _mixed_chain(self, clips, arena, labels, use_jitter, head_kwargs, alias=None, spec=(False, None)):
        import torch
        _advance_rng(head_kwargs)
        inp, len0, endpoints = self.features._outputs(arena.B, clips.device)
        self.features.enqueue(clips, arena, inp, len0, endpoints, use_jitter, torch.cuda.current_stream(clips.device))
        ns = self._head_loss(inp, len0, labels, head_kwargs, alias, [clips, arena, labels], spec)
        ns.endpoints, ns.status = endpoints, arena.status
        return ns

    def run(self, waves, sample_offsets, rates, labels, jitter=None, capacity=None, loss='torch', metrics=None, **head_kwargs):
        """``loss=`` / ``metrics=`` as ``TrainBatch.run``.  ``TrainBatch.run(..., capacity=N)`` with ``rates`` [B] beside the offsets (host arrays or device tensors): the launches
        ``capture`` records, on an arena cached per (B, N).  The namespace also carries ``endpoints`` (int64 [B, 2]) and
        ``status`` (``MixedRateCapacityBatch``: bit 4 = a rate outside the table)."""
        from .pipeline import check_capacity_wave
        spec = _loss_spec(loss, metrics)
        nat.require_device()
        if capacity is None:
            raise ValueError('MixedRateTrainBatch serves capacity routes only: pass capacity=N')
        check_capacity_wave(waves, capacity)
        _wave_dtype_of(waves)
        fe = self.features
        B = fe._n_utt(sample_offsets)
        labels, jitter = self._labels(labels, B, waves.device), self._jitter(jitter, B, waves.device)
        arena = fe._arena(B, capacity, waves)
        arena.write(sample_offsets, rates, jitter)
        return self._mixed_chain(waves, arena, labels, jitter is not None, head_kwargs, spec=spec)

    def capture(self, waves, sample_offsets, rates, labels, jitter=None, optimizer=None, capacity=None, loss='torch', metrics=None,
                census=False, **head_kwargs):
        """``census=``, ``loss=`` / ``metrics=`` and the batch sizes served as ``TrainBatch.capture``.  ``TrainBatch.capture(..., capacity=N)`` for a mixed-rate batch: ONE HIP graph of the handle refresh, the grouping
        front end, forward, loss, backward and -- with ``optimizer=`` -- the ``DeviceAdam`` step.  Before a ``replay()`` write
        the next batch's clips into ``waves``, its offsets into ``g.sample_offsets`` (int64 [B + 1]), its rates into ``g.rates``
        (int32 [B]), the labels into ``labels`` and -- if recorded with jitter -- its rows into ``g.jitter`` (int64 [B, 2]: the
        graph's own table, a copy of ``jitter`` as given here).  ``CAPTURE_VERIFIED`` governs the head / B pairs as before."""
        from .pipeline import check_capacity_wave
        spec = _loss_spec(loss, metrics)
        fe = self.features
        B = fe._n_utt(sample_offsets)
        clips, check = self._check_capture(waves, B, labels, jitter, head_kwargs, loss)
        if capacity is None:
            raise ValueError('MixedRateTrainBatch serves capacity routes only: pass capacity=N')
        check_capacity_wave(waves, capacity)
        arena = fe.prepare(B, capacity, waves)                 # the graph's own
        arena.write(sample_offsets, rates, jitter)
        use_jitter = jitter is not None
        g = self._record(waves.device, lambda alias: self._mixed_chain(clips, arena, labels, use_jitter, head_kwargs, alias, spec),
                         optimizer, [arena, clips, labels], head_kwargs.get('rng'), spec, census, check)
        g.sample_offsets, g.rates, g.status = arena.sample_offsets, arena.rates, arena.status
        g.jitter = arena.jitter if use_jitter else None
        return g


class AdvTrainBatch(TrainBatch):
    """adv_model.py:33-48 for a batch of raw clips of one sample rate: ``TrainBatch`` over a ``features.adversarial.AdvHRNNHead``
    with the speakers beside the labels and ``loss = CE(logits, labels) + CE(logits2, speakers)`` (adv_model.py:45-47).

    ``run(waves, sample_offsets, labels, speakers, ...)`` / ``capture(..., optimizer=)`` take ``TrainBatch``'s arguments plus
    ``speakers`` (int64 [B]; for ``capture`` a contiguous device tensor that is read in place on every replay),
    ``speaker_metrics`` (a ``features.metrics.Metrics`` over the head's n_speakers classes, updated by the native discriminator's
    loss call: it needs ``native_disc=True``) and ``native_disc`` (None follows ``AdvHRNNHead.native_disc_default``): the
    discriminator as ONE native call whose backward launches nothing (``dsp_adv_disc_train``).  The namespace gains
    ``loss_label``, ``loss_speaker`` and ``logits2``; ``loss`` is their sum.  ``AdvTrainBatch.backward(ns)`` differentiates both
    losses from ``features.metrics.unit_grad``, so neither native loss launches anything in backward; the recorded step does
    the same.  ``MixedRateTrainBatch`` and ``features.fit.Trainer.fit`` over speakers are out of scope: mixed-rate batches and
    the epoch schedule serve the five label-only heads."""

    _verified = ADV_CAPTURE_VERIFIED

    def __init__(self, rate, head, frame=0.03, step=0.01):
        from .adversarial import AdvHRNNHead
        if not isinstance(head, AdvHRNNHead):
            raise TypeError(f'AdvTrainBatch needs a features.adversarial.AdvHRNNHead, not {type(head).__name__}')
        super().__init__(rate, head, frame=frame, step=step)

    @staticmethod
    def _adv_spec(speakers, B, loss, speaker_metrics, native_disc, head, device_tensor=False):
        """The refusals of the speaker arguments; they need no device."""
        import torch
        if loss not in ('torch', 'native'):
            raise ValueError(f"loss must be 'torch' or 'native', got {loss!r}")
        if speaker_metrics is not None:
            if loss != 'native':
                raise ValueError("speaker_metrics= needs loss='native': the device metrics are updated by the native loss calls")
            from .metrics import Metrics
            if not isinstance(speaker_metrics, Metrics):
                raise TypeError(f'speaker_metrics must be a features.metrics.Metrics, not {type(speaker_metrics).__name__}')
            if not (head.native_disc_default if native_disc is None else native_disc):
                raise ValueError('speaker_metrics= needs native_disc=True: they are updated by the native discriminator call')
        if not torch.is_tensor(speakers):
            a = np.asarray(speakers)
            if a.dtype.kind not in 'iu':
                raise TypeError(f'speakers must be integers (int64 [B]), got {a.dtype}')
            speakers = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
        if speakers.dtype != torch.int64:
            raise TypeError(f'speakers must be int64, got {speakers.dtype}')
        if tuple(speakers.shape) != (B,):
            raise ValueError(f'speakers must be [B] = [{B}], got {tuple(speakers.shape)}')
        if device_tensor and not (speakers.is_cuda and speakers.is_contiguous()):
            raise TypeError('capture needs speakers as a contiguous [B] int64 device tensor: the graph reads it in place')
        return speakers

    @staticmethod
    def _n_utt(sample_offsets):
        import torch
        return int(sample_offsets.shape[0] if torch.is_tensor(sample_offsets) else len(sample_offsets)) - 1

    def _head_loss(self, inp, len0, labels, head_kwargs, alias, hold, spec=(False, None)):
        """``TrainBatch._head_loss`` with the second loss.  The speaker arguments travel from ``run`` / ``capture`` through the
        base class's chain among the head's keywords, under the reserved key ``_adv``."""
        import torch
        from .classifier import head_length_info
        head_kwargs = dict(head_kwargs)
        speakers, speaker_metrics, native_disc = head_kwargs.pop('_adv')
        speakers = speakers.to(inp.device)
        kw = dict(device_len=True, device_grad=True, speakers=speakers, native_disc=native_disc, speaker_metrics=speaker_metrics,
                  **head_kwargs)
        if alias is None:
            logits, logits2, loss_speaker = self.head(inp, len0, **kw)
        else:
            logits, logits2, loss_speaker = torch.func.functional_call(self.head, alias, (inp, len0), kw)
        if spec[0]:
            from .metrics import cross_entropy
            loss_label = cross_entropy(logits, labels, spec[1])
        else:
            loss_label = torch.nn.functional.cross_entropy(logits, labels)
        n_clamped = head_length_info(len0, inp.shape[0], 1)[2][2:3]
        return types.SimpleNamespace(loss=(loss_label + loss_speaker).detach(), loss_label=loss_label, loss_speaker=loss_speaker,
                                     logits=logits, logits2=logits2, inp=inp, len0=len0, n_clamped=n_clamped,
                                     _hold=list(hold) + [speakers])

    @staticmethod
    def backward(ns):
        """Differentiate both losses of a ``run`` namespace from ``unit_grad``: one autograd pass over both roots."""
        import torch
        from .metrics import unit_grad
        u = unit_grad(ns.loss_label.device)
        torch.autograd.backward([ns.loss_label, ns.loss_speaker], [u, u])

    @staticmethod
    def _backward(out, native):
        AdvTrainBatch.backward(out)

    def run(self, waves, sample_offsets, labels, speakers, jitter=None, capacity=None, loss='torch', metrics=None, speaker_metrics=None,
            native_disc=None, **head_kwargs):
        """``TrainBatch.run`` with ``speakers`` (class docstring).  ``loss`` in the namespace is the detached sum; call
        ``AdvTrainBatch.backward(ns)`` (or ``(ns.loss_label + ns.loss_speaker).backward()``)."""
        speakers = self._adv_spec(speakers, self._n_utt(sample_offsets), loss, speaker_metrics, native_disc, self.head)
        return super().run(waves, sample_offsets, labels, jitter=jitter, capacity=capacity, loss=loss, metrics=metrics,
                           _adv=(speakers, speaker_metrics, native_disc), **head_kwargs)

    def capture(self, waves, sample_offsets, labels, speakers, jitter=None, optimizer=None, capacity=None, loss='torch', metrics=None,
                speaker_metrics=None, native_disc=None, census=False, **head_kwargs):
        """``TrainBatch.capture`` with ``speakers``: the recorded step reads them in place on every replay, and every replay
        updates ``speaker_metrics`` (``capture`` itself leaves the block as it found it).  ``ADV_CAPTURE_VERIFIED['AdvHRNNHead']``
        governs the batch sizes as ``CAPTURE_VERIFIED`` governs ``TrainBatch.capture``'s: any other size is served with
        ``native_sums=True`` (which needs ``native_disc=True``) and ``loss='native'``, checked by the census.  ``census=`` as there."""
        import torch
        speakers = self._adv_spec(speakers, self._n_utt(sample_offsets), loss, speaker_metrics, native_disc, self.head, device_tensor=True)
        from .metrics import unit_grad
        unit_grad(speakers.device)                             # (made here, not while recording)
        saved = None if speaker_metrics is None else speaker_metrics.state.clone()
        g = super().capture(waves, sample_offsets, labels, jitter=jitter, optimizer=optimizer, capacity=capacity, loss=loss,
                            metrics=metrics, census=census, _adv=(speakers, speaker_metrics, native_disc), **head_kwargs)
        if saved is not None:                                  # the warm-up steps moved it; recording ran nothing
            speaker_metrics.state.copy_(saved)
        g.hold.append((speakers, speaker_metrics, self.head.d_gamma))
        g.result.loss_label, g.result.loss_speaker = g.result.loss_label.detach(), g.result.loss_speaker.detach()
        g.result.logits2 = g.result.logits2.detach()
        return g
