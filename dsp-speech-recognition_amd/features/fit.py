"""The reference's ``train`` mode (model.py:219-240 over ``RNNModel.train``, model.py:137-150, and ``RNNModel.test``,
model.py:162-187) on the device, over an in-memory data set: epochs with a fresh Adam each, validation, the learning-rate
schedule, saving on improvement, early stopping and ``adjust_param`` -- with ONE download per epoch and phase
(``Metrics.result()``) instead of a ``loss.data[0]`` per step and a ``pred_`` per batch.

* ``Schedule`` is model.py:220-236 as a pure object: accuracy in, (improved, stop) out, ``lr`` updated.  It needs no device.
* ``epoch_order`` is reader.py:90: ``random.Random(0).shuffle`` of the list the iterator holds, in place, so the order is
  cumulative over epochs.
* ``Trainer`` drives ``TrainBatch`` (``loss='native', metrics=``), ``DeviceAdam`` (``reset`` / ``set_lr``) and ``EnsembleBatch``
  (``labels=, metrics=``) -- or, for the shuffled 44.1 / 48 kHz batches of reader.py:80, the mixed-rate pair ``MixedRateTrainBatch``
  and ``MixedRateCapacityEnsembleBatch``.  Host arrays are uploaded batch by batch; nothing overlaps the upload with the step.
"""
from __future__ import annotations

import random
import types

import numpy as np


class Schedule:
    """model.py:220-236: ``prev_acc = 0``, ``early_stop = 3``; an epoch whose accuracy is strictly above the best so far is
    saved and ``lr *= 0.8``; any other epoch costs one of the ``early_stop`` lives and ``lr *= 0.5``, and the run stops when
    none is left."""

    def __init__(self, lr, early_stop=3):
        self.lr, self.early_stop, self.prev_acc = lr, int(early_stop), 0

    def step(self, acc):
        """-> (improved, stop); ``lr`` is the next epoch's afterwards."""
        if acc > self.prev_acc:
            self.prev_acc = acc
            self.lr *= 0.8
            return True, False
        self.early_stop -= 1
        self.lr *= 0.5
        return False, not self.early_stop


def epoch_order(order):
    """reader.py:90 on the list the caller holds: shuffled in place by a new ``random.Random(0)``; returns it."""
    random.Random(0).shuffle(order)
    return order


def check_rates(rates, served, what='a clip'):
    """ValueError for the first of ``rates`` that is not one of ``served`` (the batches' rate or rate table): on the host, before
    any launch."""
    served = tuple(int(r) for r in served)
    for r in rates:
        if int(r) not in served:
            only = f'{served[0]} Hz only' if len(served) == 1 else f'the rate table {list(served)} only'
            raise ValueError(f'{what} at {int(r)} Hz: this Trainer serves {only}')


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


class _Phase:
    """One data set with the list of indices it holds, its device buffers and its recorded graph."""

    def __init__(self, data, what):
        feat, labels = data
        self.clips = [np.asarray(sig).reshape(-1) for sig, _ in feat]
        self.rates = [int(rate) for _, rate in feat]
        self.labels = np.ascontiguousarray(labels, dtype=np.int64)
        if len(self.labels) != len(self.clips) or not self.clips:
            raise ValueError(f'{what}: {len(self.clips)} clips with {len(self.labels)} labels (at least one clip is needed)')
        self.order = list(range(len(self.clips)))
        self.graph = self.buf = self.lab = self.jit = None
        self.part = None           # the trailing partial batch's own buffers and graph (``fit(native_sums=True)``): a _Slot

    def batches(self, batch_size):
        for s in range(0, len(self.order), batch_size):
            yield self.order[s:s + batch_size]


class _Slot:
    """The capacity buffers and the recorded graph of one batch size."""

    def __init__(self):
        self.graph = self.buf = self.lab = self.jit = None


class Trainer:
    """``Trainer(train_batch, eval_batch, optimizer, n_classes)``: a ``features.train.TrainBatch`` over the head, a
    ``features.ensemble.EnsembleBatch`` over the SAME head (with its rules, or none) for validation, and a
    ``features.optim.DeviceAdam`` over the head's trainable parameters.  One sample rate: every clip's rate must be the
    batches'.  Or the mixed-rate pair: a ``features.train.MixedRateTrainBatch`` with a
    ``features.ensemble.MixedRateCapacityEnsembleBatch`` over the same head and the same rate table -- ``fit`` then serves clips
    at any of the table's rates, in any order; any other pairing of a mixed-rate with a single-rate class is a TypeError.

    ``head_kwargs``: keywords of the head for both phases (``dropout=False``, ``rng=...``); ``eval_kwargs``: those of validation
    where they differ.  ``jitter_rng``: the ``random.Random`` the endpoint jitter of model.py:54-60 is drawn from
    (``TrainBatch.draw_jitter``).  ``wrong_capacity``: of the two ``Metrics`` blocks (``train_metrics``, ``val_metrics``)."""

    def __init__(self, train_batch, eval_batch, optimizer, n_classes, wrong_capacity=4096, head_kwargs=None, eval_kwargs=None,
                 jitter_rng=None):
        from .ensemble import EnsembleBatch, MixedRateCapacityEnsembleBatch
        from .metrics import Metrics
        from .optim import DeviceAdam
        from .train import MixedRateTrainBatch, TrainBatch
        self.mixed = isinstance(train_batch, MixedRateTrainBatch) and isinstance(eval_batch, MixedRateCapacityEnsembleBatch)
        if self.mixed:
            if eval_batch.head is not train_batch.head:
                raise ValueError('train_batch and eval_batch must share one head')
            if tuple(eval_batch.rates) != tuple(train_batch.rates):
                raise ValueError(f'train_batch is for the rate table {list(train_batch.rates)}, eval_batch for {list(eval_batch.rates)}')
        elif isinstance(train_batch, MixedRateTrainBatch) or isinstance(eval_batch, MixedRateCapacityEnsembleBatch):
            raise TypeError('a features.train.MixedRateTrainBatch goes with a features.ensemble.MixedRateCapacityEnsembleBatch, and '
                            'only with it: a mixed-rate class is not paired with a single-rate one')
        elif not isinstance(train_batch, TrainBatch):
            raise TypeError('Trainer drives a features.train.TrainBatch (one sample rate) or a features.train.MixedRateTrainBatch')
        elif not isinstance(eval_batch, EnsembleBatch):
            raise TypeError('Trainer validates through a features.ensemble.EnsembleBatch')
        if not isinstance(optimizer, DeviceAdam):
            raise TypeError('Trainer needs a features.optim.DeviceAdam: only its step can be recorded and reset in place')
        if not self.mixed:
            if eval_batch.head is not train_batch.head:
                raise ValueError('train_batch and eval_batch must share one head')
            if eval_batch.rate != train_batch.rate:
                raise ValueError(f'train_batch is for {train_batch.rate} Hz, eval_batch for {eval_batch.rate} Hz')
        self.tb, self.eb, self.opt, self.head = train_batch, eval_batch, optimizer, train_batch.head
        self.n_classes = int(n_classes)
        self.head_kwargs = dict(head_kwargs or {})
        self.eval_kwargs = dict(self.head_kwargs if eval_kwargs is None else eval_kwargs)
        self.jitter_rng = random.Random(0) if jitter_rng is None else jitter_rng
        self.device = optimizer.device
        self.train_metrics = Metrics(self.n_classes, wrong_capacity, self.device)
        self.val_metrics = Metrics(self.n_classes, wrong_capacity, self.device)

    # ---- one batch ------------------------------------------------------------------------------------------------
    def _buffers(self, ph, B, capacity, dtype, jitter):
        import torch
        if ph.buf is None:
            ph.buf = torch.zeros(capacity, dtype=dtype, device=self.device)
            ph.lab = torch.zeros(B, dtype=torch.int64, device=self.device)
            ph.jit = torch.zeros((B, 2), dtype=torch.int64, device=self.device) if jitter else None

    def _upload(self, ph, flat, labels, jitter):
        import torch
        ph.buf[:len(flat)].copy_(torch.from_numpy(flat))   # (samples behind the last offset are ignored)
        ph.lab.copy_(torch.from_numpy(labels))
        if jitter is not None:
            ph.jit.copy_(torch.from_numpy(jitter))

    def _flat(self, ph, idx, dtype):
        clips = [ph.clips[i] for i in idx]
        return np.concatenate(clips).astype(dtype, copy=False), _offsets(clips), ph.labels[idx]

    # ---- one batch of the mixed-rate pair ----------------------------------------------------------------------------
    @staticmethod
    def _part(ph):
        if ph.part is None:
            ph.part = _Slot()
        return ph.part

    @staticmethod
    def _replay_mixed(g, so, rates, jit=None):
        """The next batch's tables into the graph's own tensors, then the replay."""
        import torch
        g.sample_offsets.copy_(torch.from_numpy(so))
        g.rates.copy_(torch.from_numpy(rates))
        if jit is not None:
            g.jitter.copy_(jit)
        g.replay()

    def _train_step_mixed(self, ph, idx, B, capacity, np_dtype, torch_dtype, recordable, native_sums):
        from . import metrics as M
        flat, so, labels = self._flat(ph, idx, np_dtype)
        rates = np.array([ph.rates[i] for i in idx], dtype=np.int32)
        jitter = self.tb.draw_jitter(rates, self.jitter_rng)
        m, kw = self.train_metrics, self.head_kwargs
        full = len(idx) == B
        slot = ph if full else self._part(ph)              # every size on capacity buffers of its own: an arena per (B, N)
        self._buffers(slot, len(idx), capacity, torch_dtype, True)
        self._upload(slot, flat, labels, jitter)
        if native_sums:
            kw = dict(kw, native_sums=True)
        if native_sums or (full and recordable):
            if slot.graph is None:
                slot.graph = self.tb.capture(slot.buf, so, rates, slot.lab, slot.jit, optimizer=self.opt, capacity=capacity,
                                             loss='native', metrics=m, **kw)
                self.train_graphs += 1 if native_sums else 0
            self._replay_mixed(slot.graph, so, rates, slot.jit)
            return
        out = self.tb.run(slot.buf, so, rates, slot.lab, slot.jit, capacity=capacity, loss='native', metrics=m, **kw)
        for p in self.opt.params:
            p.grad = None
        M.backward(out.loss)
        self.opt.step()

    def _eval_step_mixed(self, ph, idx, B, capacity, np_dtype, torch_dtype):
        flat, so, labels = self._flat(ph, idx, np_dtype)
        rates = np.array([ph.rates[i] for i in idx], dtype=np.int32)
        m, kw = self.val_metrics, self.eval_kwargs
        full = len(idx) == B
        slot = ph if full else self._part(ph)
        self._buffers(slot, len(idx), capacity, torch_dtype, False)
        self._upload(slot, flat, labels, None)
        if full:
            if ph.graph is None:
                ph.graph = self.eb.capture(ph.buf, so, rates, capacity=capacity, labels=ph.lab, metrics=m, **kw)
            self._replay_mixed(ph.graph, so, rates)
        else:
            self.eb.run(slot.buf, so, rates, capacity=capacity, labels=slot.lab, metrics=m, **kw)

    # ---- one batch at one rate ------------------------------------------------------------------------------------
    def _train_step(self, ph, idx, B, capacity, np_dtype, torch_dtype, recordable, native_sums=False):
        import torch
        from . import metrics as M
        if self.mixed:
            return self._train_step_mixed(ph, idx, B, capacity, np_dtype, torch_dtype, recordable, native_sums)
        flat, so, labels = self._flat(ph, idx, np_dtype)
        jitter = self.tb.draw_jitter(len(idx), self.jitter_rng)
        m, kw = self.train_metrics, self.head_kwargs
        if native_sums:                                    # any size records, the partial batch through a graph of its own
            kw = dict(kw, native_sums=True)
            slot = ph
            if len(idx) != B:
                slot = ph.part = ph.part or _Slot()
            self._buffers(slot, len(idx), capacity, torch_dtype, True)
            self._upload(slot, flat, labels, jitter)
            if slot.graph is None:
                slot.graph = self.tb.capture(slot.buf, so, slot.lab, slot.jit, optimizer=self.opt, capacity=capacity, loss='native',
                                             metrics=m, **kw)
                self.train_graphs += 1
            slot.graph.sample_offsets.copy_(torch.from_numpy(so))
            slot.graph.replay()
            return
        if len(idx) == B:                                  # a full batch: the capacity layout, recorded where it may be
            self._buffers(ph, B, capacity, torch_dtype, True)
            self._upload(ph, flat, labels, jitter)
            if recordable:
                if ph.graph is None:
                    ph.graph = self.tb.capture(ph.buf, so, ph.lab, ph.jit, optimizer=self.opt, capacity=capacity, loss='native',
                                               metrics=m, **kw)
                ph.graph.sample_offsets.copy_(torch.from_numpy(so))
                ph.graph.replay()
                return
            out = self.tb.run(ph.buf, so, ph.lab, ph.jit, capacity=capacity, loss='native', metrics=m, **kw)
        else:                                              # the trailing partial batch: its exact shape, no pad clips
            out = self.tb.run(flat, so, labels, jitter, loss='native', metrics=m, **kw)
        for p in self.opt.params:
            p.grad = None
        M.backward(out.loss)
        self.opt.step()

    def _eval_step(self, ph, idx, B, capacity, np_dtype, torch_dtype):
        import torch
        if self.mixed:
            return self._eval_step_mixed(ph, idx, B, capacity, np_dtype, torch_dtype)
        flat, so, labels = self._flat(ph, idx, np_dtype)
        m, kw = self.val_metrics, self.eval_kwargs
        if len(idx) == B:
            self._buffers(ph, B, capacity, torch_dtype, False)
            self._upload(ph, flat, labels, None)
            if ph.graph is None:
                ph.graph = self.eb.capture(ph.buf, so, capacity=capacity, labels=ph.lab, metrics=m, **kw)
            ph.graph.sample_offsets.copy_(torch.from_numpy(so))
            ph.graph.replay()
        else:
            self.eb.run(flat, so, sync_free=True, labels=torch.from_numpy(labels).to(self.device), metrics=m, **kw)

    # ---- the run --------------------------------------------------------------------------------------------------
    def fit(self, train, val, lr, epochs=10, early_stop=3, batch_size=32, capacity=None, on_improve=None, on_epoch=None,
            native_sums=False):
        """model.py:219-240.  ``train`` / ``val``: ``(feat, labels)`` with ``feat = [(sig, rate), ...]`` (reader.py:84) and one
        class index per clip.  Per epoch: ``optimizer.reset()`` and ``set_lr(lr)`` (model.py:140 makes a new Adam); the training
        list in ``epoch_order``; full batches through ONE capacity graph of the whole step -- recorded at the first full batch
        with ``loss='native', metrics=`` -- or, where ``CAPTURE_VERIFIED`` refuses the head / size pair, through
        ``run(capacity=...)``; the trailing partial batch through the exact-shape ``run`` and an eager ``optimizer.step()`` (no
        pad clips: ``TransformerHead``'s softmax runs over the batch axis).  Validation: the head in ``eval()`` under
        ``no_grad``, the validation list in ``epoch_order`` too (``RNNModel.test`` iterates through the same shuffling
        iterator), full batches through one recorded ``EnsembleBatch`` graph with ``labels=, metrics=``, the partial batch
        through ``run(sync_free=True, ...)``.  Then the schedule: on ``acc > prev`` ``on_improve(epoch, acc)`` (save there) and
        ``lr *= 0.8``; otherwise ``lr *= 0.5`` and one life less, stopping at none; ``head.adjust_param()`` where there is one;
        the head back in ``train()``.  ``adjust_param`` changes a value the recorded launches took by value, so both graphs
        are recorded anew in the next epoch for such a head.

        ``native_sums=True``: the head is trained with ``native_sums=True`` (features/classifier.py), with which ``capture`` serves
        ANY batch size; every full batch goes through the capacity graph whatever ``batch_size`` is, and the trailing partial
        batch -- whose size is the same in every epoch -- through a second capacity graph of its own.  Both are recorded anew
        after ``adjust_param``.  ``train_graphs`` in each epoch's entry (and on the trainer) counts the training graphs recorded
        so far.

        The mixed-rate pair: the same decisions, every batch on capacity buffers.  Each batch also writes its ``rates`` (and its
        jitter rows, drawn by ``MixedRateTrainBatch.draw_jitter(rates, rng)``) into the graph's own tensors, so ONE training graph
        and ONE validation graph serve full batches whatever their lengths and rate assignments are; the trailing partial
        batches go through ``run(..., capacity=)`` on an arena of their own size (training: with an eager ``optimizer.step()``, or
        through the second graph with ``native_sums=True``).  A clip whose rate is not in the table is a ValueError before any launch.

        ``capacity``: samples of the capacity buffers; default: the sum of the ``batch_size`` longest clips of both sets.
        -> the history: per epoch a namespace (epoch, lr: the epoch's rate, train / val: ``Metrics.result()``, improved, stop,
        train_order / val_order: the epoch's orders, which the ``wrong`` lists index).  ``on_epoch(entry)``: called with each
        epoch's entry behind the schedule's decision and before ``adjust_param``."""
        import torch
        from .train import CAPTURE_VERIFIED
        tr, va = _Phase(train, 'train'), _Phase(val, 'val')
        B = int(batch_size)
        if B < 1:
            raise ValueError(f'batch_size {batch_size} must be >= 1')
        for ph in (tr, va):
            check_rates(ph.rates, self.tb.rates if self.mixed else (self.tb.rate,))
        all_clips = tr.clips + va.clips
        int16 = all(c.dtype == np.int16 for c in all_clips)
        np_dtype, torch_dtype = (np.int16, torch.int16) if int16 else (np.float32, torch.float32)
        if capacity is None:
            capacity = int(sum(sorted((len(c) for c in all_clips), reverse=True)[:B]))
        recordable = B in CAPTURE_VERIFIED.get(type(self.head).__name__, ())
        self.train_graphs = 0
        sched = Schedule(lr, early_stop)
        history = []
        for epoch in range(int(epochs)):
            lr_now = sched.lr
            self.opt.reset()
            self.opt.set_lr(lr_now)
            self.head.train()
            self.train_metrics.reset()
            epoch_order(tr.order)
            for idx in tr.batches(B):
                self._train_step(tr, idx, B, capacity, np_dtype, torch_dtype, recordable, native_sums)
            train_res = self.train_metrics.result()
            self.head.eval()
            self.val_metrics.reset()
            epoch_order(va.order)
            with torch.no_grad():
                for idx in va.batches(B):
                    self._eval_step(va, idx, B, capacity, np_dtype, torch_dtype)
            val_res = self.val_metrics.result()
            improved, stop = sched.step(val_res.accuracy)
            if improved and on_improve is not None:
                on_improve(epoch, val_res.accuracy)
            history.append(types.SimpleNamespace(epoch=epoch, lr=lr_now, train=train_res, val=val_res, improved=improved, stop=stop,
                                                 train_order=list(tr.order), val_order=list(va.order), train_graphs=self.train_graphs))
            if on_epoch is not None:
                on_epoch(history[-1])
            if stop:
                self.head.train()
                break
            if hasattr(self.head, 'adjust_param'):
                self.head.adjust_param()
                tr.graph = va.graph = None                 # the recorded launches hold the old value
                if tr.part is not None:
                    tr.part.graph = None
                if va.part is not None:
                    va.part.graph = None
            self.head.train()
        return history
