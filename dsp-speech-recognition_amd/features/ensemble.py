"""The reference's ensemble (ensemble.py:44-67) on the device: the classifier answers first, and where it predicts one of a
tone-confusable pair of words with too little confidence, an RBF support-vector machine on the clip's five pitch features
decides instead (pitch_model.py:54-61).

* ``PitchSVM`` holds one fitted ``RobustScaler`` + ``SVC(kernel='rbf')`` pair as plain arrays (``from_sklearn`` reads the
  fitted objects' public attributes; nothing here imports the library that fitted them) and evaluates it with
  ``dsp_svm_decision_batch``.
* ``ensemble_decide`` is the gate: softmax, arg-max, the rules and the SVMs in one launch (``dsp_ensemble_decide_batch``).
* ``EnsembleBatch`` runs the whole path for a batch of raw clips -- endpointing and the classifier's features
  (``ModelFeatureBatch``), the classifier head, the pre-emphasised trimmed copy (``dsp_trim_preemph_batch``), the pitch
  features (``pitch_features_device``) and the gate -- on torch's current stream; no clip, logit or feature visits the host.
  ``run()`` downloads the lengths and the endpoints between the front end and the head (one synchronisation);
  ``run(sync_free=True)`` leaves them on the device (``device_len=True`` on the head), and ``capture()`` records that whole
  chain into ONE HIP graph whose ``replay()`` serves new clips written into the captured buffer.
* ``MixedRateEnsembleBatch`` is the same for a batch that mixes sample rates, bound to the batch's lengths and rates;
  ``MixedRateCapacityEnsembleBatch`` groups by rate on the device, so ONE recorded graph serves any lengths and any assignment
  of a fixed table's rates (``dsp_scatter_group_rows_batch`` brings the groups' pitch rows back to batch order).

Training (pitch_model.py:26-50) runs on the device too: ``PitchSVM.fit(X, y)`` fits the scaler and the SVM with the kernels
of csrc/kernels_svmfit.h (features/svmfit.py: ``fit_pitch_svm``, ``grid_search``, ``PitchModelTrainer``).  A pair fitted with
scikit-learn elsewhere still comes in through ``PitchSVM.from_sklearn(scaler, clf)``.
"""
from __future__ import annotations

import types

import numpy as np

from . import _native as nat
from .batch import _capture, _is_device_tensor, _on_stream, _stream_ptr, _wave_dtype_of
from .pipeline import _TensorBuffer

MAX_FEATURES, MAX_SV, MAX_RULES = 16, 65536, 4
REFERENCE_RULES = (((0, 1), 0.8), ((6, 7), 0.7))          # ensemble.py:50-53: (label pair, confidence threshold)


def _torch_stream(dev):
    import torch
    return _stream_ptr(torch.cuda.current_stream(dev))


class PitchSVM:
    """A fitted scaler + two-class RBF SVM:  dec(x) = sum_i dual[i] exp(-gamma |(x - center) / scale - sv[i]|^2) + intercept,
    predict = classes[dec > 0].  The native handle is built on first use on the current device and freed with the object."""

    def __init__(self, support_vectors, dual_coef, intercept, gamma, classes, scale=None, center=None):
        sv = np.ascontiguousarray(support_vectors, dtype=np.float64)
        if sv.ndim != 2:
            raise ValueError('support_vectors must be [n_sv, n_features]')
        self.support_vectors = sv
        self.dual_coef = np.ascontiguousarray(dual_coef, dtype=np.float64).reshape(-1)
        if len(self.dual_coef) != len(sv):
            raise ValueError(f'{len(self.dual_coef)} dual coefficients for {len(sv)} support vectors')
        self.intercept = float(np.asarray(intercept, dtype=np.float64).reshape(-1)[0])
        self.gamma = float(gamma)
        cls = np.asarray(classes).reshape(-1)
        if len(cls) != 2:
            raise ValueError(f'a two-class model is needed, got classes {cls.tolist()}')
        self.classes = (int(cls[0]), int(cls[1]))
        F = sv.shape[1]
        self.scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
        self.center = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(-1)
        for name, v in (('scale', self.scale), ('center', self.center)):
            if v is not None and len(v) != F:
                raise ValueError(f'{name} has {len(v)} entries for {F} features')
        self._handle, self._handle_dev = None, None

    # ---- construction --------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, support_vectors, dual_coef, intercept, gamma, classes, scale=None, center=None):
        return cls(support_vectors, dual_coef, intercept, gamma, classes, scale=scale, center=center)

    @classmethod
    def from_sklearn(cls, scaler, clf):
        """From a fitted ``RobustScaler`` (or None) and a fitted two-class ``SVC(kernel='rbf')``: attributes only
        (``scale_``, ``center_``, ``support_vectors_``, ``dual_coef_``, ``intercept_``, ``_gamma``, ``classes_``)."""
        kernel = getattr(clf, 'kernel', None)
        if kernel != 'rbf':
            raise ValueError(f'only RBF kernels are served on the device, got kernel={kernel!r}')
        classes = np.asarray(clf.classes_).reshape(-1)
        dual = np.asarray(clf.dual_coef_, dtype=np.float64)
        if len(classes) != 2 or dual.ndim != 2 or dual.shape[0] != 1:
            raise ValueError(f'a two-class model is needed, got classes {classes.tolist()}')
        gamma = getattr(clf, '_gamma', None)          # the resolved number; clf.gamma may be the string 'scale'
        if gamma is None:
            raise ValueError('the classifier has no resolved _gamma: is it fitted?')
        scale = getattr(scaler, 'scale_', None) if scaler is not None else None
        center = getattr(scaler, 'center_', None) if scaler is not None else None
        return cls(clf.support_vectors_, dual[0], np.asarray(clf.intercept_).reshape(-1)[0], float(gamma), classes,
                   scale=scale, center=center)

    @classmethod
    def fit(cls, X, y, **kwargs):
        """``scaler.fit`` / ``scaler.transform`` / ``clf.fit`` of pitch_model.py:48-50 on the device: see
        ``features.svmfit.fit_pitch_svm`` (classes, C, gamma, tol, max_iter, with_centering, quantile_range, valid, scaler)."""
        from .svmfit import fit_pitch_svm
        return fit_pitch_svm(X, y, **kwargs)

    def save(self, path):
        """The arrays as an .npz file (``load`` reads it back)."""
        extra = {k: v for k, v in (('scale', self.scale), ('center', self.center)) if v is not None}
        with open(path, 'wb') as f:
            np.savez(f, support_vectors=self.support_vectors, dual_coef=self.dual_coef, intercept=np.float64(self.intercept),
                     gamma=np.float64(self.gamma), classes=np.array(self.classes, dtype=np.int64), **extra)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z['support_vectors'], z['dual_coef'], z['intercept'], float(z['gamma']), z['classes'],
                       scale=z['scale'] if 'scale' in z.files else None, center=z['center'] if 'center' in z.files else None)

    # ---- the native handle ---------------------------------------------------------------------------------------
    @property
    def n_features(self):
        return self.support_vectors.shape[1]

    @property
    def n_sv(self):
        return self.support_vectors.shape[0]

    def descriptor(self):
        """The dsp_svm_desc of these arrays (it points into them: keep the object alive while it is used)."""
        d = nat.SvmDesc()
        d.n_features, d.n_sv = self.n_features, self.n_sv
        d.class0, d.class1 = self.classes
        d.gamma, d.intercept = self.gamma, self.intercept
        d.h_center = None if self.center is None else self.center.ctypes.data
        d.h_scale = None if self.scale is None else self.scale.ctypes.data
        d.h_sv, d.h_dual = self.support_vectors.ctypes.data, self.dual_coef.ctypes.data
        return d

    def handle(self):
        dev = nat.current_device()
        if self._handle is None or self._handle_dev != dev:
            self._drop_handle()
            d, h = self.descriptor(), nat.c_vp(0)
            nat.check_value(nat.load().dsp_svm_create(nat.C.byref(d), nat.C.byref(h)), 'invalid model')
            self._handle, self._handle_dev = h.value, dev
        return self._handle

    def _drop_handle(self):
        if getattr(self, '_handle', None) is not None:
            try:                                    # (at interpreter shutdown even the import may fail)
                nat.load().dsp_svm_destroy(self._handle)
            except Exception:
                pass
            self._handle, self._handle_dev = None, None

    __del__ = _drop_handle

    def __getstate__(self):
        d = self.__dict__.copy()
        d['_handle'], d['_handle_dev'] = None, None      # a copy builds its own handle
        return d

    # ---- evaluation ----------------------------------------------------------------------------------------------
    def _run(self, X, want_label):
        """-> (decision, label) as device tensors (input: device tensor) or host arrays (anything else)."""
        import torch
        nat.require_device()
        on_device = _is_device_tensor(X)
        dev = X.device if on_device else torch.device('cuda', nat.current_device())
        if on_device:
            if X.dtype != torch.float64:
                raise TypeError(f'features on the device must be float64, got {X.dtype}')
            x = X
        else:
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float64))).to(dev)
        if x.dim() == 1:
            x = x.reshape(1, -1)
        if x.dim() != 2 or x.shape[1] < self.n_features:
            raise ValueError(f'features must be [n, >= {self.n_features}], got {tuple(x.shape)}')
        if x.stride(1) != 1:
            x = x.contiguous()
        n = x.shape[0]
        dec = torch.empty(n, dtype=torch.float64, device=dev)
        lab = torch.empty(n, dtype=torch.int32, device=dev) if want_label else None
        if n:
            nat.check(nat.load().dsp_svm_decision_batch(self.handle(), x.data_ptr(), x.stride(0), n, dec.data_ptr(),
                                                        lab.data_ptr() if want_label else None, _torch_stream(dev)))
        if on_device:
            return dec, lab
        return dec.cpu().numpy(), (lab.cpu().numpy() if want_label else None)

    def decision_function(self, X):
        """SVC.decision_function(scaler.transform(X)): fp64 [n]; a device tensor in gives a device tensor out."""
        return self._run(X, False)[0]

    def predict(self, X):
        """SVC.predict(scaler.transform(X)): int32 [n] labels."""
        return self._run(X, True)[1]


def _as_rules(rules):
    """((label_a, label_b), threshold, PitchSVM) triples -> (ctypes array or None, n); keeps nothing alive itself."""
    rules = list(rules)
    if len(rules) > MAX_RULES:
        raise ValueError(f'at most {MAX_RULES} rules, got {len(rules)}')
    if not rules:
        return None, 0
    arr = (nat.EnsembleRule * len(rules))()
    for k, (labels, threshold, svm) in enumerate(rules):
        arr[k].label_a, arr[k].label_b = (int(v) for v in labels)
        arr[k].threshold = float(threshold)
        arr[k].svm = svm.handle()
    return arr, len(rules)


def ensemble_decide(logits, rules, feat=None, valid=None, stream=None):
    """model.py:156-157 + ensemble.py:49-53 for a batch, one launch.

    ``logits``: [B, C] fp32 device tensor (2 <= C <= 64, finite).  ``rules``: up to four ``((label_a, label_b), threshold,
    PitchSVM)``; a rule fires for a clip whose arg-max is one of its labels with softmax probability below the threshold.
    ``feat``: [B, >= F] fp64 device tensor (row stride free) or None without rules; ``valid``: int32 device tensor, one flag
    per clip (any stride, e.g. ``aux[:, 8]``), or None.  Returns device tensors (pred int32 [B], prob fp32 [B, C], used
    int32 [B]: 0 = no rule, r + 1 = rule r's SVM decided, -(r + 1) = rule r fired on invalid features and the classifier's
    label stands, decision fp64 [B]: the SVM's value where one was evaluated, else 0).  ``stream`` (a torch stream or a raw
    handle; default torch's current stream) takes the launch, the copy of any input whose inner stride is not 1, and the
    allocation of the outputs."""
    import torch
    if not _is_device_tensor(logits) or logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError('logits must be a [B, C] float32 device tensor')
    dev = logits.device
    with _on_stream(stream, dev):         # copies of strided inputs and the outputs: made on the stream of the launch
        if logits.stride(1) != 1:
            logits = logits.contiguous()
        B, C = logits.shape
        arr, n_rules = _as_rules(rules)
        p_feat, ld_feat, p_valid, ld_valid = None, 0, None, 0
        if n_rules:
            if feat is None or not _is_device_tensor(feat) or feat.dtype != torch.float64 or feat.dim() != 2 or feat.shape[0] != B:
                raise TypeError('feat must be a [B, F] float64 device tensor')
            if feat.stride(1) != 1:
                feat = feat.contiguous()
            p_feat, ld_feat = feat.data_ptr(), feat.stride(0)
            if valid is not None:
                if not _is_device_tensor(valid) or valid.dtype != torch.int32 or valid.dim() != 1 or valid.shape[0] != B:
                    raise TypeError('valid must be a [B] int32 device tensor')
                if B > 1 and valid.stride(0) < 1:
                    valid = valid.contiguous()
                p_valid, ld_valid = valid.data_ptr(), max(int(valid.stride(0)), 1)
        pred = torch.empty(B, dtype=torch.int32, device=dev)
        prob = torch.empty((B, C), dtype=torch.float32, device=dev)
        used = torch.empty(B, dtype=torch.int32, device=dev)
        dec = torch.empty(B, dtype=torch.float64, device=dev)
    st = _torch_stream(dev) if stream is None else _stream_ptr(stream)
    rc = nat.load().dsp_ensemble_decide_batch(logits.data_ptr(), logits.stride(0), B, C, arr, n_rules, p_feat, ld_feat, p_valid,
                                              ld_valid, pred.data_ptr(), prob.data_ptr(), used.data_ptr(), dec.data_ptr(), st)
    nat.check_value(rc, 'invalid argument')
    return pred, prob, used, dec


def _capture_scored(waves, prepare, score, census=False):
    """``_capture``; the warm call in front of the recording scores a batch, so the metrics block is put back behind it."""
    if score is None:
        return _capture(waves, prepare, census)
    saved = score[1].state.clone()
    g = _capture(waves, prepare, census)                       # (it synchronises its side stream behind the warm call)
    score[1].state.copy_(saved)
    return g


def _segments_tensor(lay, dev):
    """The segment table [B, 2] int64 of a pipeline layout THIS module owns, as a torch tensor (swapped in on first use; no
    launch of the layout is in flight then: a fresh layout has none, a cached one is swapped before its first launch)."""
    import torch
    if not isinstance(lay.d_seg, _TensorBuffer):
        lay.d_seg = _TensorBuffer(torch.zeros(2 * lay.n_utt, dtype=torch.int64, device=dev))
    return lay.d_seg.tensor.view(lay.n_utt, 2)


def _logits_of(out):
    import torch
    logits = out[0] if isinstance(out, (tuple, list)) else out
    return logits.detach().to(torch.float32)


def _score_spec(labels, metrics, device_route):
    """The ``labels=`` / ``metrics=`` keywords of ``run`` and ``capture`` -> (labels, metrics) or None; refusals need no device."""
    if labels is None and metrics is None:
        return None
    if not device_route:
        raise ValueError('labels= / metrics= are served by run(sync_free=True), run(capacity=) and capture(): the downloading run() '
                         'has a host round trip already, score its result on the host')
    if labels is None or metrics is None:
        raise ValueError('labels= and metrics= go together: the labels to score against and the features.metrics.Metrics to update')
    from .metrics import Metrics
    if not isinstance(metrics, Metrics):
        raise TypeError(f'metrics must be a features.metrics.Metrics, not {type(metrics).__name__}')
    import torch
    if not (_is_device_tensor(labels) and labels.dtype == torch.int64 and labels.dim() == 1 and labels.is_contiguous()):
        raise TypeError('labels must be a contiguous [B] int64 device tensor: it is read in place (on every replay of a graph)')
    return labels, metrics


class _EnsembleTail:
    """What ``EnsembleBatch`` and ``MixedRateEnsembleBatch`` (``head``, ``rules``, ``coeff``) share: everything behind the
    front end's launches."""

    def _tail(self, inp, d_len0, host, groups, head_kwargs, arenas=None, score=None):
        """The head, per rate group the pre-emphasised trim and the five pitch features, ONE gate launch over the batch, and
        the namespace of ``run`` -- launches on torch's current stream.  ``host``: the (len0, endpoints) arrays the front
        end downloaded, or None: they stay on the device -- the head is called with ``device_len=True`` on ``d_len0``,
        ``n_clamped`` counts what it had to clamp, and torch copies the endpoints from the groups' segment tables
        (``_segments_tensor``).  ``groups``: (layout, contiguous wave tensor, rate, d_index) per rate; ``d_index``: the
        group's batch positions (int32 device tensor), or None where the group is the whole batch and its rows are written
        in place.  ``arenas``: one dict per group for the pitch chain's buffers, or None for library scratch.  ``score``:
        ``_score_spec``'s pair or None: ONE more launch behind the gate scores ``pred`` -- the ensemble's label -- against the labels
        and takes the loss from ``logits`` (``Metrics.update``)."""
        import torch
        from .pitch import N_AUX, pitch_features_device
        lib = nat.load()
        dev, B = inp.device, inp.shape[1]
        st = _torch_stream(dev)
        extra = {}
        if host is None:
            from .classifier import head_length_info
            len0 = d_len0
            logits = _logits_of(self.head(inp, len0, device_len=True, **head_kwargs))
            extra['n_clamped'] = head_length_info(len0, inp.shape[0], 1)[2][2:3]
        else:
            len0, endpoints = host
            logits = _logits_of(self.head(inp, len0, **head_kwargs))
        # the pitch chain's other buffers are library scratch that the next call reuses (or the arena's): the two results
        # this call returns are torch's
        feat = torch.empty((B, 5), dtype=torch.float64, device=dev)
        aux = torch.empty((B, N_AUX), dtype=torch.int32, device=dev)
        trimmed = []
        for k, (lay, wave, rate, d_index) in enumerate(groups):
            n = lay.n_utt
            trim = torch.empty(max(lay.total_samples, 1), dtype=torch.float32, device=dev)
            nat.check(lib.dsp_trim_preemph_batch(wave.data_ptr(), _wave_dtype_of(wave), lay.vad.p_sample, lay.d_seg.ptr,
                                                 lay.d_dst_off.ptr, n, self.coeff, trim.data_ptr(), st))
            one = d_index is None
            feat_g = feat if one else torch.empty((n, 5), dtype=torch.float64, device=dev)
            aux_g = aux if one else torch.empty((n, N_AUX), dtype=torch.int32, device=dev)
            pitch_features_device(trim.data_ptr(), lay.d_dst_off.ptr, n, lay.total_samples, rate, stream=st,
                                  d_feat=feat_g.data_ptr(), d_aux=aux_g.data_ptr(), arena=None if arenas is None else arenas[k])
            if not one:                           # five doubles and nine ints per clip
                pos = d_index.long()
                feat.index_copy_(0, pos, feat_g)
                aux.index_copy_(0, pos, aux_g)
            trimmed.append(trim)
        valid = aux[:, N_AUX - 1]
        pred, prob, used, dec = ensemble_decide(logits, self.rules, feat, valid, stream=st)
        if score is not None:
            score[1].update(logits, score[0], pred)
        if host is None:
            endpoints = torch.empty((B, 2), dtype=torch.int64, device=dev)
            for lay, _, _, d_index in groups:
                seg = _segments_tensor(lay, dev)
                if d_index is None:
                    endpoints.copy_(seg)
                else:
                    endpoints.index_copy_(0, d_index.long(), seg)
        return types.SimpleNamespace(pred=pred, prob=prob, used=used, decision=dec, logits=logits, feat=feat, valid=valid,
                                     endpoints=endpoints, inp=inp, len0=len0, _clips=[g[1] for g in groups], _trimmed=trimmed,
                                     **extra)


class EnsembleBatch(_EnsembleTail):
    """ensemble.EnsembleModel.test's loop body (ensemble.py:48-53) for a batch of raw clips, device-resident.

    ``head``: any callable ``head(inp, len0, **kwargs)`` returning the logits [B, C] first (``HMRNNHead``; the caller passes
    ``dropout=False`` and the like through ``run``).  ``rules``: ``((label_a, label_b), threshold, PitchSVM)`` triples, e.g.
    built from ``REFERENCE_RULES``."""

    def __init__(self, rate, head, rules, frame=0.03, step=0.01, coeff=0.97):
        from .model_glue import ModelFeatureBatch
        self.rate, self.head, self.rules, self.coeff = rate, head, list(rules), float(coeff)
        self.features = ModelFeatureBatch(rate, frame=frame, step=step)
        self._layouts = {}

    def _layout(self, so):
        """The pipeline layout of this batch shape, owned by this object: its d_seg / d_dst_off stay valid after
        ModelFeatureBatch.run returns (a few shapes are kept, the most recently used last)."""
        key = (nat.current_device(), so.tobytes())
        lay = self._layouts.pop(key, None)
        if lay is None:
            lay = self.features.pipe.prepare(so, 0)
            while len(self._layouts) >= 4:
                self._layouts.pop(next(iter(self._layouts)))
        self._layouts[key] = lay
        return lay

    def run(self, waves, sample_offsets, sync_free=False, capacity=None, labels=None, metrics=None, **head_kwargs):
        """``labels=`` (int64 [B] device tensor) with ``metrics=`` (a ``features.metrics.Metrics``), on the sync-free routes only: one
        more launch behind the gate scores ``pred`` against the labels and adds the loss of ``logits`` to the epoch state.
        ``capacity=N``: the sync-free chain on a capacity layout cached per (B, N) -- the launches ``capture(...,
        capacity=N)`` records, queued eagerly: ``waves`` is a contiguous device tensor of exactly N samples (ValueError
        otherwise), ``sample_offsets`` ([B + 1], host array or device tensor) any B lengths >= 1 that sum to at most N; no
        layout is built, uploaded or synchronised per batch shape.  ``status`` (int32 [1]) is added to the namespace.
        ``waves``: concatenated clips, a 1-D host array (int16 or float) or device tensor (int16 / float32);
        ``sample_offsets`` [B + 1].  Returns a namespace of device tensors: pred int32 [B] (the ensemble's labels), prob fp32
        [B, C], used int32 [B], decision fp64 [B] (see ``ensemble_decide``), logits, feat fp64 [B, 5] and valid int32 [B]
        (the pitch features), endpoints int64 [B, 2] (host array, samples), len0 [B] (host array).  This call downloads len0
        and the endpoints between the front end and the head: one host synchronisation per batch.
        ``sync_free=True``: nothing is synchronised -- the head is called with ``device_len=True`` (so it must be one of
        features/classifier.py's), ``len0`` (int32) and ``endpoints`` are device tensors, and ``n_clamped`` (int32 [1]) counts
        the lengths the head had to clamp."""
        import torch
        score = _score_spec(labels, metrics, sync_free or capacity is not None)
        nat.require_device()
        if capacity is not None:
            from .pipeline import check_capacity_wave
            check_capacity_wave(waves, capacity)
            _wave_dtype_of(waves)
            B = int(sample_offsets.shape[0] if torch.is_tensor(sample_offsets) else len(sample_offsets)) - 1
            lay = self.features.pipe._capacity_layout(B, capacity, 0)
            lay.write_offsets(sample_offsets)
            ns = self._chain(waves, lay, self._m0(lay, waves.device), None, head_kwargs, score)
            ns.status = lay.status
            return ns
        so = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        # ONE contiguous device copy of the clips, held until the call returns: endpointing, the feature kernels and the
        # pre-emphasised trim all read this buffer
        if _is_device_tensor(waves):
            clips = waves.reshape(-1).contiguous()
        else:
            host, _ = nat.as_wave(np.asarray(waves).reshape(-1))
            clips = torch.from_numpy(host).to(torch.device('cuda', nat.current_device()))
        _wave_dtype_of(clips)                              # TypeError for anything but int16 / float32
        lay = self._layout(so)
        if sync_free:
            return self._chain(clips, lay, self._m0(lay, clips.device), None, head_kwargs, score)
        inp, len0, endpoints = self.features.run(clips, layout=lay)
        return self._tail(inp, None, (len0, endpoints), [(lay, clips, self.rate, None)], head_kwargs)

    def pitch_rows(self, waves, sample_offsets):
        """The rows ``PitchModel.train`` collects (pitch_model.py:38-41) for a batch of raw clips -> (feat [B, 5] fp64, valid
        [B] int32), device tensors, nothing synchronised: the front end's launches for the endpoints (its rows go to scratch;
        no classifier input is laid out, no head is called), then the trim and the pitch features of ``_tail``."""
        import torch
        from .pitch import N_AUX, pitch_features_device
        nat.require_device()
        so = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        if _is_device_tensor(waves):
            clips = waves.reshape(-1).contiguous()
        else:
            host, _ = nat.as_wave(np.asarray(waves).reshape(-1))
            clips = torch.from_numpy(host).to(torch.device('cuda', nat.current_device()))
        dtype, dev = _wave_dtype_of(clips), clips.device
        lay = self._layout(so)
        m0 = self._m0(lay, dev)
        stream = torch.cuda.current_stream(dev)
        self.features.pipe.launch(clips.data_ptr(), dtype, lay, m0.data_ptr(), stream, None, defer_c0_shift=True)
        st, B = _stream_ptr(stream), lay.n_utt
        trim = torch.empty(max(lay.total_samples, 1), dtype=torch.float32, device=dev)
        nat.check(nat.load().dsp_trim_preemph_batch(clips.data_ptr(), dtype, lay.vad.p_sample, lay.d_seg.ptr, lay.d_dst_off.ptr, B,
                                                    self.coeff, trim.data_ptr(), st))
        feat = torch.empty((B, 5), dtype=torch.float64, device=dev)
        aux = torch.empty((B, N_AUX), dtype=torch.int32, device=dev)
        pitch_features_device(trim.data_ptr(), lay.d_dst_off.ptr, B, lay.total_samples, self.rate, stream=st, d_feat=feat.data_ptr(),
                              d_aux=aux.data_ptr())
        return feat, aux[:, N_AUX - 1].contiguous()

    def _m0(self, lay, dev):
        """The front end's [frames_bound, C] scratch for ``_chain``; the layout's segment table becomes a torch tensor."""
        import torch
        _segments_tensor(lay, dev)
        return torch.empty((max(lay.frames_bound, 1), self.features.pipe.features.C), dtype=torch.float32, device=dev)

    def _chain(self, clips, lay, m0, arena, head_kwargs, score=None):
        """The whole path as launches on torch's current stream, nothing synchronised, no device memory read from the host:
        front end (``ModelFeatureBatch.enqueue``), then ``_tail`` with the lengths on the device.  ``lay`` / ``m0``: a layout
        of this object and its scratch (``_m0``); ``arena``: the pitch chain's buffers (None: library scratch, for an eager
        call)."""
        import torch
        mfb, dev, B = self.features, clips.device, lay.n_utt
        inp = torch.empty((mfb.max_len, B, 3 * mfb.pipe.features.C), dtype=torch.float32, device=dev)
        len0 = torch.empty(B, dtype=torch.int32, device=dev)
        mfb.enqueue(clips.data_ptr(), _wave_dtype_of(clips), lay, m0.data_ptr(), inp.data_ptr(), len0.data_ptr(),
                    torch.cuda.current_stream(dev))
        return self._tail(inp, len0, None, [(lay, clips, self.rate, None)], head_kwargs, None if arena is None else [arena], score)

    def capture(self, waves, sample_offsets, capacity=None, labels=None, metrics=None, census=False, **head_kwargs):
        """``census=True`` attaches ``g.census``, the node census of the recorded graph (features/graphcheck.py); the default records
        exactly as before.  ``labels=`` / ``metrics=`` as ``run``: the scoring launch is recorded behind the gate, ``labels`` is read in place on every
        replay, and ``capture`` itself leaves the metrics block as it found it.
        ONE HIP graph of the whole path over device-resident ``waves`` (a contiguous tensor, int16 / float32):
        ``g = eb.capture(waves, so, dropout=False)``; write new clips into ``waves`` -- of the same lengths, unless the graph
        was recorded with ``capacity=`` -- and call
        ``g.replay()`` -> the namespace of ``run(sync_free=True)``, every field a device tensor, valid after the current
        stream's work.  One eager call runs first (it builds the native handles and the layout's index tables and fills the
        graph's own arena).  The graph object owns every buffer its kernels touch -- the layout, the front end's scratch,
        the pitch chain's buffers and FIR taps -- so no later call of the library can free or overwrite what a replay reads.
        The graph reads ``waves`` at its address: a non-contiguous view raises ValueError; the head must accept
        ``device_len=True``.

        ``capacity=N``: ``waves`` is a contiguous 1-D tensor of exactly N samples (ValueError otherwise) and ``so`` the offsets
        of the batch it holds now.  The graph then serves ANY B = len(so) - 1 clips whose lengths are >= 1 and sum to at most
        N: write the clips into ``waves`` and their [B + 1] offsets into ``g.sample_offsets`` (int64 device tensor), replay;
        samples behind ``offsets[B]`` are ignored, ``g.status`` (int32 [1]) is 0 for a valid table.  The batch layout -- the
        sanitised offsets, the frame offsets, the VAD kernel's index tables -- is rebuilt by two launches at the head of the
        recorded sequence (``CapacityLayout``); every grid and buffer behind is sized by the capacity."""
        box = []
        score = _score_spec(labels, metrics, True)

        def prepare():
            nat.require_device()
            so = np.ascontiguousarray(sample_offsets, dtype=np.int64)
            if capacity is None:
                clips = waves.reshape(-1)                      # a view: the same memory
                _wave_dtype_of(clips)                          # TypeError for anything but int16 / float32
                lay = self.features.pipe.prepare(so, 0)        # the graph's own: nothing else launches on its tables
            else:
                from .pipeline import check_capacity_wave
                check_capacity_wave(waves, capacity)
                clips = waves
                _wave_dtype_of(clips)
                lay = self.features.pipe.prepare_capacity(len(so) - 1, capacity, 0)
                lay.write_offsets(so)
                box.append(lay)
            m0, arena = self._m0(lay, waves.device), {}
            return (lambda: self._chain(clips, lay, m0, arena, head_kwargs, score)), [lay, m0, arena, clips, list(self.rules), score]
        g = _capture_scored(waves, prepare, score, census)
        if box:
            g.sample_offsets, g.status = box[0].sample_offsets_in, box[0].status
        return g


class MixedRateEnsembleBatch(_EnsembleTail):
    """EnsembleBatch for a batch whose clips have different sample rates (reader.mini_batch_iterator shuffles the file list,
    reader.py:80; ensemble.py:48-53 and pitch_model.py:54-61 treat every clip at its own rate): the classifier's features
    from MixedRateFeatureBatch, ONE ``head`` call on the whole batch, the pre-emphasised trim and the five pitch features per
    rate group with their rows placed in batch order, and one gate launch over the batch."""

    def __init__(self, head, rules, frame=0.03, step=0.01, coeff=0.97):
        from .model_glue import MixedRateFeatureBatch
        self.head, self.rules, self.coeff = head, list(rules), float(coeff)
        self.features = MixedRateFeatureBatch(frame=frame, step=step)

    def run(self, waves, sample_offsets=None, rates=None, sync_free=False, capacity=None, labels=None, metrics=None, **head_kwargs):
        """``labels=`` / ``metrics=`` as ``EnsembleBatch.run`` (with ``sync_free=True``).
        ``capacity=``: NotImplementedError (``MixedRateFeatureBatch.capture`` says why).
        ``waves`` / ``sample_offsets`` / ``rates`` as MixedRateFeatureBatch.run.  Returns the namespace of EnsembleBatch.run,
        every row in batch order; ``sync_free=True`` as there (device input: no synchronisation once the plan of the batch
        shape exists)."""
        from .model_glue import _no_mixed_capacity
        _no_mixed_capacity(capacity)
        score = _score_spec(labels, metrics, sync_free)
        mr = self.features
        if sync_free:
            import torch
            clips, so, r = mr._inputs(waves, sample_offsets, rates)
            on_device = _is_device_tensor(clips)
            dev = clips.device if on_device else torch.device('cuda', nat.current_device())
            plan = mr._plan(so, r, dev, on_device)       # this object's: its segment tables become torch's before the launches
            return self._chain(waves, so, r, plan, dev, None, head_kwargs, score)
        ctx = mr._launch(waves, sample_offsets, rates)
        return self._after(ctx, mr._finish(ctx), head_kwargs, None)

    def _after(self, ctx, host, head_kwargs, arenas, score=None):
        """``_tail`` behind the launches of ``MixedRateFeatureBatch._launch``: one contiguous device buffer per rate."""
        groups = [(g.lay, wave, g.rate, g.d_index) for g, wave in zip(ctx.plan.groups, ctx.group_waves)]
        ns = self._tail(ctx.inp, ctx.len0, host, groups, head_kwargs, arenas, score)
        ns._hold = ctx.hold                       # the temporaries of the launches (torch tensors: released in stream order)
        return ns

    def _chain(self, waves, so, rates, plan, dev, arenas, head_kwargs, score=None):
        """The whole path on ``plan`` with nothing synchronised: the lengths and the endpoints stay on the device."""
        for g in plan.groups:
            _segments_tensor(g.lay, dev)
        return self._after(self.features._launch(waves, so, rates, plan=plan), None, head_kwargs, arenas, score)

    def capture(self, waves, sample_offsets, rates, capacity=None, labels=None, metrics=None, **head_kwargs):
        """``labels=`` / ``metrics=`` as ``EnsembleBatch.capture``.  ``EnsembleBatch.capture`` for a mixed-rate batch: ONE HIP graph of the front end's sub-pipelines (queued one after
        the other: a chain, no forked branches), the head with ``device_len=True``, and per rate group the trim and the pitch
        features, then the gate.  ``waves``: a contiguous 1-D device tensor (a non-contiguous one raises ValueError);
        ``replay()`` -> the namespace of ``run(sync_free=True)``, rows in batch order.  The graph object owns the plan, every
        group's layout and pitch arena, and the temporaries of the launches.  (The optional ``use_pitch`` / ``use_timefeat``
        streams are not part of the capture.)
        ``capacity=`` raises NotImplementedError: the grouping by rate is host logic over the rates, so a mixed-rate graph
        stays bound to its lengths and rates (``MixedRateFeatureBatch.capture``)."""
        from .model_glue import _MixedPlan, _no_mixed_capacity
        _no_mixed_capacity(capacity)
        score = _score_spec(labels, metrics, True)

        def prepare():
            _, so, r = self.features._inputs(waves, sample_offsets, rates)
            plan = _MixedPlan(self.features, so, r, waves.device, True)    # the graph's own: nothing else writes its tables
            arenas = [{} for _ in plan.groups]
            return (lambda: self._chain(waves, so, r, plan, waves.device, arenas, head_kwargs, score)), [plan, arenas, list(self.rules),
                                                                                                        score]
        return _capture_scored(waves, prepare, score)


# ---- the ensemble over mixed-rate capacity batches: one recorded chain for any lengths and any assignment of rates ----------
# MixedRateEnsembleBatch above is bound to a batch's lengths AND rates (its plan is host logic).  Here the front end is
# MixedRateCapacityBatch -- every table rate owns a group of exactly B slots, its clips first, then pad clips of PAD_SAMPLES
# samples -- and the pitch tail runs per group over ALL B slots, pads included (DESIGN 7.22 reads every kernel of it at n = 1);
# dsp_scatter_group_rows_batch then brings the rows of the real slots back to batch order, one launch for ``feat`` and one
# for ``aux``, where the exact-shape route uses index_copy_.

class _MixedEnsembleArena:
    """What one (B, N, sample type) of a MixedRateCapacityEnsembleBatch launches on beside the front end's arena (``mixed``):
    per table rate a pre-emphasised trim buffer of N + B * PAD_SAMPLES fp32, the group's ``feat_g`` [B, 5] fp64 and ``aux_g``
    [B, 9] int32 and a dict for the pitch chain's buffers (features/pitch.py: ``_slot``), and the host arrays of table pointers
    the two scatter launches take."""

    def __init__(self, mixed):
        import ctypes as C
        import torch
        from .model_glue import PAD_SAMPLES
        from .pitch import N_AUX
        self.mixed, dev, B, G = mixed, mixed.dev, mixed.B, mixed.G
        cap = mixed.N + B * PAD_SAMPLES
        self.trim = [torch.zeros(cap, dtype=torch.float32, device=dev) for _ in range(G)]
        self.feat = [torch.zeros((B, 5), dtype=torch.float64, device=dev) for _ in range(G)]
        self.aux = [torch.zeros((B, N_AUX), dtype=torch.int32, device=dev) for _ in range(G)]
        self.pitch = [{} for _ in range(G)]
        self.p_feat = (C.c_void_p * G)(*[t.data_ptr() for t in self.feat])
        self.p_aux = (C.c_void_p * G)(*[t.data_ptr() for t in self.aux])


class MixedRateCapacityEnsembleBatch:
    """``EnsembleBatch``'s capacity route over a ``model_glue.MixedRateCapacityBatch``: ensemble.py:48-53 for ANY batch of B clips
    at the rates of a fixed table whose lengths are >= 1 and sum to at most N, as ONE launch sequence that reads lengths and
    rates from device memory.  Capacity routes only (``run`` and ``capture`` need ``capacity=N``); no jitter, no optional
    streams.  The sequence, one chain:

      MixedRateCapacityBatch.enqueue   grouping, gather, the groups' front ends, the endpoints back to batch order
      head(inp, len0, device_len=True) ONE call on the whole batch
      per table rate                   dsp_trim_preemph_batch on the group's wave buffer and capacity layout, then
                                       pitch_features_device over all B slots of the group, pads included
      dsp_scatter_group_rows_batch     twice: the groups' ``feat`` and ``aux`` rows to batch order, pad slots skipped
      ensemble_decide                  the gate over the batch;  with ``labels=, metrics=`` the scoring launch behind it

    No index_copy_, no memset, no library scratch slot.  ``status`` is ``MixedRateCapacityBatch``'s (bit 4: a rate outside the
    table; that clip ran in group 0 and every result stays defined)."""

    def __init__(self, rates=(44100, 48000), head=None, rules=(), frame=0.03, step=0.01, coeff=0.97):
        from .model_glue import MixedRateCapacityBatch
        self.features = MixedRateCapacityBatch(rates, frame=frame, step=step)     # ValueError for a bad table, before any device work
        if head is None:
            raise TypeError('MixedRateCapacityEnsembleBatch needs a head')
        self.rates, self.head, self.rules, self.coeff = self.features.rates, head, list(rules), float(coeff)
        self._arenas = {}

    def _arena(self, n_utt, capacity, waves):
        """``run``: one arena per (device, B, N, sample type), a few kept, the most recently used last."""
        key = (waves.device.index, int(n_utt), int(capacity), str(waves.dtype))
        arena = self._arenas.pop(key, None)
        if arena is None:
            arena = _MixedEnsembleArena(self.features.prepare(n_utt, capacity, waves))
            while len(self._arenas) >= 4:
                self._arenas.pop(next(iter(self._arenas)))
        self._arenas[key] = arena
        return arena

    def _chain(self, waves, arena, head_kwargs, score=None):
        """The whole path as launches on torch's current stream: nothing synchronised, no device memory read from the host."""
        import torch
        from .classifier import head_length_info
        from .pitch import N_AUX, pitch_features_device
        lib, mc, mixed = nat.load(), self.features, arena.mixed
        dev, B, G = waves.device, mixed.B, mixed.G
        stream = torch.cuda.current_stream(dev)
        st, dtype = _stream_ptr(stream), _wave_dtype_of(waves)
        inp, len0, endpoints = mc._outputs(B, dev)
        mc.enqueue(waves, mixed, inp, len0, endpoints, False, stream)
        logits = _logits_of(self.head(inp, len0, device_len=True, **head_kwargs))
        n_clamped = head_length_info(len0, inp.shape[0], 1)[2][2:3]
        for g, mfb in enumerate(mc.groups):
            lay = mixed.lays[g]
            nat.check(lib.dsp_trim_preemph_batch(mixed.waves[g].data_ptr(), dtype, lay.vad.p_sample, lay.d_seg.ptr, lay.d_dst_off.ptr,
                                                 B, self.coeff, arena.trim[g].data_ptr(), st))
            pitch_features_device(arena.trim[g].data_ptr(), lay.d_dst_off.ptr, B, lay.total_samples, mfb.rate, stream=st,
                                  d_feat=arena.feat[g].data_ptr(), d_aux=arena.aux[g].data_ptr(), arena=arena.pitch[g])
        feat = torch.empty((B, 5), dtype=torch.float64, device=dev)
        aux = torch.empty((B, N_AUX), dtype=torch.int32, device=dev)
        nat.check(lib.dsp_scatter_group_rows_batch(arena.p_feat, mixed.p_dst_col, B, G, 5 * 8, feat.data_ptr(), st))
        nat.check(lib.dsp_scatter_group_rows_batch(arena.p_aux, mixed.p_dst_col, B, G, N_AUX * 4, aux.data_ptr(), st))
        valid = aux[:, N_AUX - 1]
        pred, prob, used, dec = ensemble_decide(logits, self.rules, feat, valid, stream=st)
        if score is not None:
            score[1].update(logits, score[0], pred)
        return types.SimpleNamespace(pred=pred, prob=prob, used=used, decision=dec, logits=logits, feat=feat, valid=valid,
                                     endpoints=endpoints, inp=inp, len0=len0, n_clamped=n_clamped, status=mixed.status)

    def _check(self, waves, sample_offsets, capacity):
        from .pipeline import check_capacity_wave
        if capacity is None:
            raise ValueError('MixedRateCapacityEnsembleBatch serves capacity routes only: pass capacity=N '
                             '(MixedRateEnsembleBatch.run takes exact shapes)')
        check_capacity_wave(waves, capacity)
        _wave_dtype_of(waves)
        return self.features._n_utt(sample_offsets)

    def run(self, waves, sample_offsets, rates, capacity=None, labels=None, metrics=None, **head_kwargs):
        """Eager and sync-free: ``waves`` a contiguous device tensor of exactly ``capacity`` = N samples (int16 / float32;
        ValueError otherwise), ``sample_offsets`` [B + 1] and ``rates`` [B] host arrays or device tensors.  -> the namespace of
        ``EnsembleBatch.run(sync_free=True)`` plus ``status``, every row in batch order: exactly the launches ``capture`` records,
        on an arena cached per (device, B, N, sample type).  ``labels=`` / ``metrics=`` as ``EnsembleBatch.run``."""
        score = _score_spec(labels, metrics, True)
        B = self._check(waves, sample_offsets, capacity)      # (the refusals need no device)
        nat.require_device()
        arena = self._arena(B, capacity, waves)
        arena.mixed.write(sample_offsets, rates, None)
        return self._chain(waves, arena, head_kwargs, score)

    def capture(self, waves, sample_offsets, rates, capacity=None, labels=None, metrics=None, census=False, **head_kwargs):
        """ONE HIP graph of ``run``'s launches over ``waves`` (contiguous [N] device tensor) and the batch it holds now.  Before a
        ``g.replay()`` write the next batch's clips into ``waves``, its offsets into ``g.sample_offsets`` (int64 [B + 1]) and its
        rates into ``g.rates`` (int32 [B]): ANY B clips at the table's rates whose lengths are >= 1 and sum to at most N are
        served, in any order of rates.  ``replay()`` -> the namespace of ``run``; ``g.status`` as there.  The graph owns every
        buffer its launches touch: the front end's arena, the groups' trim buffers, rows and pitch arenas, and the batch-order
        outputs.  ``labels=`` / ``metrics=`` / ``census=`` as ``EnsembleBatch.capture``."""
        score = _score_spec(labels, metrics, True)
        if capacity is None:
            self._check(waves, sample_offsets, capacity)
        box = []

        def prepare():
            nat.require_device()
            B = self._check(waves, sample_offsets, capacity)
            arena = _MixedEnsembleArena(self.features.prepare(B, capacity, waves))      # the graph's own
            arena.mixed.write(sample_offsets, rates, None)
            box.append(arena)
            return (lambda: self._chain(waves, arena, head_kwargs, score)), [arena, list(self.rules), score, self.head]
        g = _capture_scored(waves, prepare, score, census)
        mixed = box[0].mixed
        g.sample_offsets, g.rates, g.status = mixed.sample_offsets, mixed.rates, mixed.status
        return g
