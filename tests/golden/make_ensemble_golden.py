#!/usr/bin/env python3
"""Generate tests/golden/ensemble_golden.npz: scikit-learn's own numbers for the two pitch SVMs and the predictions of the
ACTUAL reference loop (ensemble.EnsembleModel.test over pitch_model.PitchModel.test_iter) on tests/ensemble_cases.py.

Like make_pitch_golden.py this runs only where the reference checkout exists (default /root/reference; override with
REFERENCE_ROOT) and scikit-learn is installed; nothing of the reference is copied: it is imported from where it lies,
called on seeded synthetic inputs, and only numbers are stored.

    python tests/golden/make_ensemble_golden.py     # rewrites ensemble_golden.npz (+ ensemble_manifest.json)

(A) fits RobustScaler(with_centering=False) + SVC(kernel='rbf') for both label pairs, stores their public arrays and
    decision_function / predict on 512 queries each; refuses a model with a query of |decision| < 1e-6.
(B) drives EnsembleModel.test without data or pickles: the object is made with __new__, `mfcc_rnn` is a stub whose
    test_iter returns (arg-max list, torch.softmax rows) of the designed logits and keeps the list it returned -- the loop
    overwrites its entries in place, replaced ones come back as numpy.int64 --, `pitch_clf01` / `pitch_clf67` are
    PitchModel.__new__ objects carrying the fitted scaler / clf, `reader` yields one batch of (int16 clip, rate).  Stores
    the probabilities, the final predictions, which entries were replaced, the endpoints, the reference's pitch_feature
    rows and both models' decisions on them.  Refuses a clip whose single-precision track differs from the
    double-precision one, a gate probability within 1e-4 of its threshold and a used decision with |decision| < 1e-3.
(C) (l, r) and preemphasis(sig, 0.97)[l:r] as float64 for three of the clips.
"""
import contextlib
import io
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)

from make_pitch_golden import load_reference, single_precision_track  # noqa: E402


def fit_models(np):
    from sklearn.preprocessing import RobustScaler
    from sklearn.svm import SVC
    from ensemble_cases import PAIRS, svm_queries, svm_training_set
    out, fitted = {}, []
    for k, pair in enumerate(PAIRS):
        X, y = svm_training_set(k)
        scaler = RobustScaler(with_centering=False)
        clf = SVC(kernel='rbf')
        clf.fit(scaler.fit_transform(X), y)
        Q = svm_queries(k)
        dec = clf.decision_function(scaler.transform(Q))
        if np.min(np.abs(dec)) < 1e-6:
            raise SystemExit(f'model {pair}: a query has |decision| {np.min(np.abs(dec)):.2e} < 1e-6: pick another seed')
        assert list(clf.classes_) == list(pair) and scaler.center_ is None
        name = f'svm{pair[0]}{pair[1]}'
        out.update({f'{name}/scale': scaler.scale_, f'{name}/support_vectors': clf.support_vectors_,
                    f'{name}/dual_coef': clf.dual_coef_[0], f'{name}/intercept': np.float64(clf.intercept_[0]),
                    f'{name}/gamma': np.float64(clf._gamma), f'{name}/classes': np.asarray(clf.classes_, dtype=np.int64),
                    f'{name}/queries': Q, f'{name}/decision': dec,
                    f'{name}/predict': clf.predict(scaler.transform(Q)).astype(np.int64)})
        fitted.append((scaler, clf))
        print(name, 'n_sv', len(clf.support_vectors_), 'gamma', clf._gamma, 'sum|dual|', np.abs(clf.dual_coef_).sum(),
              'min|dec|', np.min(np.abs(dec)))
    return out, fitted


def run_gate(np, rp, fitted):
    import torch
    from ensemble_cases import PAIRS, THRESHOLDS, design_logits, make_clips
    os.makedirs('models', exist_ok=True)                 # the loop pickles a confusion matrix there
    with contextlib.redirect_stdout(io.StringIO()):
        import ensemble as ref_ensemble                  # noqa: the reference module
        from pitch_model import PitchModel
    clips, rate = make_clips()
    logits = design_logits()
    prob = torch.softmax(torch.from_numpy(logits), dim=1)
    assert prob.dtype == torch.float32

    class StubRNN:
        def test_iter(self, itr, total_iter, feat, label, files):
            _, pred = torch.max(torch.from_numpy(logits), 1)              # model.py:156-159
            self.pred = pred.numpy().tolist()
            return self.pred, prob.numpy().tolist()

    class StubReader:
        val_person = None

        def mini_batch_iterator(self, _):
            yield 1, 1, [(c, rate) for c in clips], [0] * len(clips), [''] * len(clips)

    m = ref_ensemble.EnsembleModel.__new__(ref_ensemble.EnsembleModel)
    m.mfcc_rnn, m.reader = StubRNN(), StubReader()
    for name, pair, (scaler, clf) in zip(('pitch_clf01', 'pitch_clf67'), PAIRS, fitted):
        pm = PitchModel.__new__(PitchModel)
        pm.label, pm.scaler, pm.clf = list(pair), scaler, clf
        setattr(m, name, pm)
    with contextlib.redirect_stdout(io.StringIO()):
        m.test()
    final = m.mfcc_rnn.pred
    replaced = np.array([isinstance(v, np.integer) for v in final])
    rnn_pred = np.argmax(logits, axis=1)
    # the margins of the gate, and the pieces behind the replaced entries
    p = prob.numpy()
    feats, ends, dec = [], [], np.zeros((len(clips), len(PAIRS)))
    for b, c in enumerate(clips):
        l, r = rp.basic_endpoint_detection(c, rate)
        y = rp.preemphasis(c, coeff=0.97)[l:r]
        p64, _ = rp.pitch_detect(y, rate)
        p32, _ = single_precision_track(rp, y.astype(np.float32).astype(np.float64), rate)
        if not np.array_equal(np.array(p64), p32):
            raise SystemExit(f'clip {b}: the single-precision track differs: pick another seed')
        with contextlib.redirect_stdout(io.StringIO()):
            feats.append(np.array(rp.pitch_feature(y, rate), dtype=np.float64))
        ends.append((l, r))
        for k, (scaler, clf) in enumerate(fitted):
            dec[b, k] = clf.decision_function(scaler.transform([feats[-1]]))[0]
    for b in range(len(clips)):
        fired = None
        for k, (pair, thr) in enumerate(zip(PAIRS, THRESHOLDS)):
            if rnn_pred[b] in pair:
                if abs(float(p[b, rnn_pred[b]]) - thr) < 1e-4:
                    raise SystemExit(f'clip {b}: probability {p[b, rnn_pred[b]]} is within 1e-4 of {thr}')
                if float(p[b, rnn_pred[b]]) < thr:
                    fired = k
        assert (fired is not None) == bool(replaced[b]), (b, fired, replaced[b])
        if fired is not None:
            if abs(dec[b, fired]) < 1e-3:
                raise SystemExit(f'clip {b}: |decision| {abs(dec[b, fired]):.2e} < 1e-3: pick another seed')
            assert final[b] == fitted[fired][1].classes_[int(dec[b, fired] > 0)]
    print('rnn  ', rnn_pred.tolist())
    print('final', [int(v) for v in final])
    print('replaced', replaced.astype(int).tolist())
    return dict(logits=logits, prob=p, final=np.array([int(v) for v in final], dtype=np.int64), replaced=replaced,
                rnn_pred=rnn_pred.astype(np.int64), endpoints=np.array(ends, dtype=np.int64), feat=np.array(feats),
                decision=dec), clips, ends


def main():
    import numpy as np
    from ensemble_cases import TRIM_CLIPS
    out, fitted = fit_models(np)             # (before the reference's modules are imported: the fits do not depend on them)
    rp = load_reference()                    # (changes into a scratch directory)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        gate, clips, ends = run_gate(np, rp, fitted)
    out.update({f'gate/{k}': v for k, v in gate.items()})
    for b in TRIM_CLIPS:
        l, r = ends[b]
        out[f'trim/{b}'] = np.asarray(rp.preemphasis(clips[b], coeff=0.97)[l:r], dtype=np.float64)
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    assert len(buf.getvalue()) < (1 << 20), len(buf.getvalue())
    path = os.path.join(HERE, 'ensemble_golden.npz')
    with open(path, 'wb') as f:
        f.write(buf.getvalue())
    import sklearn
    with open(os.path.join(HERE, 'ensemble_manifest.json'), 'w') as f:
        json.dump({'numpy': np.__version__, 'sklearn': sklearn.__version__,
                   'arrays': {k: [list(np.shape(v)), str(np.asarray(v).dtype)] for k, v in out.items()}}, f, indent=1, sort_keys=True)
    print(f'wrote {path}: {len(out)} arrays, {len(buf.getvalue()) / 1e6:.2f} MB')


if __name__ == '__main__':
    main()
