"""NumPy restatement of the ensemble's last step, in this project's own words (fp64 throughout): the decision function of
a RobustScaler + two-class RBF SVC from their public arrays, the softmax / arg-max of the classifier's logits and the
confidence gate of the reference's loop.  tests/test_ensemble_host.py pins it to scikit-learn's stored decisions and to
the predictions the reference's own loop produced; the GPU tests then use it on shapes no fixture covers."""
import numpy as np


def preemph_trim(x, l, r, coeff=0.97):
    """preemphasis over the whole clip, then [l:r] -> fp64."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0:
        return x
    y = np.concatenate([x[:1], x[1:] - coeff * x[:-1]])
    return y[l:r]


def decision(model, X):
    """model: dict with support_vectors [n, F], dual_coef [n], intercept, gamma and optionally scale / center [F].
    X [m, >= F] -> dec [m] = sum_i dual_i exp(-gamma |z - sv_i|^2) + intercept, z = (x - center) / scale."""
    sv = np.asarray(model['support_vectors'], dtype=np.float64)
    F = sv.shape[1]
    z = np.asarray(X, dtype=np.float64)[:, :F]
    if model.get('center') is not None:
        z = z - np.asarray(model['center'], dtype=np.float64)
    if model.get('scale') is not None:
        z = z / np.asarray(model['scale'], dtype=np.float64)
    d2 = ((z[:, None, :] - sv[None, :, :]) ** 2).sum(axis=2)
    return np.exp(-float(model['gamma']) * d2) @ np.asarray(model['dual_coef'], dtype=np.float64) + float(model['intercept'])


def predict(model, X):
    c = model['classes']
    return np.where(decision(model, X) > 0, int(c[1]), int(c[0])).astype(np.int32)


def decision_bound(model):
    """The bound on |device - reference| of one decision: 2 (16 + n_sv) 2^-52 (sum |dual| + |intercept|)."""
    dual = np.asarray(model['dual_coef'], dtype=np.float64)
    return 2.0 * (16 + len(dual)) * 2.0 ** -52 * (np.abs(dual).sum() + abs(float(model['intercept'])))


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def gate(logits, rules, feat=None, valid=None, prob=None):
    """logits [B, C] fp32; rules: ((label_a, label_b), threshold, model).  -> (pred, used, decision): the arg-max (lowest
    index on a tie), overruled by the first rule whose pair holds it while the fp32 probability, read as a double, is below
    the threshold -- by that rule's model where the clip's features are valid (used = r + 1), not at all where they are not
    (used = -(r + 1)).  ``prob``: the fp32 probabilities to gate on (default: softmax64 rounded to fp32)."""
    logits = np.asarray(logits, dtype=np.float32)
    B = len(logits)
    p32 = softmax64(logits).astype(np.float32) if prob is None else np.asarray(prob, dtype=np.float32)
    pred = np.argmax(logits, axis=1).astype(np.int32)          # numpy returns the first of equal maxima
    used = np.zeros(B, dtype=np.int32)
    dec = np.zeros(B, dtype=np.float64)
    for b in range(B):
        for r, (labels, threshold, model) in enumerate(rules):
            if int(pred[b]) in (int(labels[0]), int(labels[1])) and float(p32[b, pred[b]]) < float(threshold):
                if valid is None or valid[b]:
                    dec[b] = decision(model, np.asarray(feat)[b:b + 1])[0]
                    pred[b] = int(model['classes'][1]) if dec[b] > 0 else int(model['classes'][0])
                    used[b] = r + 1
                else:
                    used[b] = -(r + 1)
                break
    return pred, used, dec
