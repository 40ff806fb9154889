"""The ensemble path on the device (features/ensemble.py; dsp_svm_decision_batch, dsp_ensemble_decide_batch,
dsp_trim_preemph_batch) against scikit-learn's stored numbers, the reference loop's stored predictions
(tests/golden/ensemble_golden.npz) and, on shapes no fixture covers, the NumPy restatement that reproduces both
(tests/ensemble_ref.py, pinned in tests/test_ensemble_host.py).

Bounds: a decision within 2 (16 + n_sv) 2^-52 (sum |dual| + |intercept|) of scikit-learn / the restatement (a few ulp of
|dual_i| per term since u e^-u <= 1 / e, n ulp of the terms' magnitudes for the fp64 sum, twice for the two sides);
probabilities within 2^-24 of the fp64 softmax of the same fp32 logits (half an fp32 ulp below 1) and within 1e-6 of the
stored torch.softmax; labels, pred and used exact; trimmed pre-emphasised rows bitwise; pitch features of the end-to-end
run within the 1e-9 max(1, |ref|) tests/test_gpu_pitch_cepstrum.py applies to pitch_feature rows.

Where a label or a gate outcome is compared with the restatement on RANDOM inputs, rows whose decision lies within the
bound of 0 are left to the decision check (the fixtures keep their margins by construction: the maker refuses otherwise).
With 2 classes at most two rules with disjoint label sets exist, so that size runs with 0 and 2 rules instead of 0 and 4."""
import os

import numpy as np
import pytest

import ensemble_ref as ref
from conftest import record
from ensemble_cases import PAIRS, THRESHOLDS, TRIM_CLIPS, make_clips

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 4096
SENT32 = np.int32(0x7fc0beef)            # a quiet-NaN pattern: never a result


@pytest.fixture(scope='module')
def egold():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ensemble_golden.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def env():
    import types

    import torch
    from features import _native as nat
    from features import ensemble
    nat.require_device()
    return types.SimpleNamespace(nat=nat, lib=nat.load(), ens=ensemble, torch=torch, dev=torch.device('cuda', 0))


def model_of(egold, pair):
    name = f'svm{pair[0]}{pair[1]}'
    return {k: egold[f'{name}/{k}'] for k in ('scale', 'support_vectors', 'dual_coef', 'intercept', 'gamma', 'classes')}


def svm_of(env, m):
    return env.ens.PitchSVM.from_arrays(m['support_vectors'], m['dual_coef'], m['intercept'], m['gamma'], m['classes'],
                                        scale=m.get('scale'), center=m.get('center'))


@pytest.fixture(scope='module')
def fixture_rules(env, egold):
    """[(pair, threshold, PitchSVM)], [(pair, threshold, arrays)] of the two fitted models."""
    models = [model_of(egold, pair) for pair in PAIRS]
    return ([(pair, thr, svm_of(env, m)) for pair, thr, m in zip(PAIRS, THRESHOLDS, models)],
            [(pair, thr, m) for pair, thr, m in zip(PAIRS, THRESHOLDS, models)])


def random_model(seed, n_sv, F, classes=(0, 1), scale=True, center=True):
    rng = np.random.default_rng(seed)
    m = dict(support_vectors=rng.standard_normal((n_sv, F)), dual_coef=rng.uniform(-1, 1, n_sv), intercept=rng.uniform(-0.2, 0.2),
             gamma=0.5 / F, classes=np.array(classes))
    if scale:
        m['scale'] = rng.uniform(0.5, 2.0, F) * rng.choice([-1.0, 1.0], F)
    if center:
        m['center'] = rng.standard_normal(F)
    return m


def _guarded(env, nbytes):
    torch = env.torch
    total = (PAD + nbytes + PAD + 3) // 4 * 4
    buf = torch.empty(total // 4, dtype=torch.int32, device=env.dev)
    buf.fill_(int(SENT32))
    raw = buf.view(torch.uint8)

    def check(what):
        torch.cuda.synchronize(env.dev)
        host = raw.cpu().numpy()
        sent = np.full(total // 4, SENT32, dtype=np.int32).view(np.uint8)
        assert np.array_equal(host[:PAD], sent[:PAD]), f'{what}: bytes BEFORE the buffer were written'
        assert np.array_equal(host[PAD + nbytes:], sent[PAD + nbytes:]), f'{what}: bytes AFTER the buffer were written'
        return host[PAD:PAD + nbytes]
    return buf, buf.data_ptr() + PAD, check


def _dev(env, arr):
    return env.torch.from_numpy(np.ascontiguousarray(arr)).to(env.dev)


# ---- 1: the stand-alone SVM ----
def test_fixture_queries_against_sklearn(env, egold):
    for pair in PAIRS:
        name = f'svm{pair[0]}{pair[1]}'
        m = model_of(egold, pair)
        svm = svm_of(env, m)
        Q, want = egold[f'{name}/queries'], egold[f'{name}/decision']
        dec = svm.decision_function(Q)
        worst = float(np.max(np.abs(dec - want)))
        print(name, 'n_sv', svm.n_sv, 'max |device - sklearn|', worst, 'bound', ref.decision_bound(m))
        record('svm_decision_abs', worst)
        assert worst <= ref.decision_bound(m)
        assert np.array_equal(svm.predict(Q), egold[f'{name}/predict'])
        # a device tensor in gives device tensors out, the same bits
        d = svm.decision_function(_dev(env, Q))
        assert d.is_cuda and d.cpu().numpy().tobytes() == dec.tobytes()
        assert svm.predict(_dev(env, Q)).cpu().numpy().tolist() == egold[f'{name}/predict'].tolist()


@pytest.mark.parametrize('F', [1, 5, 16])
@pytest.mark.parametrize('n_sv', [1, 63, 64, 65, 257])
def test_models_and_row_counts_against_the_restatement(env, n_sv, F):
    torch = env.torch
    rng = np.random.default_rng(1000 * n_sv + F)
    for variant, (scale, center) in enumerate(((True, True), (False, False), (True, False))):
        m = random_model(n_sv * 100 + F * 3 + variant, n_sv, F, classes=(3, 11), scale=scale, center=center)
        svm = svm_of(env, m)
        bound = ref.decision_bound(m)
        for rows in (1, 3, 4, 5, 257):
            ld = F + (rows % 3)                                   # ld_feat == F and ld_feat > F
            X = rng.standard_normal((rows, ld))
            want = ref.decision(m, X)
            x = _dev(env, X)
            dec = torch.full((rows,), float('nan'), dtype=torch.float64, device=env.dev)
            lab = torch.full((rows,), -1, dtype=torch.int32, device=env.dev)
            env.nat.check(env.lib.dsp_svm_decision_batch(svm.handle(), x.data_ptr(), ld, rows, dec.data_ptr(), lab.data_ptr(), None))
            torch.cuda.synchronize(env.dev)
            got, labels = dec.cpu().numpy(), lab.cpu().numpy()
            worst = float(np.max(np.abs(got - want)))
            record('svm_decision_abs', worst)
            assert worst <= bound, (n_sv, F, rows, variant, worst, bound)
            assert np.array_equal(labels, np.where(got > 0, 11, 3))                  # the label is the sign of the decision written
            sure = np.abs(want) > bound
            assert np.array_equal(labels[sure], ref.predict(m, X)[sure])
            # either output alone
            only = torch.full((rows,), -1, dtype=torch.int32, device=env.dev)
            env.nat.check(env.lib.dsp_svm_decision_batch(svm.handle(), x.data_ptr(), ld, rows, None, only.data_ptr(), None))
            assert only.cpu().numpy().tolist() == labels.tolist()


# ---- 2: pre-emphasis and trim ----
def _trim(env, x, so, seg, coeff=0.97):
    """-> (rows per clip as the device wrote them, fp32), with sentinels around the output."""
    nat, torch = env.nat, env.torch
    seg = np.asarray(seg, dtype=np.int64).reshape(-1, 2)
    lens = seg[:, 1] - seg[:, 0]
    dst = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    d_x, d_so, d_seg, d_dst = _dev(env, x), _dev(env, so), _dev(env, seg), _dev(env, dst)      # (held until the check below)
    dtype = nat.WAVE_I16 if x.dtype == np.int16 else nat.WAVE_F32
    keep, p_out, check = _guarded(env, int(dst[-1]) * 4)
    nat.check(env.lib.dsp_trim_preemph_batch(d_x.data_ptr(), dtype, d_so.data_ptr(), d_seg.data_ptr(), d_dst.data_ptr(), len(seg),
                                             coeff, p_out, None))
    out = check('d_out').view(np.float32)
    assert not np.any(out.view(np.int32) == SENT32)                            # every element written
    return [out[dst[b]:dst[b + 1]] for b in range(len(seg))]


@pytest.mark.parametrize('kind', ['int16', 'float32'])
def test_trim_preemph_is_bitwise_numpy(env, kind):
    rng = np.random.default_rng(5)
    cases = [([1], [(0, 1)]),                                                   # a one-sample clip
             ([1000], [(3, 700)]),
             ([1, 300, 1000, 257, 2049], [(0, 1), (0, 300), (17, 17), (5, 257), (1000, 2000)])]   # l = 0, r = len, l = r
    for lens, seg in cases:
        so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        x = rng.integers(-20000, 20000, int(so[-1])).astype(np.int16)
        if kind == 'float32':
            x = (x + rng.uniform(-0.5, 0.5, len(x))).astype(np.float32)
        rows = _trim(env, x, so, seg)
        for b, (l, r) in enumerate(seg):
            want = np.float32(ref.preemph_trim(x[so[b]:so[b + 1]], l, r))
            assert rows[b].tobytes() == want.tobytes(), (kind, lens, b)
        if len(lens) > 1:
            assert rows[4][0] == np.float32(float(x[so[4] + 1000]) - 0.97 * float(x[so[4] + 999]))   # the sample in front of l


def test_trim_preemph_on_the_stored_clips(env, egold):
    clips, _ = make_clips()
    pick = [clips[b] for b in TRIM_CLIPS]
    so = np.concatenate([[0], np.cumsum([len(c) for c in pick])]).astype(np.int64)
    seg = [tuple(int(v) for v in egold['gate/endpoints'][b]) for b in TRIM_CLIPS]
    rows = _trim(env, np.concatenate(pick), so, seg)
    for k, b in enumerate(TRIM_CLIPS):
        assert rows[k].tobytes() == np.float32(egold[f'trim/{b}']).tobytes(), b


# ---- 3: the gate ----
def test_gate_on_the_stored_logits_and_reference_features(env, egold, fixture_rules):
    rules, rule_arrays = fixture_rules
    logits, feat = egold['gate/logits'], egold['gate/feat']
    pred, prob, used, dec = env.ens.ensemble_decide(_dev(env, logits), rules, _dev(env, feat))
    pred, prob, used, dec = (t.cpu().numpy() for t in (pred, prob, used, dec))
    assert pred.tolist() == egold['gate/final'].tolist()
    assert (used != 0).tolist() == egold['gate/replaced'].tolist() and used.min() >= 0
    want_pred, want_used, _ = ref.gate(logits, rule_arrays, feat)
    assert used.tolist() == want_used.tolist() and pred.tolist() == want_pred.tolist()
    e64 = float(np.max(np.abs(prob.astype(np.float64) - ref.softmax64(logits))))
    et = float(np.max(np.abs(prob.astype(np.float64) - egold['gate/prob'].astype(np.float64))))
    print('prob: max |device - fp64 softmax|', e64, ' max |device - torch.softmax|', et)
    record('ensemble_prob_abs_fp64', e64)
    record('ensemble_prob_abs_torch', et)
    assert e64 <= 2.0 ** -24 and et <= 1e-6
    # the decision of the gate is the stand-alone call's, bit for bit, and sklearn's within the bound
    for r, (pair, thr, svm) in enumerate(rules):
        alone = svm.decision_function(_dev(env, feat)).cpu().numpy()
        sel = used == r + 1
        assert sel.any() and dec[sel].tobytes() == alone[sel].tobytes()
        worst = float(np.max(np.abs(alone - egold['gate/decision'][:, r])))
        record('svm_decision_abs', worst)
        assert worst <= ref.decision_bound(rule_arrays[r][2])
    assert np.all(dec[used == 0] == 0.0)


def _gate_case(env, C, n_rules, B=257, seed=0):
    """Random logits at confidences around the thresholds, F = 5 features with stride 7, valid flags with stride 9."""
    rng = np.random.default_rng(seed + 10 * C + n_rules)
    if C == 2:
        pairs = [(0, 0), (1, 1)][:n_rules]
    else:
        pairs = [(0, 1), (6, 7), (C - 1, 3), (10, 12)][:n_rules]
    thresholds = [0.8, 0.7, 0.9, 0.6][:n_rules]
    arrays = [random_model(50 + r, (37, 64, 129, 200)[r], 5, classes=(pairs[r][1], pairs[r][0])) for r in range(n_rules)]
    logits = rng.standard_normal((B, C)) * 0.3
    top = rng.integers(0, C, B)
    if C > 2:
        top[: B // 2] = rng.choice([0, 1, 6, 7, C - 1, 3, 10, 12, 4, 5], B // 2)          # half the clips inside some pair
    conf = rng.uniform(0.35, 0.99, B) if C > 2 else rng.uniform(0.51, 0.99, B)
    logits[np.arange(B), top] = np.log((C - 1) * conf / (1 - conf))
    logits = logits.astype(np.float32)
    logits[5, :] = -1.0
    logits[5, [min(3, C - 1), min(7, C - 1)]] = 0.25                          # an exact tie: the lowest index wins
    logits[6, :] = 0.5                                                         # all equal: index 0, probability 1 / C
    feat = rng.standard_normal((B, 7))
    aux = np.ones((B, 9), dtype=np.int32)
    aux[::5, 8] = 0
    feat[::5, :5] = np.nan                                                     # what an invalid row holds
    return pairs, thresholds, arrays, logits, feat, aux


@pytest.mark.parametrize('C,n_rules', [(2, 0), (2, 2), (20, 0), (20, 4), (64, 0), (64, 4)])
def test_synthetic_gate_cases(env, C, n_rules):
    pairs, thresholds, arrays, logits, feat, aux = _gate_case(env, C, n_rules)
    B = len(logits)
    svms = [svm_of(env, m) for m in arrays]
    rules = list(zip(pairs, thresholds, svms))
    d_aux = _dev(env, aux)
    d_feat = _dev(env, feat)
    pred, prob, used, dec = env.ens.ensemble_decide(_dev(env, logits), rules, d_feat[:, :5] if n_rules else None,
                                                    d_aux[:, 8] if n_rules else None)
    pred, prob, used, dec = (t.cpu().numpy() for t in (pred, prob, used, dec))
    e64 = float(np.max(np.abs(prob.astype(np.float64) - ref.softmax64(logits))))
    record('ensemble_prob_abs_fp64', e64)
    assert e64 <= 2.0 ** -24
    rnn = np.argmax(logits, axis=1)
    assert rnn[5] == min(3, C - 1) and rnn[6] == 0
    # the gate of the restatement on the device's own fp32 probabilities (their values are checked above)
    want_pred, want_used, want_dec = ref.gate(logits, list(zip(pairs, thresholds, arrays)), feat[:, :5], valid=aux[:, 8], prob=prob)
    assert used.tolist() == want_used.tolist()
    if n_rules == 0:
        assert not used.any() and pred.tolist() == rnn.tolist() and not dec.any()
        return
    assert (used > 0).any() and (used < 0).any() and (used == 0).any()
    kept = used <= 0
    assert pred[kept].tolist() == rnn[kept].tolist()                          # no rule, or invalid features: the classifier's label
    covered = np.isin(rnn, [v for p in pairs for v in p])
    assert not used[~covered].any()                                           # labels outside every pair are untouched
    assert np.all(aux[used < 0, 8] == 0) and np.all(dec[used <= 0] == 0.0)
    for r in range(n_rules):
        sel = used == r + 1
        bound = ref.decision_bound(arrays[r])
        assert np.max(np.abs(dec[sel] - want_dec[sel]), initial=0.0) <= bound
        c0, c1 = arrays[r]['classes']
        assert pred[sel].tolist() == np.where(dec[sel] > 0, c1, c0).tolist()
        sure = sel & (np.abs(want_dec) > bound)
        assert pred[sure].tolist() == want_pred[sure].tolist()
        alone = svms[r].decision_function(d_feat[:, :5]).cpu().numpy()
        assert dec[sel].tobytes() == alone[sel].tobytes()                      # bit for bit the stand-alone call


# ---- 4: end to end ----
@pytest.fixture(scope='module')
def stored_batch(env, egold):
    clips, rate = make_clips()
    so = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    return np.concatenate(clips), so, rate


def test_ensemble_batch_on_the_stored_clips(env, egold, fixture_rules, stored_batch):
    rules, _ = fixture_rules
    flat, so, rate = stored_batch
    logits = _dev(env, egold['gate/logits'])
    seen = {}

    def head(inp, len0):
        seen['shape'], seen['len0'] = tuple(inp.shape), np.asarray(len0)
        return logits, None

    eb = env.ens.EnsembleBatch(rate, head, rules)
    for waves in (flat, _dev(env, flat)):                                     # host array and device tensor
        out = eb.run(waves, so)
        assert seen['shape'] == (200, len(so) - 1, 39) and (seen['len0'] > 0).all()
        assert np.array_equal(out.endpoints, egold['gate/endpoints'])
        assert out.pred.cpu().numpy().tolist() == egold['gate/final'].tolist()
        used = out.used.cpu().numpy()
        assert (used != 0).tolist() == egold['gate/replaced'].tolist() and used.min() >= 0
        assert out.valid.cpu().numpy().all()
        feat, want = out.feat.cpu().numpy(), egold['gate/feat']
        err = float(np.max(np.abs(feat - want) / np.maximum(1.0, np.abs(want))))
        print('pitch features: max |device - reference| / max(1, |reference|)', err)
        record('ensemble_pitch_feat_rel', err)
        assert np.all(np.abs(feat - want) <= 1e-9 * np.maximum(1.0, np.abs(want)))
        assert float(np.max(np.abs(out.prob.cpu().numpy().astype(np.float64) - egold['gate/prob']))) <= 1e-6


def test_ensemble_batch_with_a_seeded_hmrnn_head(env, egold, fixture_rules, stored_batch):
    torch = env.torch
    from features.classifier import HMRNNHead, fill_parameters
    rules, rule_arrays = fixture_rules
    flat, so, rate = stored_batch
    B = 5
    head = HMRNNHead().to(env.dev)
    fill_parameters(head, 3)
    # a third and a fourth rule, so that more of the 20 labels are gated (a seeded head is far from confident)
    extra = [((2, 3), 0.9, random_model(7, 40, 5, classes=(2, 3))), ((12, 13), 0.9, random_model(8, 90, 5, classes=(12, 13)))]
    arrays = list(rule_arrays) + extra
    all_rules = list(rules) + [(p, t, svm_of(env, m)) for p, t, m in extra]
    eb = env.ens.EnsembleBatch(rate, head, all_rules)
    with torch.no_grad():
        out = eb.run(flat[:so[B]], so[:B + 1], dropout=False)
    logits = out.logits.cpu().numpy()
    assert logits.shape == (B, 20) and np.isfinite(logits).all()
    want_pred, want_used, _ = ref.gate(logits, arrays, out.feat.cpu().numpy(), valid=out.valid.cpu().numpy())
    assert out.used.cpu().numpy().tolist() == want_used.tolist()
    assert out.pred.cpu().numpy().tolist() == want_pred.tolist()
    assert np.array_equal(out.endpoints, egold['gate/endpoints'][:B])


# ---- 5: buffers and capture ----
def test_outputs_stay_inside_their_buffers(env, egold, fixture_rules):
    rules, _ = fixture_rules
    nat, lib = env.nat, env.lib
    B, C = 5, 20
    logits = _dev(env, np.ascontiguousarray(egold['gate/logits'][[0, 1, 4, 10, 13]]))
    feat = _dev(env, np.ascontiguousarray(egold['gate/feat'][[0, 1, 4, 10, 13]]))
    arr, n = env.ens._as_rules(rules)
    k_pred, p_pred, c_pred = _guarded(env, B * 4)
    k_prob, p_prob, c_prob = _guarded(env, B * C * 4)
    k_used, p_used, c_used = _guarded(env, B * 4)
    k_dec, p_dec, c_dec = _guarded(env, B * 8)
    nat.check(lib.dsp_ensemble_decide_batch(logits.data_ptr(), C, B, C, arr, n, feat.data_ptr(), 5, None, 0, p_pred, p_prob, p_used,
                                            p_dec, None))
    assert c_pred('d_pred').view(np.int32).tolist() == egold['gate/final'][[0, 1, 4, 10, 13]].tolist()
    assert not np.any(c_prob('d_prob').view(np.int32) == SENT32)
    assert c_used('d_used').view(np.int32).tolist() == [1, 0, 2, 0, 2]
    assert np.isfinite(c_dec('d_decision').view(np.float64)).all()
    k_d, p_d, c_d = _guarded(env, B * 8)
    k_l, p_l, c_l = _guarded(env, B * 4)
    nat.check(lib.dsp_svm_decision_batch(rules[0][2].handle(), feat.data_ptr(), 5, B, p_d, p_l, None))
    assert np.isfinite(c_d('d_decision').view(np.float64)).all()
    assert set(c_l('d_label').view(np.int32).tolist()) <= {0, 1}
    # (dsp_trim_preemph_batch's output is fenced in every call of _trim above)


def test_three_calls_in_one_graph_replay_to_the_same_bytes(env, egold, fixture_rules):
    torch, nat, lib = env.torch, env.nat, env.lib
    rules, _ = fixture_rules
    arr, n_rules = env.ens._as_rules(rules)
    rng = np.random.default_rng(3)
    B, C = 6, 20
    lens = [900, 1200, 700, 1500, 1000, 800]
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seg = np.array([(0, 900), (100, 1100), (5, 5), (1, 1500), (300, 301), (0, 700)], dtype=np.int64)
    dst = np.concatenate([[0], np.cumsum(seg[:, 1] - seg[:, 0])]).astype(np.int64)
    x = _dev(env, rng.integers(-9000, 9000, int(so[-1])).astype(np.int16))
    d_so, d_seg, d_dst = _dev(env, so), _dev(env, seg), _dev(env, dst)
    logits = _dev(env, egold['gate/logits'][:B].copy())
    feat = _dev(env, egold['gate/feat'][:B].copy())
    trimmed = torch.zeros(int(dst[-1]), dtype=torch.float32, device=env.dev)
    alone = torch.zeros(B, dtype=torch.float64, device=env.dev)
    label = torch.zeros(B, dtype=torch.int32, device=env.dev)
    pred = torch.zeros(B, dtype=torch.int32, device=env.dev)
    used = torch.zeros(B, dtype=torch.int32, device=env.dev)
    prob = torch.zeros((B, C), dtype=torch.float32, device=env.dev)
    dec = torch.zeros(B, dtype=torch.float64, device=env.dev)
    handle = rules[0][2].handle()

    def enqueue(stream):
        st = stream.cuda_stream
        nat.check(lib.dsp_trim_preemph_batch(x.data_ptr(), nat.WAVE_I16, d_so.data_ptr(), d_seg.data_ptr(), d_dst.data_ptr(), B, 0.97,
                                             trimmed.data_ptr(), st))
        nat.check(lib.dsp_svm_decision_batch(handle, feat.data_ptr(), 5, B, alone.data_ptr(), label.data_ptr(), st))
        nat.check(lib.dsp_ensemble_decide_batch(logits.data_ptr(), C, B, C, arr, n_rules, feat.data_ptr(), 5, None, 0, pred.data_ptr(),
                                                prob.data_ptr(), used.data_ptr(), dec.data_ptr(), st))

    def snapshot():
        torch.cuda.synchronize(env.dev)
        return tuple(t.cpu().numpy().tobytes() for t in (trimmed, alone, label, pred, used, prob, dec))

    side = torch.cuda.Stream(env.dev)
    side.wait_stream(torch.cuda.current_stream(env.dev))
    with torch.cuda.stream(side):
        enqueue(side)
    side.synchronize()
    first = snapshot()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream(env.dev))
    # new data in the same buffers
    x.copy_(_dev(env, rng.integers(-9000, 9000, int(so[-1])).astype(np.int16)))
    logits.copy_(_dev(env, egold['gate/logits'][B:2 * B].copy()))
    feat.copy_(_dev(env, egold['gate/feat'][B:2 * B].copy()))
    torch.cuda.synchronize(env.dev)
    graph.replay()
    replayed = snapshot()
    with torch.cuda.stream(side):
        enqueue(side)
    eager = snapshot()
    assert replayed == eager
    assert all(replayed[k] != first[k] for k in (0, 1, 3, 4, 5, 6))            # the replay did see the new inputs
    assert np.frombuffer(replayed[3], dtype=np.int32).tolist() == egold['gate/final'][B:2 * B].tolist()
