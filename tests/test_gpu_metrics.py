"""The loss / metrics kernels on the device (csrc/kernels_loss.h: dsp_xent_metrics_batch, dsp_metrics_reset;
features/metrics.py) and the keywords that put them behind the training loss and the ensemble gate.

Cases: tests/metrics_cases.py.  The reference is tools/metrics_emul.py (fp64 / int64 NumPy; tests/test_metrics_host.py holds it to
torch on the CPU).  Bars:
  * ``d_prob`` / ``d_pred``: ``==`` against ``ensemble_decide(logits, [])`` (one device function serves both kernels);
  * every integer of the state: ``==`` against the emulation;
  * ``loss`` / ``nll``: within 2^-23 max(1, |ref|) -- one fp32 rounding (2^-24) of an fp64 value, with a factor 2 over it;
  * ``dlogits``: within 2^-23 |ref| + 1e-12, exact zeros in ignored rows;  ``loss_sum``: 1e-12 relative;
  * the same bits on two runs, canaries intact (behind every row of the strided logits / dlogits and behind every output);
  * heads: ``loss='native'`` against ``loss='torch'``: loss within 2e-6, every gradient within 2e-5 max(1, max |ref|)
    (tests/test_gpu_device_train.py's bar between two fp32 routes);
  * recorded: three replays equal three eager steps in every bit (loss, parameters, moments, metrics integers, loss_sum)."""
import copy
import os
import random
import sys

import numpy as np
import pytest

import metrics_cases as mc
from conftest import ROOT, record
from ensemble_cases import PAIRS, THRESHOLDS, make_clips

sys.path.insert(0, os.path.join(ROOT, 'tools'))

import metrics_emul as me  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
BAR = 2e-5
GUARD = 16
CAN_BITS = 0x7fc0beef
INTS = ('seen', 'scored', 'correct', 'ignored', 'bad_label', 'wrong_total', 'calls')


@pytest.fixture(scope='module')
def env():
    import types
    import torch
    from features import _native as nat
    from features import metrics
    nat.require_device()
    return types.SimpleNamespace(nat=nat, lib=nat.load(), torch=torch, dev=torch.device('cuda', 0), M=metrics)


def _canaries(env, n, dtype):
    a = np.full(n, CAN_BITS, dtype=np.uint32).view(np.float32 if dtype == 'f' else np.int32)
    return env.torch.from_numpy(a.copy()).to(env.dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _call(env, case, C, pred_in=False, grad_out=None, metrics=None):
    """One raw call with a row stride of C + PAD on logits and dlogits and GUARD canary words behind every output ->
    host arrays (bit views where a canary may sit) + the guard check."""
    torch = env.torch
    B, LD = len(case.labels), C + mc.PAD
    lg = torch.from_numpy(mc.strided(case.logits)).to(env.dev)
    lab = torch.from_numpy(case.labels).to(env.dev)
    pin = torch.from_numpy(case.pred_in).to(env.dev) if pred_in else None
    go = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device=env.dev)
    nll, loss, prob = _canaries(env, B + GUARD, 'f'), _canaries(env, 1 + GUARD, 'f'), _canaries(env, B * C + GUARD, 'f')
    pred, dl = _canaries(env, B + GUARD, 'i'), _canaries(env, B * LD + GUARD, 'f')
    rc = env.lib.dsp_xent_metrics_batch(lg.data_ptr(), LD, B, C, lab.data_ptr(), None if pin is None else pin.data_ptr(),
                                        None if go is None else go.data_ptr(), nll.data_ptr(), loss.data_ptr(), pred.data_ptr(),
                                        prob.data_ptr(), dl.data_ptr(), LD, None if metrics is None else metrics.state.data_ptr(),
                                        0 if metrics is None else metrics.wrong_capacity, torch.cuda.current_stream(env.dev).cuda_stream)
    env.nat.check(rc)
    torch.cuda.synchronize(env.dev)
    # canaries: behind every output, between the rows of dlogits, and the logits' padding untouched
    for name, t, n in (('nll', nll, B), ('loss', loss, 1), ('prob', prob, B * C), ('pred', pred, B), ('dlogits', dl, B * LD)):
        assert (_bits(t)[n:] == np.int32(CAN_BITS)).all(), f'{name}: a word behind the output was written'
    dl2 = _bits(dl)[:B * LD].reshape(B, LD)
    assert (dl2[:, C:] == np.int32(CAN_BITS)).all(), 'dlogits: a word between the rows was written'
    assert np.array_equal(_bits(lg), mc.strided(case.logits).view(np.int32)), 'the logits were written'
    import types
    return types.SimpleNamespace(nll=nll.cpu().numpy()[:B], loss=loss.cpu().numpy()[0], prob=prob.cpu().numpy()[:B * C].reshape(B, C),
                                 pred=pred.cpu().numpy()[:B], dlogits=dl.cpu().numpy()[:B * LD].reshape(B, LD)[:, :C].copy(),
                                 lg=lg, raw=[_bits(t).copy() for t in (nll, loss, prob, pred, dl)])


def _check_values(tag, got, ref):
    """The bars of the module docstring on one call's outputs; records the measured worst cases."""
    scale = max(1.0, abs(float(ref.loss))) if np.isfinite(ref.loss) else 1.0
    if np.isnan(ref.loss):
        assert np.isnan(got.loss)
    else:
        e = record('xent_loss_vs_fp64_ulps_of_bar', abs(float(got.loss) - float(ref.loss)) / (EPS * scale))
        print(f'{tag}: loss {float(got.loss):.9g} against {float(ref.loss):.12g}: {e:.3f} of the bar')
        assert e <= 1.0
    e = record('xent_nll_vs_fp64_ulps_of_bar', float(np.max(np.abs(got.nll.astype(np.float64) - ref.nll) / (EPS * np.maximum(1.0, np.abs(ref.nll))))))
    print(f'{tag}: nll worst {e:.3f} of the bar')
    assert e <= 1.0
    assert not got.nll[~ref.scored].any()
    err = np.abs(got.dlogits.astype(np.float64) - ref.dlogits)
    bound = EPS * np.abs(ref.dlogits) + 1e-12
    e = record('xent_dlogits_vs_fp64_of_bar', float(np.max(err / bound)))
    print(f'{tag}: dlogits worst {e:.3f} of the bar')
    assert e <= 1.0
    assert not got.dlogits[~ref.scored].view(np.int32).any()              # exact +0.0 in ignored rows


def _check_state(r, want):
    for name in INTS:
        assert getattr(r, name) == getattr(want, name), (name, getattr(r, name), getattr(want, name))
    assert np.array_equal(r.confusion, want.confusion) and np.array_equal(r.wrong, want.wrong)
    assert abs(r.loss_sum - want.loss_sum) <= 1e-12 * max(abs(want.loss_sum), 1e-300), (r.loss_sum, want.loss_sum)
    record('xent_loss_sum_rel_vs_fp64', abs(r.loss_sum - want.loss_sum) / max(abs(want.loss_sum), 1e-300))


# ---- the kernels ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,C', mc.SHAPES)
@pytest.mark.parametrize('pred_in', [False, True])
def test_kernels_against_the_restatement(env, B, C, pred_in):
    from features.ensemble import ensemble_decide
    case = mc.make(B, C)
    m = env.M.Metrics(C, 2 * B)
    got = _call(env, case, C, pred_in=pred_in, grad_out=None, metrics=m)
    x64 = case.logits.astype(np.float64)
    ref = me.xent(x64, case.labels, case.pred_in if pred_in else None)
    _check_values(f'B={B} C={C}', got, ref)
    # prob / pred: the gate's, in every bit, from the same strided view
    pred_g, prob_g, _, _ = ensemble_decide(got.lg[:, :C], [])
    assert np.array_equal(got.pred, pred_g.cpu().numpy()) and np.array_equal(got.pred, ref.pred.astype(np.int32))
    assert np.array_equal(got.prob.view(np.int32), prob_g.cpu().numpy().view(np.int32))
    st = me.State(C, 2 * B)
    st.update(x64, case.labels, case.pred_in if pred_in else None)
    _check_state(m.result(), st.result())
    # the same bits on a second run (and the state moved a second time, by the same integers)
    again = _call(env, case, C, pred_in=pred_in, grad_out=None, metrics=m)
    for a, b in zip(got.raw, again.raw):
        assert np.array_equal(a, b)
    st.update(x64, case.labels, case.pred_in if pred_in else None)
    _check_state(m.result(), st.result())


@pytest.mark.parametrize('B,C', [(5, 20), (67, 20)])
def test_upstream_gradient_scales_dlogits(env, B, C):
    case = mc.make(B, C)
    got = _call(env, case, C, grad_out=2.5)
    _check_values(f'B={B} grad_out=2.5', got, me.xent(case.logits.astype(np.float64), case.labels, grad_out=2.5))


@pytest.mark.parametrize('B,C', [s for s in mc.SHAPES if s[0] > 1])
def test_two_updates_of_halves_equal_one_of_the_whole(env, B, C):
    torch = env.torch
    case = mc.make(B, C)
    lg, lab, pin = (torch.from_numpy(a).to(env.dev) for a in (case.logits, case.labels, case.pred_in))
    whole, halves = env.M.Metrics(C, 7), env.M.Metrics(C, 7)
    whole.update(lg, lab, pin)
    h = B // 2
    halves.update(lg[:h], lab[:h], pin[:h])
    halves.update(lg[h:], lab[h:], pin[h:])
    a, b = whole.result(), halves.result()
    for name in INTS[:-1]:
        assert getattr(a, name) == getattr(b, name), name
    assert (a.calls, b.calls) == (1, 2)
    assert np.array_equal(a.confusion, b.confusion) and np.array_equal(a.wrong, b.wrong)
    assert abs(a.loss_sum - b.loss_sum) <= 1e-12 * abs(a.loss_sum)
    st = me.State(C, 7)
    st.update(case.logits.astype(np.float64), case.labels, case.pred_in)
    _check_state(a, st.result())


def test_wrong_capacity_reset_and_the_all_ignored_batch(env):
    torch = env.torch
    C = 20
    logits = np.zeros((6, C), dtype=np.float32)
    logits[np.arange(6), [1, 2, 3, 4, 5, 6]] = 1.0
    labels = np.array([0, 2, 0, 0, 0, 0], dtype=np.int64)               # clip 1 is right, the five others wrong
    m = env.M.Metrics(C, 2)
    lg, lab = torch.from_numpy(logits).to(env.dev), torch.from_numpy(labels).to(env.dev)
    m.update(lg[:3], lab[:3])
    m.update(lg[3:], lab[3:])
    r = m.result()
    assert r.wrong_total == 5 and r.wrong.tolist() == [[0, 1, 0], [2, 3, 0]] and (r.seen, r.scored, r.correct) == (6, 6, 1)
    assert r.accuracy == 1 / 6 and r.confusion[0, 1] == 1 and r.confusion[2, 2] == 1 and r.confusion.sum() == 6
    assert r.confusion_present().shape == (7, 7)                           # labels 0 .. 6 occur
    m.reset()
    torch.cuda.synchronize(env.dev)
    assert not m.state.cpu().numpy().any()
    # every label ignored: NaN, zeros, and only seen / ignored / bad_label moved
    case = mc.make(5, C)
    case.labels = np.array([mc.IGNORE, 23, mc.IGNORE, -1, mc.IGNORE], dtype=np.int64)
    got = _call(env, case, C, metrics=m)
    assert np.isnan(got.loss) and not got.dlogits.view(np.int32).any() and not got.nll.view(np.int32).any()
    r = m.result()
    assert (r.seen, r.scored, r.correct, r.ignored, r.bad_label, r.wrong_total, r.calls) == (5, 0, 0, 5, 2, 0, 1)
    assert r.loss_sum == 0.0 and not r.confusion.any() and len(r.wrong) == 0 and np.isnan(r.accuracy)


# ---- autograd -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,C', [(32, 20), (67, 20)])
@pytest.mark.parametrize('scale', [None, 2.5])
def test_cross_entropy_autograd(env, B, C, scale):
    torch = env.torch
    import torch.nn.functional as F
    case = mc.make(B, C)
    x = torch.from_numpy(case.logits).to(env.dev).requires_grad_(True)
    lab = torch.from_numpy(case.labels).to(env.dev)
    loss = env.M.cross_entropy(x, lab)
    assert loss.dim() == 0 and loss.requires_grad and loss.dtype == torch.float32
    (loss if scale is None else scale * loss).backward()
    x64 = torch.from_numpy(case.logits).double().requires_grad_(True)
    y = torch.from_numpy(np.where((case.labels >= 0) & (case.labels < C), case.labels, mc.IGNORE))
    ref = F.cross_entropy(x64, y)
    (ref if scale is None else scale * ref).backward()
    refv = float(ref.detach())
    assert abs(float(loss.detach()) - refv) <= EPS * max(1.0, abs(refv))
    g, g64 = x.grad.cpu().numpy().astype(np.float64), x64.grad.numpy()
    # (a non-unit upstream gradient goes through one fp32 multiply behind the rounded dlogits: two roundings of at most
    # 2^-24 / (1 + 2^-24) each stay inside 2^-23)
    bound = EPS * np.abs(g64) + 1e-12
    e = record('xent_autograd_grad_of_bar', float(np.max(np.abs(g - g64) / bound)))
    assert e <= 1.0
    # the unit gradient of ``backward`` hands the stored gradient on: the same bits as ``loss.backward()``
    x2 = torch.from_numpy(case.logits).to(env.dev).requires_grad_(True)
    env.M.backward(env.M.cross_entropy(x2, lab))
    if scale is None:
        assert torch.equal(x2.grad.view(torch.int32), x.grad.view(torch.int32))
    with pytest.raises(TypeError, match='float32'):
        env.M.cross_entropy(x.detach().double(), lab)


# ---- the heads ------------------------------------------------------------------------------------------------------------------

def _head(kind, dev):
    import torch
    from features import classifier as C
    torch.manual_seed(0)
    head = getattr(C, kind)().train()
    C.fill_parameters(head, 3)
    for m in head.modules():
        if isinstance(m, C._DynEnc):
            m.gru.dropout = 0.0
    return head.to(dev)


def _cut(stored, B, k):
    """Batch k of B clips: prefixes of the stored clips in an order and at lengths that change with k."""
    out = []
    for i in range(B):
        c = stored[(i + 3 * k) % len(stored)]
        frac = (0.60 + 0.05 * ((3 * i) % 5)) if k == 0 else (0.55 + 0.05 * ((7 * i + 3 * k) % 5))
        out.append(c[:int(frac * len(c)) + 7 * i + k])
    return out


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


def _kw(kind):
    return {} if kind == 'RNNHead' else {'dropout': False}


@pytest.mark.parametrize('kind,B', [('RNNHead', 32), ('HRNNHead', 32), ('HRNNAttHead', 32), ('TransformerHead', 32), ('HMRNNHead', 32),
                                    ('HMRNNHead', 5)])
def test_native_loss_against_torch_loss_on_the_heads(env, kind, B):
    torch = env.torch
    from features.train import TrainBatch
    stored, rate = make_clips()
    clips = _cut(stored, B, 0)
    flat, so = np.concatenate(clips), _offsets(clips)
    head = _head(kind, env.dev)
    tb = TrainBatch(rate, head)
    labels = np.random.default_rng(B).integers(0, 20, B).astype(np.int64)
    jitter = tb.draw_jitter(B, random.Random(B))
    params = list(head.parameters())
    res = {}
    m = env.M.Metrics(20, 64)
    for route in ('torch', 'native'):
        head.zero_grad(set_to_none=True)
        extra = dict(loss='native', metrics=m) if route == 'native' else {}
        out = tb.run(flat, so, labels, jitter, **extra, **_kw(kind))
        out.loss.backward()
        res[route] = (float(out.loss.detach()), [p.grad.detach().cpu().numpy().astype(np.float64) for p in params], out.logits.detach().cpu().numpy())
    e = record(f'native_loss_vs_torch_{kind}_{B}', abs(res['native'][0] - res['torch'][0]))
    worst = 0.0
    for (name, _), a, b in zip(head.named_parameters(), res['native'][1], res['torch'][1]):
        ge = float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))
        worst = max(worst, ge)
        assert ge <= BAR, (kind, name, ge)
    record(f'native_loss_grads_vs_torch_{kind}_{B}', worst)
    print(f'{kind} B={B}: loss {res["native"][0]:.9g} against {res["torch"][0]:.9g} (|d| = {e:.3g}), worst gradient {worst:.3g}')
    assert e <= 2e-6
    r = m.result()
    st = me.State(20, 64)
    st.update(res['native'][2].astype(np.float64), labels)
    _check_state(r, st.result())
    with pytest.raises(ValueError, match="needs loss='native'"):
        tb.run(flat, so, labels, jitter, metrics=m, **_kw(kind))


def _same_bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


@pytest.mark.parametrize('kind,B', [('HMRNNHead', 5), ('TransformerHead', 32)])
def test_three_replays_with_native_loss_and_metrics_equal_three_eager_steps(env, kind, B):
    torch = env.torch
    from features.optim import DeviceAdam
    from features.train import CAPTURE_VERIFIED, TrainBatch
    assert B in CAPTURE_VERIFIED[kind]
    stored, rate = make_clips()
    head = _head(kind, env.dev)
    twin = copy.deepcopy(head)
    tb, tb_twin = TrainBatch(rate, head), TrainBatch(rate, twin)
    batches = [_cut(stored, B, k) for k in range(3)]
    cap = (5 * max(sum(len(c) for c in b) for b in batches)) // 4
    rng = np.random.default_rng(B)
    content = []
    for k, clips in enumerate(batches):
        labels = rng.integers(0, 20, B).astype(np.int64)
        labels[k % B] = mc.IGNORE                                          # an ignored clip in every batch
        content.append((np.concatenate(clips), _offsets(clips), labels, tb.draw_jitter(B, random.Random(B + k))))
    opt = DeviceAdam(list(head.parameters()), lr=1e-3)
    m, m_twin = env.M.Metrics(20, 8), env.M.Metrics(20, 8)
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    flat, so0, l0, j0 = content[0]
    buf[:len(flat)].copy_(torch.from_numpy(flat))
    lab, jit = torch.from_numpy(l0).to(env.dev), torch.from_numpy(j0).to(env.dev)
    g = tb.capture(buf, so0, lab, jit, optimizer=opt, capacity=cap, loss='native', metrics=m, **_kw(kind))
    torch.cuda.synchronize(env.dev)
    assert not m.state.cpu().numpy().any() and opt.device_state()[0] == 0      # capture left both as it found them
    losses = []
    for flat, so, l, j in content:
        buf.fill_(12345)
        buf[:len(flat)].copy_(torch.from_numpy(flat))
        g.sample_offsets.copy_(torch.from_numpy(so))
        lab.copy_(torch.from_numpy(l))
        jit.copy_(torch.from_numpy(j))
        losses.append(g.replay().loss.clone())
    torch.cuda.synchronize(env.dev)
    assert int(g.status.cpu()[0]) == 0
    opt_twin = DeviceAdam(list(twin.parameters()), lr=1e-3)
    want = []
    for flat, so, l, j in content:
        for p in opt_twin.params:
            p.grad = None
        out = tb_twin.run(torch.from_numpy(flat).to(env.dev), so, torch.from_numpy(l).to(env.dev), torch.from_numpy(j).to(env.dev),
                          loss='native', metrics=m_twin, **_kw(kind))
        out.loss.backward()
        opt_twin.step()
        want.append(out.loss.detach().clone())
    torch.cuda.synchronize(env.dev)
    differing = [k for k in range(3) if not _same_bits(losses[k], want[k])]
    print(f'{kind} B={B}: losses {[float(x) for x in losses]}, differing from the eager steps in bits: {differing}')
    assert not differing
    names = [n for n, _ in head.named_parameters()]
    bad = [n for n, p, q in zip(names, head.parameters(), twin.parameters()) if not _same_bits(p, q)]
    bad += [n + '.exp_avg' for n, p, q in zip(names, opt.exp_avg, opt_twin.exp_avg) if not _same_bits(p, q)]
    bad += [n + '.exp_avg_sq' for n, p, q in zip(names, opt.exp_avg_sq, opt_twin.exp_avg_sq) if not _same_bits(p, q)]
    assert not bad, bad
    assert opt.device_state() == opt_twin.device_state() and opt.device_state()[0] == 3
    a, b = m.result(), m_twin.result()
    for name in INTS:
        assert getattr(a, name) == getattr(b, name), name
    assert (a.seen, a.ignored, a.calls) == (3 * B, 3, 3)
    assert np.array_equal(a.confusion, b.confusion) and np.array_equal(a.wrong, b.wrong) and a.loss_sum == b.loss_sum


# ---- scoring behind the gate ----------------------------------------------------------------------------------------------------

def _numpy_metrics(C, cap, calls):
    """The metrics from downloaded (logits, pred, labels) triples, call after call."""
    st = me.State(C, cap)
    for logits, pred, labels in calls:
        st.update(logits.astype(np.float64), labels, pred)
    return st.result()


def _compare_scoring(r, want):
    for name in INTS:
        assert getattr(r, name) == getattr(want, name), name
    assert np.array_equal(r.confusion, want.confusion) and np.array_equal(r.wrong, want.wrong)
    assert abs(r.loss - want.loss) <= 1e-6, (r.loss, want.loss)
    record('ensemble_metrics_loss_vs_numpy', abs(r.loss - want.loss))


@pytest.fixture(scope='module')
def ens(env):
    """The 14 committed ensemble clips, an eval-mode head, the reference's two rules from the golden file and one rule built so
    that the gate RE-LABELS clips: the pair (a, b) with a the classifier's label of clip 0, a threshold no probability reaches
    and an SVM that always answers b."""
    import types
    from features import ensemble
    from features.classifier import HMRNNHead, fill_parameters
    torch = env.torch
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ensemble_golden.npz')) as z:
        models = [{k: z[f'svm{p[0]}{p[1]}/{k}'] for k in ('scale', 'support_vectors', 'dual_coef', 'intercept', 'gamma', 'classes')}
                  for p in PAIRS]
    rules = [(p, t, ensemble.PitchSVM.from_arrays(m['support_vectors'], m['dual_coef'], m['intercept'], m['gamma'], m['classes'],
                                                  scale=m['scale'])) for p, t, m in zip(PAIRS, THRESHOLDS, models)]
    head = HMRNNHead().to(env.dev).eval()
    fill_parameters(head, 3)
    clips, rate = make_clips()
    flat, so = np.concatenate(clips), _offsets(clips)
    with torch.no_grad():
        plain = ensemble.EnsembleBatch(rate, head, []).run(flat, so, sync_free=True, dropout=False)
    arg = plain.pred.cpu().numpy()
    taken = {v for p in PAIRS for v in p}
    free = [int(v) for v in arg if int(v) not in taken]
    if free:                                               # (otherwise the golden rules alone must re-label: the test asserts it)
        a = free[0]
        b = next(v for v in range(20) if v != a and v not in taken)
        rules.append(((a, b), 1.5, ensemble.PitchSVM.from_arrays(np.zeros((1, 5)), np.array([1e-9]), 10.0, 0.1, (a, b))))
    return types.SimpleNamespace(ens=ensemble, rules=rules, head=head, clips=clips, rate=rate, flat=flat, so=so, argmax=arg)


def test_ensemble_scoring_sync_free_and_recorded(env, ens):
    torch = env.torch
    B = len(ens.clips)
    assert B == 14
    eb = ens.ens.EnsembleBatch(ens.rate, ens.head, ens.rules)
    labels = ens.argmax.astype(np.int64).copy()
    labels[1::4] = (labels[1::4] + 1) % 20                                 # some wrong, one ignored
    labels[5] = mc.IGNORE
    lab = torch.from_numpy(labels).to(env.dev)
    m = env.M.Metrics(20, 32)
    with torch.no_grad():
        out = eb.run(ens.flat, ens.so, sync_free=True, labels=lab, metrics=m, dropout=False)
    pred, logits = out.pred.cpu().numpy(), out.logits.cpu().numpy()
    assert (pred != logits.argmax(axis=1)).any(), 'no clip was re-labelled by the gate: the fixture does not cover pred != argmax'
    print(f'gate re-labelled {int((pred != logits.argmax(axis=1)).sum())} of {B} clips')
    _compare_scoring(m.result(), _numpy_metrics(20, 32, [(logits, pred, labels)]))
    with pytest.raises(ValueError, match='downloading run'):
        eb.run(ens.flat, ens.so, labels=lab, metrics=m, dropout=False)
    # recorded on a capacity layout, replayed on two length vectors
    batches = [_cut(ens.clips, B, k) for k in (1, 2)]
    cap = (5 * max(sum(len(c) for c in b) for b in batches)) // 4
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    flat0 = np.concatenate(batches[0])
    buf[:len(flat0)].copy_(torch.from_numpy(flat0))
    m.reset()
    g = eb.capture(buf, _offsets(batches[0]), capacity=cap, labels=lab, metrics=m, dropout=False)
    torch.cuda.synchronize(env.dev)
    assert not m.state.cpu().numpy().any()                                 # capture left the block as it found it
    calls = []
    for k, clips in enumerate(batches):
        flat = np.concatenate(clips)
        buf.fill_(12345)
        buf[:len(flat)].copy_(torch.from_numpy(flat))
        g.sample_offsets.copy_(torch.from_numpy(_offsets(clips)))
        lab_k = np.roll(labels, k)
        lab.copy_(torch.from_numpy(lab_k))
        res = g.replay()
        torch.cuda.synchronize(env.dev)
        assert int(g.status.cpu()[0]) == 0
        calls.append((res.logits.cpu().numpy().copy(), res.pred.cpu().numpy().copy(), lab_k))
    _compare_scoring(m.result(), _numpy_metrics(20, 32, calls))


def test_mixed_rate_ensemble_scoring(env, ens):
    torch = env.torch
    from golden_cases import make_signal
    rates = [44100, 48000, 44100, 48000, 48000, 44100]
    clips = [make_signal(('vad', 700 + i, int(s * r) + 37 * i + 1, r, 0.6)) for i, (s, r) in enumerate(zip([0.9, 1.0, 1.1, 1.2, 1.3, 1.4], rates))]
    flat, so = torch.from_numpy(np.concatenate(clips)).to(env.dev), _offsets(clips)
    mb = ens.ens.MixedRateEnsembleBatch(ens.head, ens.rules)
    labels = np.array([3, 0, mc.IGNORE, 7, 1, 12], dtype=np.int64)
    lab = torch.from_numpy(labels).to(env.dev)
    m = env.M.Metrics(20, 8)
    with torch.no_grad():
        out = mb.run(flat, so, rates, sync_free=True, labels=lab, metrics=m, dropout=False)
    _compare_scoring(m.result(), _numpy_metrics(20, 8, [(out.logits.cpu().numpy(), out.pred.cpu().numpy(), labels)]))
