"""The speaker discriminator of the adversarial head on the device (csrc/kernels_adv.h: dsp_adv_disc_forward,
dsp_adv_disc_train; features/adversarial.py; features/train.py: AdvTrainBatch).

Kernel.  The reference is fp64 torch autograd on the CPU over the restated chain of adv_clf.py:34-38 under ``F.cross_entropy``:
``loss2, logits2, dfeat, dW1, db1, dW2, db2``.  Bars:
  * every tensor: max |got - ref| / max |ref| <= 2e-5, the project's bar for a native fp32 block, measured as
    tests/test_gpu_attn_train.py measures the attention gradients -- relative to the tensor's OWN largest value, so gamma = 0.01
    cannot hide an error in ``dfeat``;
  * ``loss2``: the loss call's bar (tests/test_gpu_metrics.py), 2^-23 max(1, |ref|), against the fp64 cross-entropy of the
    logits the kernel itself produced (the loss kernels' contract is over their inputs), and 2e-5 max(1, |ref|) against the
    fp64 chain (the logits are fp32 sums of up to 2048 products);
  * torch's fp32 error on the same device is printed and recorded beside every native figure;
  * two runs, a run with gamma in device memory, and a run on 4-byte-aligned views give the same bits; NULL outputs leave the
    other outputs' bits unchanged; canaries behind every output and between the rows of every strided tensor stay intact.
Head.  ``native_disc=True`` against ``native_disc=False``: every parameter gradient within 2e-5 of the tensor's largest value.
Capture.  Three replays equal three eager steps in every bit of both losses, every parameter, every Adam moment and both metrics
blocks, with ``set_lr`` and a new gamma in device memory before the third."""
import copy
import random
import types

import numpy as np
import pytest

from conftest import record
from ensemble_cases import make_clips

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
BAR = 2e-5
GUARD = 16
CAN_BITS = 0x7fc0beef
SHAPES = [(1, 7, 5, 2), (5, 400, 200, 35), (17, 400, 200, 35), (33, 64, 16, 64), (512, 400, 200, 35)]
OUTS = ('logits2', 'dfeat', 'dW1', 'db1', 'dW2', 'db2')
IGNORE = -100


@pytest.fixture(scope='module')
def env():
    import torch
    from features import _native as nat
    from features import adversarial, metrics
    nat.require_device()
    return types.SimpleNamespace(nat=nat, lib=nat.load(), torch=torch, dev=torch.device('cuda', 0), M=metrics, A=adversarial)


def _case(B, F, H, S, seed=0):
    rng = np.random.default_rng(1000 * seed + B + F + H + S)
    u = lambda *shape: rng.uniform(-0.08, 0.08, shape).astype(np.float32)
    return types.SimpleNamespace(B=B, F=F, H=H, S=S, feat=rng.uniform(-1.0, 1.0, (B, F)).astype(np.float32), W1=u(H, F), b1=u(H),
                                 W2=u(S, H), b2=u(S), speakers=rng.integers(0, S, B).astype(np.int64))


_REF = {}


def _chain(torch, A, c, gamma, dtype, dev, grad_out=1.0):
    """The restated chain with autograd in ``dtype`` on ``dev`` -> the seven tensors as fp64 host arrays."""
    t = lambda a: torch.from_numpy(a).to(device=dev, dtype=dtype).requires_grad_(True)
    feat, W1, b1, W2, b2 = (t(a) for a in (c.feat, c.W1, c.b1, c.W2, c.b2))
    spk = c.speakers.copy()
    spk[(spk < 0) | (spk >= c.S)] = IGNORE                                  # the library ignores every label outside [0, S)
    z = torch.tanh(A.gradient_reverse(feat, gamma) @ W1.T + b1) @ W2.T + b2
    loss = torch.nn.functional.cross_entropy(z, torch.from_numpy(spk).to(dev))
    (loss * grad_out).backward()
    h = lambda x: x.detach().cpu().numpy().astype(np.float64)
    return types.SimpleNamespace(loss2=h(loss), logits2=h(z), dfeat=h(feat.grad), dW1=h(W1.grad), db1=h(b1.grad), dW2=h(W2.grad),
                                 db2=h(b2.grad))


def _reference(env, c, gamma, key):
    """fp64 on the CPU, computed once per case and left unchanged."""
    if key not in _REF:
        _REF[key] = _chain(env.torch, env.A, c, gamma, env.torch.float64, env.torch.device('cpu'))
    return _REF[key]


def _canaries(env, n):
    a = np.full(n, CAN_BITS, dtype=np.uint32).view(np.float32)
    return env.torch.from_numpy(a.copy()).to(env.dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _strided(env, a, ld, offset=0):
    """A host [rows, cols] array as a device buffer of canaries with row stride ``ld``, ``offset`` floats in -> (buffer, view)."""
    rows, cols = a.shape
    buf = _canaries(env, offset + rows * ld + GUARD)
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(env.torch.from_numpy(a))
    return buf, view


def _call(env, c, gamma=0.01, device_gamma=False, pad=0, nulls=(), grad_out=None, metrics=None, offset=0):
    """One raw ``dsp_adv_disc_train`` with GUARD canary words behind every output, row strides of cols + pad on feat, logits2 and
    dfeat and ``offset`` floats in front of feat / W1 / W2 -> bit views of every output, after the guard checks."""
    torch = env.torch
    B, F, H, S = c.B, c.F, c.H, c.S
    fbuf, feat = _strided(env, c.feat, F + pad, offset)
    w1buf, W1 = _strided(env, c.W1, F, offset)
    w2buf, W2 = _strided(env, c.W2, H, offset)
    b1, b2 = torch.from_numpy(c.b1).to(env.dev), torch.from_numpy(c.b2).to(env.dev)
    spk = torch.from_numpy(c.speakers).to(env.dev)
    go = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device=env.dev)
    dg = torch.tensor([gamma], dtype=torch.float32, device=env.dev) if device_gamma else None
    sizes = dict(a=(B, H, H), logits2=(B, S, S + pad), loss2=(1, 1, 1), dz=(B, S, S), dfeat=(B, F, F + pad), dW1=(H, F, F), db1=(1, H, H),
                 dW2=(S, H, H), db2=(1, S, S))
    bufs = {k: _canaries(env, r * ld + GUARD) for k, (r, _, ld) in sizes.items()}
    out = env.nat.c_i64(0)
    env.nat.check(env.lib.dsp_adv_disc_work_bytes(B, F, H, S, env.nat.C.byref(out)))
    work = _canaries(env, out.value // 4 + GUARD)
    ptr = lambda k: None if k in nulls else bufs[k].data_ptr()
    rc = env.lib.dsp_adv_disc_train(
        feat.data_ptr(), F + pad, B, F, H, S, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), spk.data_ptr(),
        None if go is None else go.data_ptr(), 123.0 if device_gamma else float(gamma), None if dg is None else dg.data_ptr(),
        ptr('a'), ptr('logits2'), S + pad, ptr('loss2'), ptr('dz'), ptr('dfeat'), F + pad, ptr('dW1'), ptr('db1'), ptr('dW2'), ptr('db2'),
        None if metrics is None else metrics.state.data_ptr(), 0 if metrics is None else metrics.wrong_capacity, work.data_ptr(),
        out.value, torch.cuda.current_stream(env.dev).cuda_stream)
    env.nat.check(rc)
    torch.cuda.synchronize(env.dev)
    res = {}
    for k, (r, cols, ld) in sizes.items():
        w = _bits(bufs[k])
        assert (w[r * ld:] == np.int32(CAN_BITS)).all(), f'{k}: a word behind the output was written'
        body = w[:r * ld].reshape(r, ld)
        if k in nulls:
            assert (body == np.int32(CAN_BITS)).all(), f'{k}: a NULL output was written'
            continue
        assert (body[:, cols:] == np.int32(CAN_BITS)).all(), f'{k}: a word between the rows was written'
        res[k] = body[:, :cols].copy()
    assert (_bits(work)[out.value // 4:] == np.int32(CAN_BITS)).all(), 'a word behind the workspace was written'
    fw = _bits(fbuf)
    assert (fw[:offset] == np.int32(CAN_BITS)).all() and (fw[offset + B * (F + pad):] == np.int32(CAN_BITS)).all()
    assert (fw[offset:offset + B * (F + pad)].reshape(B, F + pad)[:, F:] == np.int32(CAN_BITS)).all(), 'the padding of feat was written'
    assert np.array_equal(fw[offset:offset + B * (F + pad)].reshape(B, F + pad)[:, :F], c.feat.view(np.int32)), 'feat was written'
    return res


def _f64(bits):
    return bits.view(np.float32).astype(np.float64)


def _errors(got, ref):
    """Per tensor max |got - ref| / max |ref|; a tensor whose largest value is below 1e-9 of the case's largest is measured
    against that (tests/test_gpu_attn_train.py)."""
    names = ('logits2', 'dfeat', 'dW1', 'db1', 'dW2', 'db2')
    top = max(float(np.max(np.abs(getattr(ref, n)))) for n in names)
    errs = {}
    for n in names:
        r = getattr(ref, n)
        scale = float(np.max(np.abs(r)))
        if scale < 1e-9 * top:
            scale = top
        errs[n] = float(np.max(np.abs(np.asarray(got[n], dtype=np.float64).reshape(r.shape) - r))) / scale
    return errs


def _xent64(logits, speakers, S):
    z = logits.astype(np.float64)
    ok = (speakers >= 0) & (speakers < S)
    m = z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z - m).sum(axis=1)) + m[:, 0]
    return float((lse[ok] - z[ok, speakers[ok]]).sum() / ok.sum())


# ---- the kernel -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('gamma', [0.01, 1.0])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_against_fp64_autograd(env, shape, gamma):
    c = _case(*shape)
    ref = _reference(env, c, gamma, (shape, gamma))
    got = _call(env, c, gamma)
    vals = {k: _f64(v) for k, v in got.items()}
    tor = _chain(env.torch, env.A, c, gamma, env.torch.float32, env.dev)
    e_nat, e_tor = _errors(vals, ref), _errors({n: getattr(tor, n) for n in OUTS}, ref)
    tag = 'x'.join(map(str, shape)) + f' gamma={gamma}'
    print(f'{tag}: native ' + ', '.join(f'{n} {v:.3g}' for n, v in e_nat.items()))
    print(f'{tag}: torch fp32 ' + ', '.join(f'{n} {v:.3g}' for n, v in e_tor.items()))
    for n in OUTS:
        record(f'adv_disc_{n}_native_vs_fp64', e_nat[n])
        record(f'adv_disc_{n}_torch_vs_fp64', e_tor[n])
    loss = float(vals['loss2'][0, 0])
    own = _xent64(got['logits2'].view(np.float32), c.speakers, c.S)
    e_own = record('adv_disc_loss2_vs_fp64_of_own_logits_of_bar', abs(loss - own) / (EPS * max(1.0, abs(own))))
    e_chain = record('adv_disc_loss2_native_vs_fp64', abs(loss - float(ref.loss2)) / max(1.0, abs(float(ref.loss2))))
    record('adv_disc_loss2_torch_vs_fp64', abs(float(tor.loss2) - float(ref.loss2)) / max(1.0, abs(float(ref.loss2))))
    print(f'{tag}: loss2 {loss:.9g} against {float(ref.loss2):.12g}: {e_own:.3f} of the loss bar on its own logits, {e_chain:.3g} of the chain')
    for n in OUTS:
        assert np.isfinite(vals[n]).all(), n
        assert e_nat[n] <= BAR, (n, e_nat[n])
    assert e_own <= 1.0 and e_chain <= BAR
    # gamma from device memory (the by-value argument is then ignored): the same bits; and a second run
    again, dev_g = _call(env, c, gamma), _call(env, c, gamma, device_gamma=True)
    for k in got:
        assert np.array_equal(got[k], again[k]), f'{k}: two runs differ'
        assert np.array_equal(got[k], dev_g[k]), f'{k}: gamma by value and gamma in device memory differ'


def test_strides_views_and_null_outputs(env):
    c = _case(17, 400, 200, 35)
    ref = _reference(env, c, 0.01, ((17, 400, 200, 35), 0.01))
    base = _call(env, c)
    padded = _call(env, c, pad=3)                                           # row strides F + 3 / S + 3: no 16-byte loads on feat
    e = _errors({k: _f64(v) for k, v in padded.items()}, ref)
    assert max(e.values()) <= BAR, e
    for k in base:                                                          # the values loaded are the same, and so are the bits
        assert np.array_equal(base[k], padded[k]), f'{k}: a row stride above the columns changed the bits'
    shifted = _call(env, c, offset=1)                                       # feat, W1, W2 4-byte aligned, not 16
    for k in base:
        assert np.array_equal(base[k], shifted[k]), f'{k}: a 4-byte-aligned view changed the bits'
    for nulls in (('dW1', 'db1'), ('dfeat',), ('dW2', 'db2', 'logits2'), ('dW1',), ('db2',), OUTS):
        part = _call(env, c, nulls=nulls)
        assert set(part) == set(base) - set(nulls)
        for k in part:
            assert np.array_equal(base[k], part[k]), f'{k} changed with {nulls} NULL'


def test_ignored_speakers_grad_out_and_metrics(env):
    B, F, H, S = 33, 64, 16, 64
    c = _case(B, F, H, S, seed=1)
    c.speakers[[0, 7, 32]] = IGNORE
    c.speakers[[3, 20]] = [S, -1]                                           # out of range: ignored and counted as bad labels
    m = env.M.Metrics(S, 8)
    got = _call(env, c, gamma=1.0, grad_out=0.5, metrics=m)
    ref = _chain(env.torch, env.A, c, 1.0, env.torch.float64, env.torch.device('cpu'), grad_out=0.5)
    e = _errors({k: _f64(v) for k, v in got.items()}, ref)
    print('ignored speakers: ' + ', '.join(f'{n} {v:.3g}' for n, v in e.items()))
    assert max(e.values()) <= BAR, e
    dead = [0, 3, 7, 20, 32]
    assert not got['dz'][dead].any(), 'dz: an ignored row is not exact +0.0'
    assert got['dz'][[1, 2, 4]].any(axis=1).all()
    assert not got['dfeat'][dead].view(np.float32).any()                    # (zero rows of dz give zero rows of dfeat)
    r = m.result()
    assert (r.seen, r.scored, r.ignored, r.bad_label, r.calls) == (B, B - 5, 5, 2, 1)
    assert r.correct + r.wrong_total == r.scored and int(r.confusion.sum()) == r.scored
    own = _xent64(got['logits2'].view(np.float32), c.speakers, S)
    assert abs(r.loss - own) <= 1e-12 * max(1.0, abs(own))
    _call(env, c, gamma=1.0, grad_out=0.5, metrics=m)                       # the counts move as the loss call documents
    r2 = m.result()
    assert (r2.seen, r2.scored, r2.ignored, r2.bad_label, r2.calls) == (2 * B, 2 * (B - 5), 10, 4, 2)
    assert np.array_equal(r2.confusion, 2 * r.confusion)


def test_forward_alone_and_the_autograd_node(env):
    torch, A = env.torch, env.A
    c = _case(17, 400, 200, 35)
    t = lambda a: torch.from_numpy(a).to(env.dev)
    feat, W1, b1, W2, b2, spk = (t(a) for a in (c.feat, c.W1, c.b1, c.W2, c.b2, c.speakers))
    full = A.disc_train(feat, W1, b1, W2, b2, spk)
    logits2, a = A.disc_forward(feat, W1, b1, W2, b2, want_a=True)
    assert torch.equal(logits2.view(torch.int32), full.logits2.view(torch.int32)) and torch.equal(a.view(torch.int32), full.a.view(torch.int32))
    # the node: unit_grad hands the stored gradients on; any other upstream gradient multiplies them
    head = A.AdvHRNNHead().to(env.dev).train()
    from features.classifier import fill_parameters
    fill_parameters(head, 5)
    grads = {}
    for route, g in (('unit', None), ('half', 0.5), ('torch', None)):
        head.zero_grad(set_to_none=True)
        x = feat.clone().requires_grad_(True)
        r = head.speaker_loss(x, spk, native=route != 'torch')
        if route == 'unit':
            env.M.backward(r.loss)
        else:
            (r.loss * g if g else r.loss).backward()
        grads[route] = [x.grad.clone()] + [p.grad.clone() for p in (head.d1.weight, head.d1.bias, head.d2.weight, head.d2.bias)]
    for u, h, tq in zip(grads['unit'], grads['half'], grads['torch']):
        assert torch.equal(h, u * 0.5)
        assert float((u - tq).abs().max()) <= BAR * float(tq.abs().max())
    # under no_grad and in eval mode: the forward kernel and the loss call alone
    with torch.no_grad():
        r = head.speaker_loss(feat, spk, native=True)
    assert not r.loss.requires_grad and float((r.logits2 - head.d2(torch.tanh(head.d1(feat))).detach()).abs().max()) <= BAR
    r_eval = head.eval().speaker_loss(feat, spk, native=True)
    assert torch.equal(r_eval.logits2, r.logits2) and torch.equal(r_eval.loss, r.loss) and not r_eval.loss.requires_grad


# ---- the head -------------------------------------------------------------------------------------------------------------------

def _head(dev, gamma=0.01, rnn_dropout=False):
    import torch
    from features import classifier as C
    torch.manual_seed(0)
    head = C.AdvHRNNHead(gamma=gamma).train()
    C.fill_parameters(head, 3)
    if not rnn_dropout:
        for m in head.modules():
            if isinstance(m, C._DynEnc):
                m.gru.dropout = 0.0
    return head.to(dev)


def _head_input(B, rows, dev):
    import torch
    rng = np.random.default_rng(B + rows)
    len0 = rng.integers(20, rows + 1, B).astype(np.int32)
    len0[B // 2] = rows
    inp = rng.standard_normal((200, B, 39)).astype(np.float32)
    for b in range(B):
        inp[len0[b]:, b] = 0.0
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(inp), t(len0), t(rng.integers(0, 20, B).astype(np.int64)), t(rng.integers(0, 35, B).astype(np.int64))


def _head_grads(head, inp, len0, labels, speakers, native_disc):
    import torch
    head.zero_grad(set_to_none=True)
    logits, logits2, loss2 = head(inp, len0, speakers=speakers, native_disc=native_disc, dropout=False, device_len=True, device_grad=True)
    loss = torch.nn.functional.cross_entropy(logits, labels) + loss2
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in head.named_parameters()}


def _rel(a, b, top):
    scale = float(np.max(np.abs(b)))
    return float(np.max(np.abs(a - b))) / (scale if scale >= 1e-9 * top else top)


@pytest.mark.parametrize('rows', [200, 131])
@pytest.mark.parametrize('B', [5, 32])
def test_head_native_discriminator_against_torch_discriminator(env, B, rows):
    head = _head(env.dev)
    inp, len0, labels, speakers = _head_input(B, rows, env.dev)
    l_t, g_t = _head_grads(head, inp, len0, labels, speakers, False)
    l_n, g_n = _head_grads(head, inp, len0, labels, speakers, True)
    top = max(float(np.max(np.abs(v))) for v in g_t.values())
    errs = {n: _rel(g_n[n], g_t[n], top) for n in g_t}
    worst = max(errs, key=errs.get)
    print(f'AdvHRNNHead B={B}, {rows} of 200 rows: loss {l_n:.9g} against {l_t:.9g}, worst gradient {errs[worst]:.3g} ({worst})')
    record(f'adv_head_grads_native_vs_torch_disc_{B}_{rows}', errs[worst])
    assert abs(l_n - l_t) <= 2e-6 * max(1.0, abs(l_t))
    for n, v in errs.items():
        assert v <= BAR, (n, v)


def test_head_gradients_carry_the_reversed_term(env):
    """Against a plain ``HRNNHead`` step on the same ``g``: ``g.out.weight`` sees the label loss alone; the encoders see it plus
    the reversed speaker term, which flips sign with gamma."""
    import torch
    from features.classifier import HRNNHead
    inp, len0, labels, speakers = _head_input(5, 131, env.dev)
    pos, neg = _head(env.dev, gamma=1.0), _head(env.dev, gamma=-1.0)
    _, g_pos = _head_grads(pos, inp, len0, labels, speakers, True)
    _, g_neg = _head_grads(neg, inp, len0, labels, speakers, True)
    plain = HRNNHead().train()
    plain.load_state_dict(pos.g.state_dict())
    for m in plain.modules():
        if hasattr(m, 'gru'):
            m.gru.dropout = 0.0
    plain = plain.to(env.dev)
    logits, _ = plain(inp, len0, dropout=False, device_len=True, device_grad=True)
    torch.nn.functional.cross_entropy(logits, labels).backward()
    g_plain = {'g.' + n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in plain.named_parameters()}
    top = max(float(np.max(np.abs(v))) for v in g_plain.values())
    for n in ('g.out.weight', 'g.out.bias'):
        assert _rel(g_pos[n], g_plain[n], top) <= BAR and _rel(g_neg[n], g_plain[n], top) <= BAR, n
    moved = 0
    for n, p in g_plain.items():
        if not n.startswith(('g.enc1', 'g.enc2')):
            continue
        d_pos, d_neg = g_pos[n] - p, g_neg[n] - p                           # the reversed term at gamma = 1 and at gamma = -1
        scale = max(float(np.max(np.abs(d_pos))), 1e-30)
        assert float(np.max(np.abs(d_pos + d_neg))) <= 1e-3 * scale + BAR * top, n
        moved += float(np.max(np.abs(d_pos))) > 100 * BAR * float(np.max(np.abs(p)))
    assert moved >= 4, 'the reversed term did not reach the encoders'


# ---- the recorded step ----------------------------------------------------------------------------------------------------------

def _cut(stored, B, k):
    out = []
    for i in range(B):
        c = stored[(i + 3 * k) % len(stored)]
        frac = (0.60 + 0.05 * ((3 * i) % 5)) if k == 0 else (0.55 + 0.05 * ((7 * i + 3 * k) % 5))
        out.append(c[:int(frac * len(c)) + 7 * i + k])
    return out


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


def _same_bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def test_capture_sizes_are_the_compared_ones():
    from features.train import ADV_CAPTURE_VERIFIED, CAPTURE_VERIFIED
    assert set(ADV_CAPTURE_VERIFIED['AdvHRNNHead']) <= {32, 512} and 32 in ADV_CAPTURE_VERIFIED['AdvHRNNHead']
    assert 'AdvHRNNHead' not in CAPTURE_VERIFIED                             # (the label-only TrainBatch does not train the discriminator)


@pytest.mark.parametrize('B', [32, 512])
def test_three_replays_equal_three_eager_steps(env, B):
    torch = env.torch
    from features.optim import DeviceAdam
    from features.train import ADV_CAPTURE_VERIFIED, AdvTrainBatch
    if B not in ADV_CAPTURE_VERIFIED['AdvHRNNHead']:
        pytest.fail(f'B = {B} is not in ADV_CAPTURE_VERIFIED: this comparison is what puts it there')
    stored, rate = make_clips()
    head = _head(env.dev)
    head.device_gamma()
    twin = copy.deepcopy(head)
    tb, tb_twin = AdvTrainBatch(rate, head), AdvTrainBatch(rate, twin)
    batches = [_cut(stored, B, k) for k in range(3)]
    cap = (5 * max(sum(len(c) for c in b) for b in batches)) // 4
    rng = np.random.default_rng(B)
    content = []
    for k, clips in enumerate(batches):
        labels, speakers = rng.integers(0, 20, B).astype(np.int64), rng.integers(0, 35, B).astype(np.int64)
        labels[k % B] = IGNORE
        speakers[(k + 1) % B] = IGNORE
        content.append((np.concatenate(clips), _offsets(clips), labels, speakers, tb.draw_jitter(B, random.Random(B + k))))
    opt = DeviceAdam(list(head.parameters()), lr=1e-3)
    m, ms, m_twin, ms_twin = env.M.Metrics(20, 8), env.M.Metrics(35, 8), env.M.Metrics(20, 8), env.M.Metrics(35, 8)
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    flat, so0, l0, s0, j0 = content[0]
    buf[:len(flat)].copy_(torch.from_numpy(flat))
    lab, spk, jit = (torch.from_numpy(a).to(env.dev) for a in (l0, s0, j0))
    kw = dict(loss='native', native_disc=True, dropout=False)
    g = tb.capture(buf, so0, lab, spk, jit, optimizer=opt, capacity=cap, metrics=m, speaker_metrics=ms, **kw)
    torch.cuda.synchronize(env.dev)
    assert not m.state.cpu().numpy().any() and not ms.state.cpu().numpy().any() and opt.device_state()[0] == 0
    got = []
    for k, (flat, so, l, s, j) in enumerate(content):
        if k == 2:
            opt.set_lr(3e-4)
            head.device_gamma(0.05)
        buf.fill_(12345)
        buf[:len(flat)].copy_(torch.from_numpy(flat))
        g.sample_offsets.copy_(torch.from_numpy(so))
        for t, a in ((lab, l), (spk, s), (jit, j)):
            t.copy_(torch.from_numpy(a))
        r = g.replay()
        got.append((r.loss.clone(), r.loss_label.clone(), r.loss_speaker.clone()))
    torch.cuda.synchronize(env.dev)
    assert int(g.status.cpu()[0]) == 0
    opt_twin = DeviceAdam(list(twin.parameters()), lr=1e-3)
    want = []
    for k, (flat, so, l, s, j) in enumerate(content):
        if k == 2:
            opt_twin.set_lr(3e-4)
            twin.device_gamma(0.05)
        for p in opt_twin.params:
            p.grad = None
        t = lambda a: torch.from_numpy(a).to(env.dev)
        wave = torch.zeros(cap, dtype=torch.int16, device=env.dev)
        wave[:len(flat)].copy_(torch.from_numpy(flat))
        out = tb_twin.run(wave, so, t(l), t(s), t(j), capacity=cap, metrics=m_twin, speaker_metrics=ms_twin, **kw)
        AdvTrainBatch.backward(out)
        opt_twin.step()
        want.append((out.loss.detach().clone(), out.loss_label.detach().clone(), out.loss_speaker.detach().clone()))
    torch.cuda.synchronize(env.dev)
    differing = [(k, i) for k in range(3) for i in range(3) if not _same_bits(got[k][i], want[k][i])]
    print(f'AdvHRNNHead B={B}: losses {[[float(x) for x in row] for row in got]}, differing from the eager steps in bits: {differing}')
    assert not differing
    assert all(float(row[2]) > 0 for row in got) and float(got[0][0]) == float(got[0][1] + got[0][2])
    names = [n for n, _ in head.named_parameters()]
    bad = [n for n, p, q in zip(names, head.parameters(), twin.parameters()) if not _same_bits(p, q)]
    bad += [n + '.exp_avg' for n, p, q in zip(names, opt.exp_avg, opt_twin.exp_avg) if not _same_bits(p, q)]
    bad += [n + '.exp_avg_sq' for n, p, q in zip(names, opt.exp_avg_sq, opt_twin.exp_avg_sq) if not _same_bits(p, q)]
    assert not bad, bad
    assert opt.device_state() == opt_twin.device_state() and opt.device_state()[0] == 3
    for a, b, C in ((m, m_twin, 20), (ms, ms_twin, 35)):
        assert torch.equal(a.state, b.state), f'the metrics block over {C} classes differs'
        r = a.result()
        assert (r.seen, r.ignored, r.calls) == (3 * B, 3, 3)


def test_second_replay_equals_the_eager_step_with_dropout_on(env):
    torch = env.torch
    from features.dropout import DeviceRng
    from features.train import AdvTrainBatch
    B, dev = 32, env.dev
    stored, rate = make_clips()
    head = _head(dev, rnn_dropout=True)
    tb = AdvTrainBatch(rate, head)
    clips = [stored[i % len(stored)] for i in range(B)]
    so = _offsets(clips)
    flat = np.concatenate(clips).astype(np.int32)
    r0 = np.random.default_rng(B)
    content = [((flat if k == 0 else -flat // 2).astype(np.int16), r0.integers(0, 20, B).astype(np.int64), r0.integers(0, 35, B).astype(np.int64),
                tb.draw_jitter(B, random.Random(B + k))) for k in range(2)]
    rng = DeviceRng(20261021, dev)
    rng.set_step(11)
    kw = dict(dropout=True, rng=rng, native_disc=True, loss='native')
    buf, lab, spk, jit = (torch.from_numpy(a).to(dev) for a in content[0])
    params = list(head.parameters())
    g = tb.capture(buf, so, lab, spk, jit, **kw)
    assert rng.state_dict()['step'] == 11
    first = g.replay().logits.clone()
    torch.optim.Adam(params, lr=1e-3).step()
    for t, a in zip((buf, lab, spk, jit), content[1]):
        t.copy_(torch.from_numpy(a))
    res = g.replay()
    torch.cuda.synchronize(dev)
    second, losses, logits = [gr.clone() for gr in g.grads], (res.loss_label.clone(), res.loss_speaker.clone()), res.logits.clone()
    s = rng.state_dict()['step']
    assert s == 13 and not _same_bits(first, logits)
    rng.set_step(s - 1)
    for p in params:
        p.grad = None
    eager = tb.run(buf, so, lab, spk, jit, **kw)
    AdvTrainBatch.backward(eager)
    torch.cuda.synchronize(dev)
    bad = [n for (n, p), a in zip(head.named_parameters(), second) if not _same_bits(a, p.grad)]
    print(f'AdvHRNNHead B={B}, dropouts on: second replay against eager, differing in bits: {bad}')
    assert _same_bits(losses[0], eager.loss_label) and _same_bits(losses[1], eager.loss_speaker) and _same_bits(logits, eager.logits)
    assert not bad
    assert bool((logits == 0).any())


# ---- inference ------------------------------------------------------------------------------------------------------------------

def test_ensemble_batch_serves_the_adversarial_head(env):
    torch = env.torch
    from features.classifier import HRNNHead
    from features.ensemble import EnsembleBatch
    clips, rate = make_clips()
    flat, so = np.concatenate(clips), _offsets(clips)
    adv = _head(env.dev).eval()
    plain = HRNNHead().to(env.dev).eval()
    plain.load_state_dict(adv.g.state_dict())
    with torch.no_grad():
        a = EnsembleBatch(rate, adv, []).run(flat, so, sync_free=True, dropout=False)
        b = EnsembleBatch(rate, plain, []).run(flat, so, sync_free=True, dropout=False)
    assert torch.equal(a.pred, b.pred) and _same_bits(a.logits, b.logits)
    assert len(set(a.pred.cpu().numpy().tolist())) > 1
