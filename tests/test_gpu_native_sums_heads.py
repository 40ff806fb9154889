"""``native_sums=True`` on the six classifier heads (features/classifier.py, features/adversarial.py): the whole backward of the
device-length training route off torch's reduction kernels -- ``native_wgrad`` on, the attention blocks' sums, the output layer's
dW / db and the LayerNorm statistics of ``attn_param_grads`` as native launches or products (features/wgrad.py: ``rows_gemm``,
``rows_colsum``).

Fixtures as in tests/test_gpu_device_train.py: tests/golden/rnn_golden.npz (T = 200 buffers), ``dropout=False``,
``fill_parameters``, the GRUs' inter-layer dropout 0, B = 5:
  * 'full': the column of length 200 and four others -- the kernels run all 200 rows;
  * 'sub': columns [1, 2, 4, 5, 7], lengths 57, 131, 12, 99, 64 -- the row-bounded launches stop at 131 of 200 rows.

Every head on the device route (``device_len=True, device_grad=True``; ``AdvHRNNHead`` with speakers and ``native_disc=True``):
the logits with ``native_sums=True`` equal those without it in every bit (the forward is the same launches), and every gradient
-- the input's and each parameter's -- is within 2e-5 max(1, max |ref|) of the same route without it."""
import os

import numpy as np
import pytest

import hmrnn_cases as hc
from conftest import record

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 2e-5                 # between two fp32 routes (tests/test_gpu_device_train.py)
KINDS = ['rnn', 'hrnn', 'hrnn_att', 'transformer', 'hmrnn', 'adv']
SUB = [1, 2, 4, 5, 7]


def _err(got, ref):
    ref = ref.detach().cpu().numpy().astype(np.float64)
    return float(np.max(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


@pytest.fixture(scope='module')
def env():
    import types
    import torch
    from features import classifier as C
    dev = torch.device('cuda', 0)
    rg = np.load(os.path.join(HERE, 'golden', 'rnn_golden.npz'))
    cg = np.load(os.path.join(HERE, 'golden', 'clf_golden.npz'))
    hg = hc.load_golden()
    spec = {'rnn': (C.RNNHead, int(rg['seed'])), 'hrnn': (C.HRNNHead, int(cg['seed'])), 'hrnn_att': (C.HRNNAttHead, int(cg['seed']) + 1),
            'transformer': (C.TransformerHead, int(cg['seed']) + 2), 'hmrnn': (C.HMRNNHead, int(hg['head_seed'])),
            'adv': (C.AdvHRNNHead, int(cg['seed']) + 3)}
    heads = {}
    for kind, (cls, seed) in spec.items():
        torch.manual_seed(0)
        head = cls().train()
        C.fill_parameters(head, seed)
        for m in head.modules():
            if isinstance(m, C._DynEnc):
                m.gru.dropout = 0.0
        heads[kind] = head.to(dev)
    len_all = np.asarray(rg['len0'])
    longest = int(np.argmax(len_all))
    full = [longest] + [i for i in range(len(len_all)) if i != longest][:4]
    batches = {}
    for tag, cols in (('full', full), ('sub', SUB)):
        len0 = len_all[cols]
        batches[tag] = (torch.from_numpy(np.ascontiguousarray(rg['inp'][:, cols])).to(dev), torch.from_numpy(len0.astype(np.int32)).to(dev),
                        int(len0.max()))
    assert batches['full'][2] == 200 == rg['inp'].shape[0] and batches['sub'][2] == 131
    speakers = torch.tensor([3, 34, 0, 17, 9], dtype=torch.int64, device=dev)
    return types.SimpleNamespace(dev=dev, heads=heads, batches=batches, speakers=speakers)


def _step(env, kind, tag, **extra):
    """One forward + backward of ``logits.square().sum()`` (plus the speaker loss for the adversarial head) on the device route
    -> (logits, [the input's gradient] + the parameters' gradients)."""
    import torch
    head = env.heads[kind]
    inp, len_d, _ = env.batches[tag]
    x = inp.clone().requires_grad_(True)
    head.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    kw = {} if kind == 'rnn' else {'dropout': False}
    if kind == 'adv':
        kw.update(speakers=env.speakers, native_disc=True)
    out = head(x, len_d, device_len=True, device_grad=True, **kw, **extra)
    logits = out if kind == 'rnn' else out[0]
    loss = logits.square().sum()
    if kind == 'adv':
        loss = loss + out[2]
    loss.backward()
    grads = [x.grad] + [p.grad for p in head.parameters()]
    assert all(g is not None for g in grads)
    return logits.detach().clone(), [g.clone() for g in grads]


@pytest.mark.parametrize('tag', ['full', 'sub'], ids=['200_rows', '131_of_200_rows'])
@pytest.mark.parametrize('kind', KINDS)
def test_every_gradient_against_the_route_without_it(env, kind, tag):
    import torch
    plain, native = _step(env, kind, tag), _step(env, kind, tag, native_sums=True)
    assert torch.equal(plain[0].view(torch.int32), native[0].view(torch.int32)), (kind, tag, 'the logits differ in bits')
    names = ['inp'] + [n for n, _ in env.heads[kind].named_parameters()]
    worst, at = 0.0, None
    for name, a, b in zip(names, native[1], plain[1]):
        assert torch.isfinite(a).all(), (kind, name)
        e = _err(a, b)
        if e > worst:
            worst, at = e, name
    record(f'native_sums_{kind}_grads_{tag}', worst)
    print(f'{kind} {tag}: worst gradient difference with native_sums {worst:.3g} ({at})')
    assert worst <= BAR, (kind, tag, at, worst)
    # unset is False, and an explicit False is the route as it was: the same bits
    again = _step(env, kind, tag, native_sums=False)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again[1], plain[1])), (kind, tag)


def test_refusals_on_the_device():
    """Where the device-length training route does not run, an explicit True raises; unset never does."""
    import torch
    from features import classifier as C
    dev = torch.device('cuda', 0)
    head = C.HRNNHead().train().to(dev)
    head.enc1.gru.dropout = 0.0                                                        # (no generator here: the native route would refuse the draw)
    inp = torch.zeros(200, 2, 39, device=dev)
    len_d = torch.tensor([200, 50], dtype=torch.int32, device=dev)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='native_sums=True cannot run'):
            head(inp, len_d, device_len=True, dropout=False, native_sums=True)             # no gradient is required
        head(inp, len_d, device_len=True, dropout=False)
    adv = C.AdvHRNNHead().train().to(dev)
    adv.g.enc1.gru.dropout = 0.0
    with pytest.raises(RuntimeError, match='needs speakers= and native_disc=True'):
        adv(inp, len_d, speakers=torch.zeros(2, dtype=torch.int64, device=dev), device_len=True, device_grad=True, dropout=False,
            native_sums=True)
    att = C._SelfAttn(200).to(dev)
    with pytest.raises(RuntimeError, match='_SelfAttn: native_sums=True cannot run'):
        att(torch.zeros(4, 2, 200, device=dev), native=True, native_sums=True)
    enc = C._TransformerEncoder(39, 200, 1, 100, 100).to(dev)
    with pytest.raises(RuntimeError, match='_TransformerEncoder: native_sums=True cannot run'):
        enc(inp, native=False, native_sums=True)
