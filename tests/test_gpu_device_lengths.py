"""``device_len=True`` on the five classifier heads (features/classifier.py): the lengths stay a [B] int32 device tensor, the
row counts, the pooling and ``_SelfAttn``'s softmax read them there (csrc/kernels_head.h), nothing is read back.

  (a) against what the REAL reference classes produced (tests/golden/rnn_golden.npz inputs, B = 8, lengths 200 .. 12; the
      ``*_nodrop`` values of clf_golden.npz / hmrnn_golden.npz, RNN's logits) at the bar the existing head tests use on the
      device, 2e-4 max(1, |ref|); HMRNN under the guard rule of tests/hmrnn_cases.py;
  (b) against the same head called with HOST lengths and every native flag on, on the sub-batch of columns [1, 2, 4, 5, 7]
      (lengths 57, 131, 12, 99, 64: max(len0) = 131 < 200 rows of the buffer), at 2e-5 max(1, |ref|), with equal bits in the
      max-pool columns and in HMRNN's h_2 columns;
  (c) captured in a HIP graph -- which raises on any host read -- and replayed on other lengths and a column permutation
      written into the same two buffers: the bytes of the eager call;
  (d) a required gradient raises;
  (e) ``dsp_hmlstm_forward`` asked for ``last_h2`` alone -- the form the device-length HMRNN head uses, in which every
      16-column slice stops at its longest length -- gives the bits of the call with every output.
"""
import os

import numpy as np
import pytest

import hmrnn_cases as hc
from conftest import record

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_BAR = 2e-4            # (a): the bar of tests/test_classifier_golden.py and tests/test_gpu_hmlstm.py on the device
BAR = 2e-5                 # (b): the project's bar between two fp32 routes
KINDS = ['rnn', 'hrnn', 'hrnn_att', 'transformer', 'hmrnn']
SUB = [1, 2, 4, 5, 7]


def _np(t):
    return t.detach().cpu().numpy()


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


@pytest.fixture(scope='module')
def env():
    import types
    import torch
    from features import classifier as C
    dev = torch.device('cuda', 0)
    rg = np.load(os.path.join(HERE, 'golden', 'rnn_golden.npz'))
    cg = np.load(os.path.join(HERE, 'golden', 'clf_golden.npz'))
    hg = hc.load_golden()
    spec = {'rnn': (C.RNNHead, int(rg['seed']), rg['names']),
            'hrnn': (C.HRNNHead, int(cg['seed']), cg['hrnn_names']),
            'hrnn_att': (C.HRNNAttHead, int(cg['seed']) + 1, cg['hrnn_att_names']),
            'transformer': (C.TransformerHead, int(cg['seed']) + 2, cg['transformer_names']),
            'hmrnn': (C.HMRNNHead, int(hg['head_seed']), hg['head_names'])}
    heads = {}
    for kind, (cls, seed, names) in spec.items():          # filled as tests/test_classifier_golden.py fills them
        torch.manual_seed(0)
        head = cls().eval()
        assert C.fill_parameters(head, seed) == [str(n) for n in names], kind
        heads[kind] = head.to(dev)
    want = {'rnn': (None, rg['logits']), 'hmrnn': (hg['head_feat_nodrop'], hg['head_logits_nodrop'])}
    for kind in ('hrnn', 'hrnn_att', 'transformer'):
        want[kind] = (cg[kind + '_feat_nodrop'], cg[kind + '_logits_nodrop'])
    return types.SimpleNamespace(dev=dev, heads=heads, want=want, inp=rg['inp'], len0=np.asarray(rg['len0']), hg=hg)


def _device_call(env, kind, inp_d, len_d):
    """-> (logits, feat or None) with device_len=True."""
    kw = {} if kind == 'rnn' else {'dropout': False}
    out = env.heads[kind](inp_d, len_d, device_len=True, **kw)
    return (out, None) if kind == 'rnn' else (out[0], out[1])


def _host_call(env, kind, inp_d, len0):
    """The same head with host lengths and every native flag on."""
    kw = {'rnn': dict(native_enc=True), 'hrnn': dict(dropout=False, native_enc=True),
          'hrnn_att': dict(dropout=False, native_enc=True, native_attn=True),
          'transformer': dict(dropout=False, native_enc=True, native_attn=True),
          'hmrnn': dict(dropout=False, native=True, native_enc=True)}[kind]
    out = env.heads[kind](inp_d, len0, **kw)
    return (out, None) if kind == 'rnn' else (out[0], out[1])


@pytest.mark.parametrize('kind', KINDS)
def test_a_device_lengths_against_the_real_reference(env, kind):
    import torch
    assert env.len0.max() == 200 and env.len0.min() == 12 and len(env.len0) == 8
    inp_d = torch.from_numpy(env.inp).to(env.dev)
    len_d = torch.from_numpy(env.len0.astype(np.int32)).to(env.dev)
    with torch.no_grad():
        lo, feat = _device_call(env, kind, inp_d, len_d)
    want_feat, want_lo = env.want[kind]
    ok = np.ones(8, dtype=bool)
    if kind == 'hmrnn':                                    # the guard rule: h_2 at len - 1 must lie before the column's cut
        ok = env.len0 <= hc.cuts(env.hg['head_z_hat'])
        assert ok.all()                                    # (the committed fixture leaves out nothing)
        f = _np(feat)
        e = record('device_len_hmrnn_pooled_vs_reference', np.max(np.abs(f[:, :400] - want_feat[:, :400])) / hc.scale(want_feat))
        assert e <= ROCM_BAR                               # the pooled 400 columns are never left out
        e = record('device_len_hmrnn_last_h2_vs_reference', np.max(np.abs(f[ok, 400:] - want_feat[ok, 400:])) / hc.scale(want_feat))
        assert e <= ROCM_BAR
    elif feat is not None:
        e = record(f'device_len_{kind}_feat_vs_reference', _err(_np(feat), want_feat))
        print(f'{kind}: feat err {e:.3g}')
        assert e <= ROCM_BAR
    e = record(f'device_len_{kind}_logits_vs_reference', np.max(np.abs(_np(lo)[ok] - want_lo[ok])) / hc.scale(want_lo))
    print(f'{kind}: logits err {e:.3g}')
    assert e <= ROCM_BAR


@pytest.mark.parametrize('kind', KINDS)
def test_b_device_lengths_against_the_host_length_native_path(env, kind):
    import torch
    len0 = env.len0[SUB]
    assert len0.tolist() == [57, 131, 12, 99, 64]          # rows = 131 < the buffer's 200
    inp_d = torch.from_numpy(np.ascontiguousarray(env.inp[:, SUB])).to(env.dev)
    len_d = torch.from_numpy(len0.astype(np.int32)).to(env.dev)
    with torch.no_grad():
        lo, feat = _device_call(env, kind, inp_d, len_d)
        lo_h, feat_h = _host_call(env, kind, inp_d, len0)
    e = record(f'device_len_{kind}_logits_vs_host_lengths', _err(_np(lo), _np(lo_h)))
    print(f'{kind}: logits vs host lengths {e:.3g}')
    assert e <= BAR
    if feat is not None:
        e = record(f'device_len_{kind}_feat_vs_host_lengths', _err(_np(feat), _np(feat_h)))
        print(f'{kind}: feat vs host lengths {e:.3g}')
        assert e <= BAR
        H = 200
        assert torch.equal(feat[:, H:2 * H].view(torch.int32), feat_h[:, H:2 * H].view(torch.int32)), 'max-pool columns differ in bits'
        if kind == 'hmrnn':
            assert torch.equal(feat[:, 2 * H:].view(torch.int32), feat_h[:, 2 * H:].view(torch.int32)), 'h_2 columns differ in bits'


@pytest.mark.parametrize('kind', KINDS)
def test_c_capture_and_replay(env, kind):
    """torch.cuda.graph raises on anything that synchronises or reads device memory from the host while it records."""
    import torch
    dev = env.dev
    inp_buf = torch.from_numpy(env.inp).to(dev)
    len_buf = torch.from_numpy(env.len0.astype(np.int32)).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.no_grad():
        with torch.cuda.stream(side):                      # the warm-up: handles are built, code objects loaded
            _device_call(env, kind, inp_buf, len_buf)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            lo_g, feat_g = _device_call(env, kind, inp_buf, len_buf)
        # other lengths and a column permutation, written into the same two buffers
        perm = np.array([3, 7, 0, 5, 1, 6, 2, 4])
        len2 = np.minimum(env.len0[perm], [150, 64, 33, 99, 131, 7, 1, 12]).astype(np.int32)
        inp2 = env.inp[:, perm].copy()
        for b in range(8):
            inp2[len2[b]:, b] = 0.0
        inp_buf.copy_(torch.from_numpy(inp2).to(dev))
        len_buf.copy_(torch.from_numpy(len2).to(dev))
        assert int(len2.max()) < 200
        lo_e, feat_e = _device_call(env, kind, inp_buf, len_buf)
        lo_e, feat_e = lo_e.clone(), None if feat_e is None else feat_e.clone()
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(lo_g.view(torch.int32), lo_e.view(torch.int32))
        if feat_e is not None:
            assert torch.equal(feat_g.view(torch.int32), feat_e.view(torch.int32))
        # ... and it is the right answer, not only the same one: the host-length native path on that content
        lo_h, _ = _host_call(env, kind, inp_buf, len2)
        assert record(f'device_len_{kind}_replay_vs_host_lengths', _err(_np(lo_g), _np(lo_h))) <= BAR


@pytest.mark.parametrize('kind', KINDS)
def test_d_a_required_gradient_raises(env, kind):
    import torch
    inp_d = torch.from_numpy(np.ascontiguousarray(env.inp[:, SUB])).to(env.dev)
    len_d = torch.from_numpy(env.len0[SUB].astype(np.int32)).to(env.dev)
    assert torch.is_grad_enabled() and any(p.requires_grad for p in env.heads[kind].parameters())
    with pytest.raises(RuntimeError, match='a gradient is required'):
        _device_call(env, kind, inp_d, len_d)
    with torch.no_grad():                                  # lengths on the host, or of another dtype, are refused as well
        with pytest.raises(TypeError, match='int32 tensor'):
            _device_call(env, kind, inp_d, env.len0[SUB])
        with pytest.raises(TypeError, match='int32 tensor'):
            _device_call(env, kind, inp_d, len_d.long())


@pytest.mark.parametrize('T,B', [(1, 1), (40, 37), (200, 5)])
def test_e_hmlstm_last_only_equals_the_full_call(T, B):
    """B = 37: three slices, the last one ragged; lengths from 1 to T, one slice whose longest length is far below T."""
    import torch
    from features.classifier import HMLSTM, fill_parameters
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    m = HMLSTM(1.0, 20, [28, 24]).eval()
    fill_parameters(m, 11)
    m = m.to(dev)
    rng = np.random.default_rng(T + B)
    lens = rng.integers(1, T + 1, B).astype(np.int32)
    lens[0] = T
    lens[16:32] = np.minimum(lens[16:32], max(1, T // 4))
    lens[-1] = 1
    x = torch.from_numpy((3.0 * rng.standard_normal((T, B, 20))).astype(np.float32)).to(dev)
    d_len = torch.from_numpy(lens).to(dev)
    with torch.no_grad():
        full = m.run(x, None, lens=lens, native=True)
        only = m.run(x, None, lens=d_len, device_len=True)
    assert only.h_1 is None and only.hidden is None and only.z_hat is None
    assert torch.equal(only.last_h2.view(torch.int32), full.last_h2.view(torch.int32))
    want = full.h_2[torch.arange(B, device=dev), torch.from_numpy(lens.astype(np.int64) - 1).to(dev)]
    assert torch.equal(only.last_h2, want)
