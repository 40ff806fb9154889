"""features/classifier.py::HMLSTM and HMRNNHead restate hmrnn.HM_LSTM (hmrnn.py:47-154) and rnn_clf.HMRNN
(rnn_clf.py:122-164).  tests/golden/hmrnn_golden.npz holds what the REAL reference classes produced on the CPU of the
build container (tests/golden/make_hmrnn_golden.py): the torch step loop must reproduce it with the same seeded weights --
every boundary bit, and values at the CPU bar of tests/test_classifier_golden.py (2e-5 x max(1, absmax)).  The native
path is pinned to the same fixtures in tests/test_gpu_hmlstm.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hmrnn_cases as hc


@pytest.fixture(scope='module')
def g():
    return hc.load_golden()


@pytest.fixture(scope='module')
def rnn_golden():
    return np.load(os.path.join(hc.HERE, 'golden', 'rnn_golden.npz'))


def _lstm(g, tag):
    import torch
    from features.classifier import HMLSTM, fill_parameters
    I, H1, H2 = (int(v) for v in g[f'lstm_{tag}_shape'])
    torch.manual_seed(0)
    m = HMLSTM(1.0, I, [H1, H2]).eval()
    names = fill_parameters(m, int(g[f'lstm_{tag}_seed']))
    assert names == [str(n) for n in g[f'lstm_{tag}_names']]          # same parameters, same names, same order as the reference
    x, x2, hid = hc.maker().lstm_inputs(int(g[f'lstm_{tag}_seed']), I, (H1, H2), np)
    return m, x, x2, hid


def _head(g):
    import torch
    from features.classifier import HMRNNHead, fill_parameters
    torch.manual_seed(0)
    head = HMRNNHead().eval()
    names = fill_parameters(head, int(g['head_seed']))
    assert names == [str(n) for n in g['head_names']]
    return head


def test_fixtures_leave_nothing_out(g):
    """The condition of the guard rule: every decision of every committed fixture is at least 2 g away from the threshold,
    and both boundaries fire in between 2 % and 98 % of the steps."""
    assert float(g['guard']) == hc.GUARD
    keys = ['head_z_hat'] + [f'lstm_{t}_call{k}_z_hat' for t in 'ab' for k in (0, 1)]
    for k in keys:
        zh = g[k]
        assert np.min(np.abs(zh - 0.5)) >= 2 * hc.GUARD, k
        assert (hc.cuts(zh) == zh.shape[0]).all(), k
        for cell in (0, 1):
            assert 0.02 <= (zh[:, cell] > 0.5).mean() <= 0.98, (k, cell)
    assert g['lstm_a_shape'].tolist() == [200, 200, 200]
    assert len(set(g['lstm_b_shape'].tolist())) == 3                  # three different sizes: a swapped U_21 / U_11 cannot hide


def test_parameter_names_and_order_equal_the_reference(g):
    head = _head(g)
    assert [n for n, _ in head.named_parameters()] == [str(n) for n in g['head_names']]
    assert [str(n) for n in g['head_names']][8 * 2:8 * 2 + 7] == ['enc2.cell_1.U_11', 'enc2.cell_1.U_21', 'enc2.cell_1.W_01',
                                                                  'enc2.cell_1.bias', 'enc2.cell_2.U_11', 'enc2.cell_2.W_01',
                                                                  'enc2.cell_2.bias']
    m = _lstm(g, 'b')[0]
    assert [tuple(p.shape) for p in m.parameters()] == [(81, 20), (81, 28), (81, 24), (81,), (113, 28), (113, 20), (113,)]


def _compare(r, g, p, T):
    """One HMLSTMResult against the fixture entries with prefix p; every bit, values at the CPU bar."""
    steps = g['steps']
    assert np.array_equal(r.z_1.squeeze(2).numpy().astype(np.uint8), g[p + 'z_1'])
    assert np.array_equal(r.z_2.squeeze(2).numpy().astype(np.uint8), g[p + 'z_2'])
    assert np.max(np.abs(r.z_hat.numpy() - g[p + 'z_hat'])) <= hc.BAR
    for name, got in (('h_1', r.h_1), ('h_2', r.h_2)):
        want = g[p + name]
        assert np.max(np.abs(got[:, steps].numpy() - want)) <= hc.BAR * hc.scale(want), name
    for name, got in zip(('h1', 'c1', 'z1', 'h2', 'c2', 'z2'), r.hidden):
        want = g[p + 'hidden_' + name]
        assert got.shape == want.shape
        assert np.max(np.abs(got.numpy() - want)) <= hc.BAR * hc.scale(want), name


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_torch_loop_reproduces_the_reference_hm_lstm(tag, g):
    import torch
    m, x, x2, hid = _lstm(g, tag)
    with torch.no_grad():
        r0 = m.run(torch.from_numpy(x), None, native=False)
        r1 = m.run(torch.from_numpy(x2), tuple(torch.from_numpy(v) for v in hid), native=False)
        fwd = m(torch.from_numpy(x), None, native=False)
    _compare(r0, g, f'lstm_{tag}_call0_', x.shape[0])
    _compare(r1, g, f'lstm_{tag}_call1_', x.shape[0])              # the non-zero initial state
    assert len(fwd) == 5 and torch.equal(fwd[1], r0.h_2) and fwd[2].shape == (16, 200, 1)      # hmrnn.py:154


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_two_chunks_with_the_state_carried_equal_one_run(tag, g):
    import torch
    m, x, _, _ = _lstm(g, tag)
    xt = torch.from_numpy(x)
    with torch.no_grad():
        whole = m.run(xt, None, native=False)
        first = m.run(xt[:77], None, native=False)
        second = m.run(xt[77:], first.hidden, native=False)
    assert torch.equal(torch.cat([first.h_2, second.h_2], 1), whole.h_2)
    assert torch.equal(torch.cat([first.z_1, second.z_1], 1), whole.z_1)
    assert torch.equal(torch.cat([first.z_hat, second.z_hat], 0), whole.z_hat)
    for a, b in zip(second.hidden, whole.hidden):
        assert torch.equal(a, b)


def test_head_reproduces_the_reference_on_cpu(g, rnn_golden):
    import torch
    head = _head(g)
    inp = torch.from_numpy(rnn_golden['inp'])
    with torch.no_grad():
        lo, feat = head(inp, rnn_golden['len0'], dropout=False)
        lo, feat = lo.numpy(), feat.numpy()
        assert feat.shape == (8, 600) and lo.shape == (8, 20)
        assert np.max(np.abs(feat - g['head_feat_nodrop'])) <= hc.BAR * hc.scale(g['head_feat_nodrop'])
        assert np.max(np.abs(lo - g['head_logits_nodrop'])) <= hc.BAR * hc.scale(g['head_logits_nodrop'])
        # the HM-LSTM inside, on the encoder's own output: every z_hat of the reference run
        r = head.enc2.run(head.enc1(inp, rnn_golden['len0']), None, lens=rnn_golden['len0'], native=False)
        assert np.max(np.abs(r.z_hat.numpy() - g['head_z_hat'])) <= hc.BAR
        assert np.array_equal(r.z_hat.numpy() > 0.5, g['head_z_hat'] > 0.5)
        assert np.max(np.abs(r.last_h2.numpy() - g['head_feat_nodrop'][:, 400:])) <= hc.BAR
        # the always-on dropouts of the reference (rnn_clf.py:138,149): logits zeroed at a rate of 0.2, and since the
        # encoder's output is dropped too, the features differ from the ones in front of it
        torch.manual_seed(5)
        lo_d, feat_d = head(inp, rnn_golden['len0'])
        kept = lo_d.numpy() != 0
        assert 0.5 < kept.mean() < 0.98
        assert np.max(np.abs(feat_d.numpy() - feat)) > 1e-3


def test_adjust_param_raises_the_slope_the_forward_pass_reads(g):
    import torch
    m, x, _, _ = _lstm(g, 'b')
    from features.classifier import HMRNNHead
    head = HMRNNHead()
    assert head.enc2.a == 1.0
    head.adjust_param()
    assert head.enc2.a == 1.5                                         # rnn_clf.py:163-164
    with torch.no_grad():
        z1 = m.run(torch.from_numpy(x[:5]), native=False).z_hat
        m.a = 1.5
        z15 = m.run(torch.from_numpy(x[:5]), native=False).z_hat
    # step 0 starts from the same state: z_hat = clamp((1.5 f + 1) / 2) against clamp((f + 1) / 2)
    f = 2 * z1[0] - 1
    assert torch.allclose(z15[0], torch.clamp((1.5 * f + 1) / 2, 0, 1), atol=1e-6)


def test_straight_through_gradient_reaches_the_boundary_rows(g):
    """hmrnn.bound.backward hands the gradient through unchanged (hmrnn.py:37-45): the boundary row 4 H1 of cell_1.W_01 and
    cell_1.bias -- which reaches the loss through the thresholded z only -- must receive a non-zero gradient."""
    import torch
    m, x, _, _ = _lstm(g, 'b')
    m.train()
    xt = torch.from_numpy(x[:12, :4])
    h_1, h_2, z_1, z_2, hidden = m(xt)                               # a gradient is required: the torch loop, whatever the device
    assert set(np.unique(z_1.detach().numpy())) <= {0.0, 1.0}
    (h_2 ** 2).sum().backward()
    H1 = m.size_list[0]
    gw, gb = m.cell_1.W_01.grad[4 * H1], m.cell_1.bias.grad[4 * H1]
    assert torch.isfinite(gw).all() and float(gw.abs().max()) > 0 and float(gb.abs()) > 0
    assert float(m.cell_2.U_11.grad[4 * m.size_list[1]].abs().max()) > 0


def test_native_insisted_on_without_a_gpu_tensor_raises(g):
    import torch
    m, x, _, _ = _lstm(g, 'b')
    with torch.no_grad(), pytest.raises(RuntimeError, match='native path cannot run'):
        m.run(torch.from_numpy(x[:3]), native=True)


@pytest.mark.parametrize('sizes', [(0, 20, 28), (24, 20, 2), (24, 22, 28), (260, 200, 200), (200, 200, 264), (-4, 8, 8)])
def test_create_refuses_unsupported_sizes_without_a_device(sizes):
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load()
    d = nat.HmlstmDesc(sizes[0], sizes[1], sizes[2], 0, *([0] * 7))
    h = nat.c_vp(0)
    assert lib.dsp_hmlstm_create(C.byref(d), C.byref(h)) == nat.EINVAL
    assert b'multiples of 4' in lib.dsp_last_error() and not h.value
    assert lib.dsp_hmlstm_create(None, C.byref(h)) == nat.EINVAL
    # supported sizes, but NULL parameter pointers: refused before any device call as well
    d = nat.HmlstmDesc(24, 20, 28, 0, *([0] * 7))
    assert lib.dsp_hmlstm_create(C.byref(d), C.byref(h)) == nat.EINVAL
    assert lib.dsp_hmlstm_forward(None, None, 1, 1, 1.0, *([None] * 10)) == nat.EINVAL
    assert lib.dsp_hmlstm_destroy(None) == nat.OK


def test_flat_state_helpers_round_trip_in_the_documented_order():
    """_pack_state lays ``hidden`` out as h1 | c1 | z1 | h2 | c2 | z2 and _split_state hands the same six tensors back."""
    import torch
    from features.classifier import _pack_state, _split_state
    H1, H2, B = 4, 8, 3
    rng = np.random.default_rng(3)
    hidden = tuple(torch.from_numpy(rng.standard_normal((n, B)).astype(np.float32)) for n in (H1, H1, 1, H2, H2, 1))
    flat = _pack_state(hidden, H1, H2, B, dtype=torch.float32)
    assert flat.shape == ((2 * H1 + 2 * H2 + 2) * B,)
    assert torch.equal(flat, torch.cat([v.reshape(-1) for v in hidden]))        # the documented order, each part row-major [rows, B]
    back = _split_state(flat, H1, H2, B)
    assert len(back) == 6
    for got, want in zip(back, hidden):
        assert got.shape == want.shape and torch.equal(got, want)
    with pytest.raises(AssertionError, match='hidden does not fit'):
        _pack_state(hidden[:5], H1, H2, B, dtype=torch.float32)


def test_lengths_helper_takes_lists_arrays_and_tensors():
    import torch
    from features.classifier import _lengths
    want = np.array([5, 1, 3], dtype=np.int64)
    for given in ([5, 1, 3], np.array([5, 1, 3], dtype=np.int32), torch.tensor([5, 1, 3]), torch.tensor([5, 1, 3], dtype=torch.int32)):
        got = _lengths(given)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
