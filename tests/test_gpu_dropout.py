"""Reproducible dropout on the device (csrc/kernels_dropout.h, features/dropout.py) against the NumPy restatement
tools/philox_emul.py, bit for bit:

  A  ``dsp_dropout_apply`` at sizes around the 4-element block, the 256-lane workgroup and one grid stride, aligned,
     misaligned by one element on either side and in place; a canary behind ``y``; the key written equals the state;
  B  ``dsp_dropout_apply_key`` reproduces the forward's mask after the state advanced, and the autograd gradient of
     ``device_dropout(x).mul(w).sum()`` is ``w * m`` in every bit;
  C  ``dsp_dropout_multipliers`` bounded and unbounded, exact zeros over NaN behind the bound, the clamps, a canary;
  D  ``_DynEnc._run_device_train(rng=)`` equals the same call with ``drop=`` the restatement's multipliers, under ``==``;
  E  the heads: HRNNHead's logits are the dropout-free logits times the site-0 multipliers; HMRNNHead and TransformerHead
     repeat themselves from the same state and differ one step apart."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))

import philox_emul as pe  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = (0x9abcdef0 << 32) | 0x12345678          # both key words in use
CANARY = np.float32(-7.5e33)


@pytest.fixture(scope='module')
def env():
    import types

    import torch
    from features import _native as nat
    from features.dropout import DeviceRng
    nat.require_device()
    return types.SimpleNamespace(nat=nat, lib=nat.load(), torch=torch, dev=torch.device('cuda', 0), DeviceRng=DeviceRng)


def _same(a, b):
    import torch
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def _stream(env):
    return env.torch.cuda.current_stream(env.dev).cuda_stream


@pytest.fixture(scope='module')
def big_input():
    """One input for every size of A: the first n elements of it are the case's x (a negative zero among them)."""
    x = np.random.default_rng(7).standard_normal((1 << 20) + 3).astype(np.float32)
    x[1] = -0.0
    return x


@pytest.mark.parametrize('p', [0.0, 0.2, 0.5])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 256, 257, 4099, (1 << 20) + 3])
def test_a_apply_equals_the_restatement(env, big_input, n, p):
    torch, dev = env.torch, env.dev
    rng = env.DeviceRng(SEED, dev)
    rng.set_step(5)
    step, site = 5, 2
    x_host = big_input[:n]
    want = torch.from_numpy(pe.apply(x_host, p, SEED, step, site)).to(dev)
    for name, ox, oy in (('aligned', 0, 0), ('x + 1', 1, 0), ('y + 1', 0, 1), ('in place', 0, None), ('in place + 1', 1, None)):
        xb = torch.zeros(n + 8, dtype=torch.float32, device=dev)
        xb[ox:ox + n] = torch.from_numpy(x_host).to(dev)
        if oy is None:
            yb, oy = xb, ox
            yb[oy + n:] = float(CANARY)
        else:
            yb = torch.full((n + 8,), float(CANARY), dtype=torch.float32, device=dev)
        key = torch.full((3,), -1, dtype=torch.int64, device=dev)
        x, y = xb[ox:ox + n], yb[oy:oy + n]
        assert x.data_ptr() % 16 == 4 * ox and y.data_ptr() % 16 == 4 * oy
        env.nat.check(env.lib.dsp_dropout_apply(x.data_ptr(), y.data_ptr(), n, p, site, rng.state.data_ptr(), key.data_ptr(), _stream(env)))
        assert _same(y, want), (name, n, p)
        assert bool((yb[oy + n:] == float(CANARY)).all()) and bool((yb[:oy] == (0.0 if yb is xb else float(CANARY))).all()), name
        assert key.tolist() == rng.state.tolist() + [-1], name
    assert rng.state_dict() == {'seed': SEED, 'step': step}


def test_b_apply_key_and_autograd(env):
    torch, dev = env.torch, env.dev
    from features.dropout import device_dropout
    rng = env.DeviceRng(SEED, dev)
    rng.advance()
    rng.advance()
    assert rng.state_dict() == {'seed': SEED, 'step': 2}
    n, p, site = 4099, 0.2, 1
    gen = np.random.default_rng(11)
    x_host, w_host = gen.standard_normal(n).astype(np.float32), gen.standard_normal(n).astype(np.float32)
    x, w = torch.from_numpy(x_host).to(dev), torch.from_numpy(w_host).to(dev)
    y, key = torch.empty_like(x), torch.empty(2, dtype=torch.int64, device=dev)
    env.nat.check(env.lib.dsp_dropout_apply(x.data_ptr(), y.data_ptr(), n, p, site, rng.state.data_ptr(), key.data_ptr(), _stream(env)))
    rng.advance()
    z = torch.empty_like(x)
    env.nat.check(env.lib.dsp_dropout_apply_key(x.data_ptr(), z.data_ptr(), n, p, site, key.data_ptr(), _stream(env)))
    assert _same(z, y) and _same(y, torch.from_numpy(pe.apply(x_host, p, SEED, 2, site)).to(dev))
    moved = torch.empty_like(x)
    env.nat.check(env.lib.dsp_dropout_apply(x.data_ptr(), moved.data_ptr(), n, p, site, rng.state.data_ptr(), None, _stream(env)))
    assert _same(moved, torch.from_numpy(pe.apply(x_host, p, SEED, 3, site)).to(dev)) and not _same(moved, y)
    # autograd: the state advances between forward and backward; a non-contiguous input is served
    xt = torch.from_numpy(np.ascontiguousarray(x_host[:4096].reshape(64, 64).T)).to(dev).t().requires_grad_(True)
    assert not xt.is_contiguous()
    wt = w[:4096].reshape(64, 64)
    out = device_dropout(xt, p, rng, site)
    rng.advance()
    out.mul(wt).sum().backward()
    assert _same(out, torch.from_numpy(pe.apply(x_host[:4096].reshape(64, 64), p, SEED, 3, site)).to(dev))
    assert _same(xt.grad, torch.from_numpy(pe.apply(w_host[:4096].reshape(64, 64), p, SEED, 3, site)).to(dev))      # w * m, dropped: +0.0
    with pytest.raises(ValueError):
        device_dropout(xt.detach().cpu(), p, rng, site)
    with pytest.raises(ValueError):
        device_dropout(xt, 1.0, rng, site)


def test_c_multipliers(env):
    torch, dev = env.torch, env.dev
    L, T, B, C, p, base, step = 2, 12, 5, 8, 0.2, 8, 4
    n = L * T * B * C
    rng = env.DeviceRng(SEED, dev)
    rng.set_step(step)

    def call(rows, offset=0):
        buf = torch.full((n + 8,), float('nan'), dtype=torch.float32, device=dev)
        buf[offset + n:] = float(CANARY)
        d_rows = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=dev)
        env.nat.check(env.lib.dsp_dropout_multipliers(buf.data_ptr() + 4 * offset, L, T, B, C, p, base, rng.state.data_ptr(),
                                                      None if d_rows is None else d_rows.data_ptr(), _stream(env)))
        torch.cuda.synchronize(dev)
        assert bool((buf[offset + n:] == float(CANARY)).all()) and bool(buf[:offset].isnan().all())
        return buf[offset:offset + n].reshape(L, T, B, C)

    full, bounded = call(None), call(7)
    assert _same(full, torch.from_numpy(pe.multipliers(L, T, B, C, p, SEED, step, base)).to(dev))
    assert _same(bounded, torch.from_numpy(pe.multipliers(L, T, B, C, p, SEED, step, base, rows=7)).to(dev))
    assert _same(bounded[:, :7], full[:, :7])
    assert bool((bounded[:, 7:].contiguous().view(torch.int32) == 0).all())            # exact +0.0 over the NaN fill
    assert _same(call(0), call(1)) and _same(call(99), full) and _same(call(-3), call(1)) and _same(call(12), full)
    assert _same(call(7, offset=1), bounded)                                           # the 4-byte route: the same bits
    m = rng.multipliers(L, T, B, C, p, base, torch.tensor([7], dtype=torch.int32, device=dev))
    assert _same(m, bounded)
    # a layer size that is no multiple of 4: blocks straddle neither layers nor the bound
    L2, T2, B2, C2 = 3, 5, 3, 3
    buf = torch.full((L2 * T2 * B2 * C2 + 4,), float(CANARY), dtype=torch.float32, device=dev)
    d_rows = torch.tensor([3], dtype=torch.int32, device=dev)
    env.nat.check(env.lib.dsp_dropout_multipliers(buf.data_ptr(), L2, T2, B2, C2, 0.5, 0, rng.state.data_ptr(), d_rows.data_ptr(), _stream(env)))
    assert _same(buf[:-4].reshape(L2, T2, B2, C2), torch.from_numpy(pe.multipliers(L2, T2, B2, C2, 0.5, SEED, step, 0, rows=3)).to(dev))
    assert bool((buf[-4:] == float(CANARY)).all())


@pytest.mark.parametrize('wgrad', [False, True])
def test_d_dynenc_draws_the_restatements_multipliers(env, wgrad):
    torch, dev = env.torch, env.dev
    from features import classifier as Cl
    torch.manual_seed(0)
    enc = Cl._DynEnc(8, 8, 2, dropout=0.2).train()
    Cl.fill_parameters(enc, 5)
    enc = enc.to(dev)
    T, B, lens = 12, 5, [7, 3, 5, 1, 6]
    x_host = np.random.default_rng(3).standard_normal((T, B, 8)).astype(np.float32)
    for b, n in enumerate(lens):
        x_host[n:, b] = 0
    d_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    rows = torch.tensor([max(lens)], dtype=torch.int32, device=dev)
    rng = env.DeviceRng(SEED, dev)
    rng.set_step(9)
    site = 12
    drop = torch.from_numpy(pe.multipliers(1, T, B, 16, 0.2, SEED, 9, site, rows=max(lens))).to(dev)
    res = []
    for kw in (dict(rng=rng, rng_site=site), dict(drop=drop)):
        x = torch.from_numpy(x_host).to(dev).requires_grad_(True)
        enc.zero_grad(set_to_none=True)
        y, hn = enc._run_device_train(x, d_len, wgrad=wgrad, d_rows=rows, **kw)
        (y.square().sum() + hn.sum()).backward()
        res.append([y.detach().clone(), hn.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in enc.parameters()])
    assert rng.state_dict()['step'] == 9
    names = ['y', 'hn', 'x.grad'] + [n for n, _ in enc.named_parameters()]
    assert [n for n, a, b in zip(names, *res) if not bool((a == b).all())] == []
    assert bool((drop[0, :7] == 0).any()) and float(res[0][0].abs().max()) > 0          # something was dropped, something ran


def _head(kind, dev, gru_dropout=None):
    import torch
    from features import classifier as Cl
    torch.manual_seed(0)
    head = getattr(Cl, kind)().train()
    Cl.fill_parameters(head, 3)
    if gru_dropout is not None:
        for m in head.modules():
            if isinstance(m, Cl._DynEnc):
                m.gru.dropout = gru_dropout
    return head.to(dev)


def _batch(dev, T=30, B=5):
    import torch
    lens = [30, 12, 21, 7, 26][:B]
    x = np.random.default_rng(21).standard_normal((T, B, 39)).astype(np.float32)
    for b, n in enumerate(lens):
        x[n:, b] = 0
    return torch.from_numpy(x).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev)


def test_e_hrnn_logits_are_the_plain_logits_times_the_site_0_multipliers(env):
    torch, dev = env.torch, env.dev
    head = _head('HRNNHead', dev, gru_dropout=0.0)
    inp, d_len = _batch(dev)
    rng = env.DeviceRng(SEED, dev)
    rng.set_step(6)
    with torch.no_grad():
        plain, _ = head(inp, d_len, dropout=False, device_len=True)
        got, _ = head(inp, d_len, dropout=True, device_len=True, rng=rng)
    m = torch.from_numpy(pe.multipliers(1, 1, plain.shape[0], plain.shape[1], 0.2, SEED, 6, 0)[0, 0]).to(dev)
    want = torch.where(m != 0, plain * m, torch.zeros_like(plain))                     # a dropped logit is +0.0 whatever its sign was
    assert _same(got, want) and bool((m == 0).any()) and bool((m != 0).any())


@pytest.mark.parametrize('kind', ['HMRNNHead', 'TransformerHead'])
def test_e_heads_repeat_from_the_same_state_and_move_with_the_step(env, kind):
    torch, dev = env.torch, env.dev
    head = _head(kind, dev)
    inp, d_len = _batch(dev)
    rng = env.DeviceRng(SEED, dev)

    def step(k):
        rng.set_step(k)
        head.zero_grad(set_to_none=True)
        logits = head(inp, d_len, dropout=True, device_len=True, device_grad=True, rng=rng)[0]
        logits.square().sum().backward()
        return [logits.detach().clone()] + [p.grad.clone() for p in head.parameters()]

    a, b, c = step(3), step(3), step(4)
    names = ['logits'] + [n for n, _ in head.named_parameters()]
    assert [n for n, u, v in zip(names, a, b) if not _same(u, v)] == []
    assert not _same(a[0], c[0]) and any(not _same(u, v) for u, v in zip(a[1:], c[1:]))
    assert rng.state_dict()['step'] == 4
