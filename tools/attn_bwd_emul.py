#!/usr/bin/env python3
"""The backward of the two attention blocks (csrc/kernels_attn_bwd.h behind dsp_attn_backward and
dsp_selfattn_pool_backward_batch) restated in NumPy in the kernels' order of operations, callable in fp64 and in fp32: what pins
the derivation without a GPU (tests/test_attn_bwd_emul.py checks it against fp64 autograd of the torch chains) and what says,
before any device run, how far fp32 arithmetic in this order sits from fp64.

    block_forward_tape(params, x, dt)            the forward as the kernels run it, keeping what the tape keeps
    block_backward(params, tape, g_y, dt)        -> (dx [T, B, d], the seven row tensors of dsp_attn_backward's d_da)
    block_gradients(params, x, g_y, dt)          the two above and features.classifier.attn_param_grads -> dx + 13 gradients
    pool_forward / pool_backward / pool_gradients   the same for layers.SelfAttn
    autograd_reference(module, x, gw)            fp64 torch autograd of _TransformerEncoder / _SelfAttn: loss = sum(gw * out)

The order restated: the scores are recomputed from x and the folded queries q' (never from keys); the weights from the saved
max_b / sum_b statistics; the statistic D = sum_b A g_A; g_S = A (g_A - D); one reduction over u (g_q') and one over t (dx);
LayerNorm's backward as (g_n - mean g_n) / s - c sum(g_n c) / (s^2 sigma (d - 1)).  params: the 13 arrays of
``_TransformerEncoder._params()`` in module order.

    python tools/attn_bwd_emul.py        # every case of tests/test_attn_bwd_emul.py, printed
"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

EPS = 1e-3


def _unpack(params, dt):
    wq, wk, wv, a1, b1, wp, bp, w1, c1, w2, c2, a2, b2 = [np.asarray(p).astype(dt) for p in params]
    return wq[0], wk[0], wv[0], a1, b1, wp, bp, w1[:, :, 0], c1, w2[:, :, 0], c2, a2, b2


def _ln(r, a, b, eps):
    d = r.shape[-1]
    c = r - r.sum(-1, keepdims=True) / r.dtype.type(d)
    sigma = np.sqrt((c * c).sum(-1, keepdims=True) / r.dtype.type(d - 1))
    return c * (r.dtype.type(1) / (sigma + eps)) * a + b


def _ln_bwd(g, r, a, eps):
    d = r.shape[-1]
    one, dd, d1 = r.dtype.type(1), r.dtype.type(d), r.dtype.type(d - 1)
    c = r - r.sum(-1, keepdims=True) / dd
    sigma = np.sqrt((c * c).sum(-1, keepdims=True) / d1)
    s = sigma + eps
    gn = g * a
    k = (gn * c).sum(-1, keepdims=True) / (s * s * sigma * d1)
    return (gn - gn.sum(-1, keepdims=True) / dd) * (one / s) - c * k


def block_forward_tape(params, x, dt=np.float64, eps=EPS):
    """x [T, B, d] -> (tape: xb [B, T, d], qp [B, T, d], m, z [T, T], M [B, T, d]; y [T, B, d])."""
    wq, wk, wv, a1, b1, wp, bp, w1, c1, w2, c2, a2, b2 = _unpack(params, dt)
    eps = dt(eps)
    xb = np.ascontiguousarray(np.asarray(x).astype(dt).transpose(1, 0, 2))
    B, T, d = xb.shape
    qp = (np.tanh(xb @ wq) @ wk.T) * dt(1.0 / np.sqrt(float(d)))
    s = qp @ xb.transpose(0, 2, 1)                              # [B, T(t), T(u)]
    m = s.max(0)
    z = np.exp(s - m).sum(0)
    M = (np.exp(s - m) / z) @ xb
    r1 = (M @ wv) @ wp.T + bp + xb
    z1 = _ln(r1, a1, b1, eps) if T > 1 else r1
    h = np.maximum(z1 @ w1.T + c1, dt(0))
    r2 = z1 + (h @ w2.T + c2)
    y = _ln(r2, a2, b2, eps) if B > 1 else r2
    return dict(xb=xb, qp=qp, m=m, z=z, M=M), np.ascontiguousarray(y.transpose(1, 0, 2))


def block_backward(params, tape, g_y, dt=np.float64, eps=EPS):
    """-> (dx [T, B, d], [g_r2, g_pre1, g_z1, g_r1, g_o, g_q', g_preQ] each [T, B, .])."""
    wq, wk, wv, a1, b1, wp, bp, w1, c1, w2, c2, a2, b2 = _unpack(params, dt)
    eps = dt(eps)
    xb, qp, m, z, M = [tape[k].astype(dt) for k in ('xb', 'qp', 'm', 'z', 'M')]
    B, T, d = xb.shape
    g = np.asarray(g_y).astype(dt).transpose(1, 0, 2)
    # launch 1: the rows again, then back
    r1 = (M @ wv) @ wp.T + bp + xb
    z1 = _ln(r1, a1, b1, eps) if T > 1 else r1
    h = np.maximum(z1 @ w1.T + c1, dt(0))
    r2 = z1 + (h @ w2.T + c2)
    g_r2 = _ln_bwd(g, r2, a2, eps) if B > 1 else g
    g_pre1 = np.where(h > 0, g_r2 @ w2, dt(0))
    g_z1 = g_r2 + g_pre1 @ w1
    g_r1 = _ln_bwd(g_z1, r1, a1, eps) if T > 1 else g_z1
    g_o = g_r1 @ wp
    g_M = g_o @ wv.T
    # launch 2: the scores again, D
    xT = xb.transpose(0, 2, 1)
    A = np.exp(qp @ xT - m) / z
    g_A = g_M @ xT
    D = (A * g_A).sum(0)
    # launch 3: the sums over u
    g_S = A * (g_A - D)
    g_q = g_S @ xb
    Qt = np.tanh(xb @ wq)
    g_preq = ((g_q @ wk) * dt(1.0 / np.sqrt(float(d)))) * (dt(1) - Qt * Qt)
    dxr = g_r1 + g_preq @ wq.T
    # launch 4: the sums over t
    dx = dxr + (A.transpose(0, 2, 1) @ g_M + g_S.transpose(0, 2, 1) @ qp)
    tb = lambda v: np.ascontiguousarray(v.transpose(1, 0, 2))
    return tb(dx), [tb(v) for v in (g_r2, g_pre1, g_z1, g_r1, g_o, g_q, g_preq)]


def block_gradients(params, x, g_y, dt=np.float64, eps=EPS, need=None):
    """-> [dx, the 13 parameter gradients] as NumPy arrays (None where autograd gives none: a skipped LayerNorm)."""
    import torch
    from features.classifier import attn_param_grads
    tape, _ = block_forward_tape(params, x, dt, eps)
    dx, da = block_backward(params, tape, g_y, dt, eps)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(np.asarray(v).astype(dt)))
    res = attn_param_grads([t(p) for p in params], t(x), t(tape['M'].transpose(1, 0, 2)), t(g_y), [t(v) for v in da], need, eps)
    return [dx] + [None if v is None else v.numpy() for v in res]


def pool_forward(params, y, dt=np.float64):
    """params: attn.weight [H, H], attn.bias [H], v.weight [1, H], v.bias [1]; y [T, B, H] -> (out [B, H], w [T, B])."""
    W, bW, v, c = [np.asarray(p).astype(dt) for p in params]
    y = np.asarray(y).astype(dt)
    e = np.tanh(y @ W.T + bW) @ v[0] + c[0]                     # [T, B]
    ex = np.exp(e - e.max(0))
    w = ex / ex.sum(0)
    return (w[:, :, None] * y).sum(0), w


def pool_backward(params, y, w, g_out, dt=np.float64):
    """-> (g_y [T, B, H], g_pre [T, B, H], g_e [T, B], gv_part [B, H])."""
    W, bW, v, c = [np.asarray(p).astype(dt) for p in params]
    y, w, g_out = [np.asarray(a).astype(dt) for a in (y, w, g_out)]
    g_w = (y * g_out).sum(2)
    g_e = w * (g_w - (w * g_w).sum(0))
    th = np.tanh(y @ W.T + bW)
    g_pre = g_e[:, :, None] * v[0] * (dt(1) - th * th)
    g_y = w[:, :, None] * g_out + g_pre @ W
    return g_y, g_pre, g_e, (g_e[:, :, None] * th).sum(0)


def pool_gradients(params, y, g_out, dt=np.float64):
    """-> [g_y, g attn.weight, g attn.bias, g v.weight, g v.bias]."""
    _, w = pool_forward(params, y, dt)
    g_y, g_pre, g_e, gv = pool_backward(params, y, w, g_out, dt)
    T, B, H = g_y.shape
    p2 = g_pre.reshape(T * B, H)
    return [g_y, p2.T @ np.asarray(y).astype(dt).reshape(T * B, H), p2.sum(0), gv.sum(0, keepdims=True), g_e.sum().reshape(1)]


def autograd_reference(module, x, gw):
    """fp64 autograd of ``module`` (a _TransformerEncoder or a _SelfAttn, left unchanged) on the CPU: loss = sum(gw * module(x)).
    -> [d loss / dx, then d loss / d parameter in named_parameters() order] as fp64 NumPy arrays, None where there is none."""
    import torch
    mod = copy.deepcopy(module).double().cpu()
    xt = torch.from_numpy(np.asarray(x)).double().requires_grad_(True)
    out = mod(xt, native=False)
    (out * torch.from_numpy(np.asarray(gw)).double()).sum().backward()
    return [xt.grad.numpy()] + [None if p.grad is None else p.grad.numpy() for p in mod.parameters()]


def errors(got, ref):
    """Per tensor max |got - ref| / max |ref|; a tensor whose max |ref| is below 1e-9 of the case's largest is measured against
    that largest value (gradients that are zero in exact arithmetic).  None on both sides is 0."""
    top = max(float(np.max(np.abs(r))) for r in ref if r is not None)
    out = []
    for g, r in zip(got, ref):
        if r is None or g is None:
            assert r is None and g is None, 'a gradient exists on one side only'
            out.append(0.0)
            continue
        scale = float(np.max(np.abs(r)))
        if scale < 1e-9 * top:
            scale = top
        out.append(float(np.max(np.abs(np.asarray(g, dtype=np.float64) - np.asarray(r, dtype=np.float64)))) / scale)
    return out


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import attn_train_cases as cases
    for name, mod, x, gw in cases.block_cases():
        ref = cases.reference(name, mod, x, gw)
        params = [p.detach().numpy() for p in mod.parameters()]
        e64 = max(errors(block_gradients(params, x, gw, np.float64), ref))
        e32 = max(errors(block_gradients(params, x, gw, np.float32), ref))
        print(f'block {name}: fp64 emulation {e64:.3g}, fp32 emulation {e32:.3g}')
    for name, mod, y, gw in cases.pool_cases():
        ref = cases.reference(name, mod, y, gw)
        params = [p.detach().numpy() for p in mod.parameters()]
        e64 = max(errors(pool_gradients(params, y, gw, np.float64), ref))
        e32 = max(errors(pool_gradients(params, y, gw, np.float32), ref))
        print(f'pooling {name}: fp64 emulation {e64:.3g}, fp32 emulation {e32:.3g}')
