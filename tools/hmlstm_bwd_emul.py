#!/usr/bin/env python3
"""The backward recurrence of the HM-LSTM (csrc/kernels_hmlstm_bwd.h behind dsp_hmlstm_backward) restated in torch, step by
step, with the tape's contents as arguments: what pins the formulas without a GPU (tests/test_hmlstm_bwd_emul.py checks it
against autograd of the fp64 step loop).

    forward_tape(params, a, x, state_in)      the loop's forward, keeping what the kernel's tape keeps
    backward(params, a, lens, state_in, tape, g_h1, g_h2, g_last)   -> dfs1 [T, B, 4 H1 + 1], dfs2 [T, B, 4 H2 + 1]
    gradients(...)                            backward + features.classifier.hm_param_grads -> dx and the seven parameter gradients

params = (U_11, U_21, W_01, bias of cell 1, U_11, W_01, bias of cell 2), state_in = (h1, c1, z1, h2, c2, z2) as [H, B] /
[1, B] or None.  Everything is [rows, B] as in hmrnn.py.  The tape of one cell: f, i, o, g, cn [T, H, B] and the mask
m = [0 <= (f_s[4H] a + 1) / 2 <= 1] [T, B]; beside it the forward's outputs h1, h2 [T, H, B] and z1, z2 [T, B].

    python tools/hmlstm_bwd_emul.py        # the check of tests/test_hmlstm_bwd_emul.py on one case, printed
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch


def _cell_forward(W_01, U_21, U_11, bias, a, c, hb, h, ht, z, zb):
    H = h.shape[0]
    fs = W_01 @ hb
    if U_21 is not None:
        fs = fs + z * (U_21 @ ht)
    fs = fs + zb * (U_11 @ h) + bias.unsqueeze(1)
    f, i, o, g = torch.sigmoid(fs[:H]), torch.sigmoid(fs[H:2 * H]), torch.sigmoid(fs[2 * H:3 * H]), torch.tanh(fs[3 * H:4 * H])
    pre = (fs[4 * H:] * a + 1) / 2.0
    keep, upd = (1 - z) * (1 - zb), (1 - z) * zb
    cn = z * (i * g) + keep * c + upd * (f * c + i * g)
    hn = (z + upd) * o * torch.tanh(cn) + keep * h
    zn = (pre.clamp(0, 1) > 0.5).to(h.dtype)
    m = ((pre >= 0) & (pre <= 1)).to(h.dtype)
    return hn, cn, zn, dict(f=f, i=i, o=o, g=g, cn=cn, m=m[0])


def forward_tape(params, a, x, state_in=None):
    """-> dict(c1=.., c2=.. (each: f, i, o, g, cn [T, H, B], m [T, B]), h1, h2 [T, H, B], z1, z2 [T, B])."""
    U11_1, U21, W01_1, b1, U11_2, W01_2, b2 = params
    T, B, _ = x.shape
    H1, H2 = U11_1.shape[1], U11_2.shape[1]
    zeros = lambda n: x.new_zeros(n, B)
    h1, c1, z1, h2, c2, z2 = state_in if state_in is not None else (zeros(H1), zeros(H1), zeros(1), zeros(H2), zeros(H2), zeros(1))
    one = x.new_ones(1, B)
    rows = {'c1': [], 'c2': [], 'h1': [], 'h2': [], 'z1': [], 'z2': []}
    for t in range(T):
        h1, c1, z1, t1 = _cell_forward(W01_1, U21, U11_1, b1, a, c1, x[t].t(), h1, h2, z1, one)
        h2, c2, z2, t2 = _cell_forward(W01_2, None, U11_2, b2, a, c2, h1, h2, None, z2, z1)
        for k, v in (('c1', t1), ('c2', t2), ('h1', h1), ('h2', h2), ('z1', z1[0]), ('z2', z2[0])):
            rows[k].append(v)
    out = {k: torch.stack(rows[k]) for k in ('h1', 'h2', 'z1', 'z2')}
    for c in ('c1', 'c2'):
        out[c] = {k: torch.stack([r[k] for r in rows[c]]) for k in rows[c][0]}
    return out


def cell_backward(tp, a, c, h, z, zb, dh, dc, dz):
    """One cell, one step.  tp: this step's f, i, o, g, cn [H, B] and m [B]; c, h: the cell's state BEFORE the step; z, zb
    [1, B]; dh, dc [H, B] and dz [1, B]: the gradients of h', c' and z'.
    -> (dfs [4H + 1, B], dc, pz, pzb, keep): dc for the step before, the pointwise parts of dz and dzb [1, B]."""
    f, i, o, g, cn = tp['f'], tp['i'], tp['o'], tp['g'], tp['cn']
    keep, upd = (1 - z) * (1 - zb), (1 - z) * zb
    s = z + upd
    tc = torch.tanh(cn)
    dot = dh * s
    dcn = dc + dot * o * (1 - tc * tc)
    do = dot * tc
    dig = dcn * s
    df = dcn * upd * c
    dfs = torch.cat([df * f * (1 - f), dig * g * i * (1 - i), do * o * (1 - o), dig * i * (1 - g * g), dz * tp['m'] * (a / 2.0)], 0)
    ig = i * g
    pz = (dcn * (ig - (1 - zb) * c - zb * (f * c + ig)) + dh * (o * tc - (1 - zb) * h - zb * o * tc)).sum(0, keepdim=True)
    pzb = (dcn * (1 - z) * (f * c + ig - c) + dh * (1 - z) * (o * tc - h)).sum(0, keepdim=True)
    return dfs, dcn * (keep + upd * f), pz, pzb, keep


def backward(params, a, lens, state_in, tape, g_h1=None, g_h2=None, g_last=None):
    """The T steps, t = T - 1 .. 0.  g_h1 [B, T, H1], g_h2 [B, T, H2], g_last [B, H2] (each may be None); lens [B] or None."""
    U11_1, U21, W01_1, _, U11_2, W01_2, _ = params
    h1s, h2s, z1s, z2s = tape['h1'], tape['h2'], tape['z1'], tape['z2']
    T, H1, B = h1s.shape
    H2 = h2s.shape[1]
    zeros = lambda n: h1s.new_zeros(n, B)
    h1_0, c1_0, z1_0, h2_0, c2_0, z2_0 = state_in if state_in is not None else (zeros(H1), zeros(H1), zeros(1), zeros(H2), zeros(H2), zeros(1))
    last_t = (torch.as_tensor(lens).clamp(1, T) - 1) if lens is not None else torch.full((B,), T - 1)
    dh1, dc1, dz1, dh2, dc2, dz2 = zeros(H1), zeros(H1), zeros(1), zeros(H2), zeros(H2), zeros(1)
    dfs1, dfs2 = [None] * T, [None] * T
    one = h1s.new_ones(1, B)
    for t in range(T - 1, -1, -1):
        step = lambda d: {k: v[t] for k, v in d.items()}
        h1p, c1p, z1p = (h1s[t - 1], tape['c1']['cn'][t - 1], z1s[t - 1:t]) if t else (h1_0, c1_0, z1_0)
        h2p, c2p, z2p = (h2s[t - 1], tape['c2']['cn'][t - 1], z2s[t - 1:t]) if t else (h2_0, c2_0, z2_0)
        z1t = z1s[t:t + 1]
        # 1. what the loss sends to this step's outputs
        if g_h1 is not None: dh1 = dh1 + g_h1[:, t].t()
        if g_h2 is not None: dh2 = dh2 + g_h2[:, t].t()
        if g_last is not None: dh2 = dh2 + g_last.t() * (last_t == t).to(h1s.dtype).unsqueeze(0)
        # 2. cell 2: z = z2 of the step before, z_bottom = z1 of this step, no top-down term
        d2, dc2, pz, pzb, keep = cell_backward(step(tape['c2']), a, c2p, h2p, z2p, z1t, dh2, dc2, dz2)
        uh = U11_2[:, :].t() @ d2
        dh2_prev = dh2 * keep + z1t * uh
        dz2 = pz
        # 3. the bottom input of cell 2 is h1 of this step, its z_bottom is z1 of this step
        dh1 = dh1 + W01_2.t() @ d2
        dz1 = dz1 + pzb + (uh * h2p).sum(0, keepdim=True)
        # 4. cell 1: z = z1 of the step before, z_bottom = 1, top = h2 of the step before
        d1, dc1, pz, _, keep = cell_backward(step(tape['c1']), a, c1p, h1p, z1p, one, dh1, dc1, dz1)
        ut = U21.t() @ d1
        dh1 = dh1 * keep + U11_1.t() @ d1
        dz1 = pz + (ut * h2p).sum(0, keepdim=True)
        # 5. the top-down term
        dh2 = dh2_prev + z1p * ut
        dfs1[t], dfs2[t] = d1.t(), d2.t()
    return torch.stack(dfs1), torch.stack(dfs2)


def gradients(params, a, x, lens, state_in, g_h1=None, g_h2=None, g_last=None):
    """forward_tape + backward + the GEMMs -> (dx, then the seven parameter gradients in the order of params)."""
    from features.classifier import hm_param_grads
    tape = forward_tape(params, a, x, state_in)
    dfs1, dfs2 = backward(params, a, lens, state_in, tape, g_h1, g_h2, g_last)
    flat = None if state_in is None else torch.cat([v.reshape(-1) for v in state_in])
    return hm_param_grads(params, x, flat, tape['h1'].permute(2, 0, 1), tape['h2'].permute(2, 0, 1), tape['z1'].t(), dfs1, dfs2)


def autograd_reference(params, a, x, lens, state_in, g_h1=None, g_h2=None, g_last=None):
    """The same gradients from autograd of the step loop (features.classifier.HMLSTM._run_torch) in the dtype of params."""
    from features.classifier import HMLSTM
    I, H1, H2 = params[2].shape[1], params[0].shape[1], params[4].shape[1]
    m = HMLSTM(a, I, [H1, H2]).to(params[0].dtype)
    with torch.no_grad():
        for p, v in zip(m._params(), params):
            p.copy_(v)
    xg = x.clone().requires_grad_(True)
    r = m._run_torch(xg, state_in, lens if lens is not None else [x.shape[0]] * x.shape[1])
    loss = 0
    for out, g in ((r.h_1, g_h1), (r.h_2, g_h2), (r.last_h2, g_last)):
        if g is not None:
            loss = loss + (out * g).sum()
    return torch.autograd.grad(loss, [xg] + m._params())


def worst_relative(got, ref):
    return max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-300)) for a, b in zip(got, ref))


def random_case(seed, I, sizes, B, T, ragged=True, with_state=True, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    H1, H2 = sizes
    sc = lambda h: 1.0 / h ** 0.5
    params = (rnd(4 * H1 + 1, H1) * sc(H1), rnd(4 * H1 + 1, H2) * sc(H1), rnd(4 * H1 + 1, I) * sc(H1), rnd(4 * H1 + 1) * sc(H1),
              rnd(4 * H2 + 1, H2) * sc(H2), rnd(4 * H2 + 1, H1) * sc(H2), rnd(4 * H2 + 1) * sc(H2))
    x = rnd(T, B, I)
    lens = torch.randint(1, T + 1, (B,), generator=g) if ragged else None
    state = None
    if with_state:
        bit = lambda: (torch.rand(1, B, generator=g) > 0.5).to(dtype)
        state = (rnd(H1, B) * 0.5, rnd(H1, B) * 0.5, bit(), rnd(H2, B) * 0.5, rnd(H2, B) * 0.5, bit())
    return params, x, lens, state, (rnd(B, T, H1), rnd(B, T, H2), rnd(B, H2))


if __name__ == '__main__':
    for I, sizes, B, T in ((24, (20, 28), 5, 9), (36, (256, 132), 3, 4)):
        params, x, lens, state, gs = random_case(1, I, sizes, B, T)
        err = worst_relative(gradients(params, 1.0, x, lens, state, *gs), autograd_reference(params, 1.0, x, lens, state, *gs))
        print(f'I {I} sizes {sizes} B {B} T {T}: worst relative deviation from autograd {err:.3g}')
