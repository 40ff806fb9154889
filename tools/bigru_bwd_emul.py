#!/usr/bin/env python3
"""The backward recurrence of the bidirectional GRU encoder (csrc/kernels_bigru_bwd.h behind dsp_bigru_backward) restated in
torch, step by step, with the tape's contents as arguments, in the kernel's step order and masking, both directions: what pins
the formulas without a GPU (tests/test_bigru_bwd_emul.py checks it against autograd of the fp64 nn.GRU route).

    forward_tape(params, x, lens, drop)       the forward in the kernel's masking, keeping what its tape keeps
    backward_layer(params_l, lens, tp, g, g_hn, top)   -> da [T, B, 2, 4 H]  (n_x | r | z | n_h)
    gradients(params, x, lens, g_y, g_hn, drop)        forward_tape + per layer backward_layer and
                                                       features.classifier.gru_param_grads -> dx and every parameter gradient

params: nn.GRU's order, 8 tensors per layer (weight_ih, weight_hh, bias_ih, bias_hh of the forward direction, then of the
reverse one).  The tape of one layer: r, z, n, nh [2, T, B, H] (nh = W_hn h + b_hn, the factor r multiplied) and the layer's
output rows out [T, B, 2 H] with zero rows behind each column's end.  drop [n_layers - 1, T, B, 2 H] or None: the multipliers
of the inputs of layers >= 1.

    python tools/bigru_bwd_emul.py        # the check of tests/test_bigru_bwd_emul.py on two cases, printed
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch


def _order(direction, steps):
    """The forward's step order of one direction; the backward runs it reversed."""
    return range(steps - 1, -1, -1) if direction else range(steps)


def forward_tape(params, x, lens, drop=None):
    """-> (list of per-layer dicts r, z, n, nh [2, T, B, H] and out [T, B, 2 H]; y [T, B, H]; h_n [2 L, B, H])."""
    T, B, _ = x.shape
    L = len(params) // 8
    H = params[1].shape[1]
    lens = torch.as_tensor(lens).clamp(1, T)
    steps = int(lens.max())
    tapes, hns, inp = [], [], x
    for l in range(L):
        if l > 0 and drop is not None:
            inp = inp * drop[l - 1]
        tp = {k: x.new_zeros(2, T, B, H) for k in ('r', 'z', 'n', 'nh')}
        out = x.new_zeros(T, B, 2 * H)
        for d in (0, 1):
            w_ih, w_hh, b_ih, b_hh = params[8 * l + 4 * d:8 * l + 4 * d + 4]
            h = x.new_zeros(B, H)
            for t in _order(d, steps):
                active = (t < lens).unsqueeze(1)
                ai, ah = inp[t] @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
                r, z = torch.sigmoid(ai[:, :H] + ah[:, :H]), torch.sigmoid(ai[:, H:2 * H] + ah[:, H:2 * H])
                nh = ah[:, 2 * H:]
                n = torch.tanh(ai[:, 2 * H:] + r * nh)
                for k, v in (('r', r), ('z', z), ('n', n), ('nh', nh)):
                    tp[k][d, t] = v
                h = torch.where(active, (1 - z) * n + z * h, h)
                out[t, :, d * H:(d + 1) * H] = torch.where(active, h, torch.zeros_like(h))
            hns.append(h)
        tp['out'] = out
        tapes.append(tp)
        inp = out
    mask = (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).unsqueeze(2)
    y = torch.where(mask, out[:, :, :H] + out[:, :, H:], torch.zeros_like(out[:, :, :H]))
    return tapes, y, torch.stack(hns)


def backward_layer(params_l, lens, tp, g=None, g_hn=None, top=False):
    """One layer, both directions, every step in the opposite order of the forward's.  g: [T, B, H] for the top layer (y is the
    sum of the halves: both directions read the same row), [T, B, 2 H] below; g_hn [2, B, H] of this layer; either may be None."""
    out = tp['out']
    T, B, H2 = out.shape
    H = H2 // 2
    lens = torch.as_tensor(lens).clamp(1, T)
    steps = int(lens.max())
    da = out.new_zeros(T, B, 2, 4 * H)
    for d in (0, 1):
        w_hh = params_l[4 * d + 1]
        dh = g_hn[d].clone() if g_hn is not None else out.new_zeros(B, H)      # both seeds enter where the backward starts
        for t in reversed(_order(d, steps)):
            active = (t < lens).unsqueeze(1)
            r, z, n, nh = (tp[k][d, t] for k in ('r', 'z', 'n', 'nh'))
            tprev = t + 1 if d else t - 1
            if d:
                hp = torch.where((tprev < lens).unsqueeze(1), out[min(tprev, T - 1), :, H:], torch.zeros_like(dh))   # the length is tested
            else:
                hp = out[tprev, :, :H] if tprev >= 0 else torch.zeros_like(dh)
            dcur = dh
            if g is not None:
                dcur = dh + (g[t] if top else g[t, :, d * H:(d + 1) * H])
            dn, dz = dcur * (1 - z), dcur * (hp - n)
            dnp = dn * (1 - n * n)
            row = torch.cat([dnp, dnp * nh * r * (1 - r), dz * z * (1 - z), dnp * r], 1)
            row = torch.where(active, row, torch.zeros_like(row))
            da[t, :, d] = row
            dh = torch.where(active, dcur * z, dh) + row[:, H:] @ w_hh
    return da


def gradients(params, x, lens, g_y=None, g_hn=None, drop=None):
    """-> [dx, then every parameter gradient in the order of params]."""
    from features.classifier import gru_param_grads
    L = len(params) // 8
    tapes, _, _ = forward_tape(params, x, lens, drop)
    grads = [None] * (1 + 8 * L)
    g = g_y
    for l in range(L - 1, -1, -1):
        da = backward_layer(params[8 * l:8 * l + 8], lens, tapes[l], g, None if g_hn is None else g_hn[2 * l:2 * l + 2], top=l == L - 1)
        dl = drop[l - 1] if (drop is not None and l > 0) else None
        x_l = x if l == 0 else (tapes[l - 1]['out'] if dl is None else tapes[l - 1]['out'] * dl)
        res = gru_param_grads(params[8 * l:8 * l + 8], x_l, tapes[l]['out'], da, dl)
        grads[1 + 8 * l:9 + 8 * l] = res[1:]
        g = res[0]
    grads[0] = g
    return grads


def reference_forward(params, x, lens, drop=None):
    """y [T, B, H], h_n of the nn.GRU route in the dtype of params, attached to autograd: ``_DynEnc._run_torch`` itself, or -- with
    multipliers -- single-layer ``_DynEnc``s with ``drop`` applied by hand between them.  -> (y, h_n, leaves)."""
    from features.classifier import _DynEnc
    L, H, I = len(params) // 8, params[1].shape[1], params[0].shape[1]
    lens = torch.as_tensor(lens, dtype=torch.int64)
    xg = x.clone().requires_grad_(True)

    def enc(i, n, ps):
        m = _DynEnc(i, H, n).to(params[0].dtype)
        with torch.no_grad():
            for p, v in zip(m._params(), ps):
                p.copy_(v)
        return m

    if drop is None:
        m = enc(I, L, params)
        y, hn = m._run_torch(xg, lens)
        return y, hn, [xg] + m._params()
    leaves, hns, inp = [xg], [], xg
    for l in range(L):
        m = enc(I if l == 0 else 2 * H, 1, params[8 * l:8 * l + 8])
        order = torch.argsort(lens, descending=True, stable=True)
        packed = torch.nn.utils.rnn.pack_padded_sequence(inp[:, order], lens[order])
        out, hn = m.gru(packed)
        out, _ = torch.nn.utils.rnn.pad_packed_sequence(out)
        out, hn = out[:, torch.argsort(order)], hn[:, torch.argsort(order)]
        hns.append(hn)
        leaves += m._params()
        inp = out * drop[l] if l + 1 < L else out
    return out[:, :, :H] + out[:, :, H:], torch.cat(hns), leaves


def autograd_reference(params, x, lens, g_y=None, g_hn=None, drop=None):
    y, hn, leaves = reference_forward(params, x, lens, drop)
    loss = 0
    if g_y is not None: loss = loss + (y * g_y[:y.shape[0]]).sum()
    if g_hn is not None: loss = loss + (hn * g_hn).sum()
    return list(torch.autograd.grad(loss, leaves))


def worst_relative(got, ref):
    return max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-300)) for a, b in zip(got, ref))


def random_case(seed, I, H, L, B, T, dtype=torch.float64):
    """Ragged lengths that include 1 and T (B >= 2)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    sc = 1.0 / H ** 0.5
    params = []
    for l in range(L):
        i = I if l == 0 else 2 * H
        for _ in (0, 1):
            params += [rnd(3 * H, i) * sc, rnd(3 * H, H) * sc, rnd(3 * H) * sc, rnd(3 * H) * sc]
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0], lens[-1] = 1, T
    drop = None
    if L > 1:
        drop = (torch.rand(L - 1, T, B, 2 * H, generator=g) < 0.8).to(dtype) / 0.8
    return params, rnd(T, B, I), lens, rnd(T, B, H), rnd(2 * L, B, H), drop


if __name__ == '__main__':
    for I, H, L, B, T in ((13, 20, 3, 5, 9), (36, 132, 1, 3, 4)):
        params, x, lens, g_y, g_hn, drop = random_case(1, I, H, L, B, T)
        for d in (None, drop):
            err = worst_relative(gradients(params, x, lens, g_y, g_hn, d), autograd_reference(params, x, lens, g_y, g_hn, d))
            print(f'{I} -> {H} x {L} B {B} T {T} drop {d is not None}: worst relative deviation from autograd {err:.3g}')
