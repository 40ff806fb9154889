"""The cases of the attention blocks' gradient tests (tests/test_attn_bwd_emul.py on the CPU, tests/test_gpu_attn_train.py on the
device, tools/attn_bwd_emul.py printed): shapes, dims, fills and inputs are those of the forward tests (tests/test_gpu_attn.py),
the loss is a random-weighted sum of the output, the reference is fp64 autograd of the torch chain on the CPU, computed once per
case and left unchanged."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'tools') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'tools'))

from hmrnn_cases import BAR                                   # 2e-5: the project's bar for the gradients of a native fp32 kernel
from test_gpu_attn import DIMS, SHAPES, _fill, _input

FILLS = ['golden', 'wide']
POOL_SHAPES = [(1, 1, 200), (7, 3, 200), (40, 17, 200), (40, 33, 200), (9, 5, 12)]      # (T, B, H)
OVERFLOW = ('head', 33, 17, 'golden', 150.0)                  # w_ks x 150: scores beyond +-88
BLOCK_NAMES = ['x', 'w_qs', 'w_ks', 'w_vs', 'ln1.a_2', 'ln1.b_2', 'proj.weight', 'proj.bias', 'w_1.weight', 'w_1.bias',
               'w_2.weight', 'w_2.bias', 'ln2.a_2', 'ln2.b_2']
POOL_NAMES = ['y', 'attn.weight', 'attn.bias', 'v.weight', 'v.bias']

_CACHE = {}


def block_case(dims, T, B, fill, k_scale=1.0):
    """-> (name, module on the CPU in fp32, x [T, B, d], the loss weights gw [T, B, d])"""
    import torch
    from features.classifier import _TransformerEncoder
    key = ('block', dims, T, B, fill, k_scale)
    if key not in _CACHE:
        d, di, dk, dv = DIMS[dims]
        enc = _fill(_TransformerEncoder(d, di, 1, dk, dv).eval(), 11, fill)
        if k_scale != 1.0:
            with torch.no_grad():
                enc.slf_attn.w_ks.mul_(k_scale)
        x = _input(T, B, d, 1000 * T + B)
        gw = np.random.default_rng(7 * T + B).standard_normal((T, B, d)).astype(np.float32)
        name = f'{dims} {fill} T {T} B {B}' + (f' w_ks x {k_scale:g}' if k_scale != 1.0 else '')
        _CACHE[key] = (name, enc, x, gw)
    return _CACHE[key]


def block_cases():
    for fill in FILLS:
        for dims in DIMS:
            for T, B in SHAPES:
                yield block_case(dims, T, B, fill)
    dims, T, B, fill, k = OVERFLOW
    yield block_case(dims, T, B, fill, k)


def pool_case(T, B, H):
    """The wide fill, an all-zero column where B >= 3.  -> (name, module, y [T, B, H], gw [B, H])"""
    from features.classifier import _SelfAttn
    key = ('pool', T, B, H)
    if key not in _CACHE:
        pool = _fill(_SelfAttn(H).eval(), 5)
        y = _input(T, B, H, 7 * T + B)
        if B >= 3:
            y[:, 2] = 0.0
        gw = np.random.default_rng(3 * T + B).standard_normal((B, H)).astype(np.float32)
        _CACHE[key] = (f'T {T} B {B} H {H}', pool, y, gw)
    return _CACHE[key]


def pool_cases():
    for T, B, H in POOL_SHAPES:
        yield pool_case(T, B, H)


def reference(name, mod, x, gw):
    """fp64 autograd on the CPU (tools/attn_bwd_emul.py: autograd_reference), once per case."""
    import attn_bwd_emul as em
    key = ('ref', type(mod).__name__, name)
    if key not in _CACHE:
        _CACHE[key] = em.autograd_reference(mod, x, gw)
    return _CACHE[key]


def max_score(enc, x):
    """max |s| of the block's scores in fp64."""
    import torch
    with torch.no_grad():
        a = enc.slf_attn
        xb = torch.from_numpy(x).double().transpose(0, 1)
        s = torch.bmm(torch.tanh(xb @ a.w_qs[0].double()), (xb @ a.w_ks[0].double()).transpose(1, 2)) / np.sqrt(x.shape[2])
    return float(s.abs().max())
