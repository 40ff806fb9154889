#!/usr/bin/env python3
"""Probe: what a HIP graph recorded through torch.cuda.graph replays.  (1) ``x.sum(0)`` at the shapes of the
heads' bias gradients, replayed four times on new content against the eager sum; (2) a recorded ``hipMemsetAsync``
(``dsp_memset``) of 256 bytes followed by ``add_(1)``: every replay should leave ones.  Prints what it finds, asserts nothing.

    python tools/probes/graph_memset_replay.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'dsp-speech-recognition_amd'))
import torch
from features import _native as nat

dev = torch.device('cuda', 0)
nat.require_device()
torch.manual_seed(0)


def probe(name, make, n_rep=4):
    x = make()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            y = x.sum(0)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        junk = torch.full((4096,), 7, dtype=torch.int32, device=dev)      # something else that takes and frees pool memory
        del junk
        y = x.sum(0)
        junk2 = torch.full((4096,), 9, dtype=torch.int32, device=dev)
        del junk2
    for k in range(n_rep):
        x.copy_(torch.randn_like(x))
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        want = x.sum(0)
        err = float((y - want).abs().max())
        print(f'{name}: replay {k}: max |graph - eager| = {err:.3g}, equal bits {bool(torch.equal(y, want))}', flush=True)


base = torch.randn(1000, 2, 800, device=dev)
probe('strided [1000, 600] of [1000, 2, 800]', lambda: base[:, 1, 200:])
probe('contiguous [1000, 801]', lambda: torch.randn(1000, 801, device=dev))
probe('contiguous [102400, 20]', lambda: torch.randn(102400, 20, device=dev))
probe('contiguous [6400, 600]', lambda: torch.randn(6400, 600, device=dev))
probe('contiguous [400000, 4]', lambda: torch.randn(400000, 4, device=dev))
probe('contiguous [4000000, 1]', lambda: torch.randn(4000000, 1, device=dev))

# a recorded memset followed by an increment: 1 after every replay if the memset node runs, in order, every time
for n_int in (1, 64, 4096):
    buf = torch.zeros(n_int, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        nat.check(nat.load().dsp_memset(buf.data_ptr(), 0, 4 * n_int, torch.cuda.current_stream(dev).cuda_stream))
        buf.add_(1)
    for k in range(4):
        g.replay()
        torch.cuda.synchronize(dev)
        print(f'memset of {4 * n_int} bytes + add_: replay {k}: values {sorted(set(buf.cpu().tolist()))[:6]}', flush=True)
    del g
