#!/usr/bin/env python3
"""Times TRAINING through the native attention blocks (csrc/kernels_attn_bwd.h) against the torch routes, in one process:

  (a) block    _TransformerEncoder(39, 200, 1, 100, 100) at T = 200, B = 8 / 64 / 512: forward + backward (x and all 13
               parameters require a gradient), ``native=True`` (_AttnTrain: three + four launches and the parameter GEMMs)
               against ``native=False`` (autograd through the torch chain, which holds [B, T, T] tensors);
  (b) pooling  _SelfAttn(200) on [40, 512, 200], forward + backward, both ways;
  (c) heads    one training step (forward, backward; no optimizer) of TransformerHead and HRNNAttHead at T = 200, B = 512, all
               dropout off, native_enc=True both times, native_attn both ways.

Each with the peak of torch.cuda.max_memory_allocated over a call above what is held in front of it.  Device events around
--iters back-to-back calls after a warm-up, medians over --repeats groups.  Prints one JSON document and, with --out, writes it
there (profiles/attn_train_kbench.json).  Every pair's gradients are compared before it is timed.  No time here is a pass / fail
condition.

    python tools/kbench_attn_train.py [--iters 50] [--repeats 5] [--out profiles/attn_train_kbench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dsp-speech-recognition_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from features import _native as nat
    from features.classifier import HRNNAttHead, TransformerHead, _SelfAttn, _TransformerEncoder, fill_parameters
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    rng = np.random.default_rng(0)

    def timed(call, iters, warm):
        for _ in range(warm):
            call()
        out = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            for _ in range(iters):
                call()
            b.record()
            torch.cuda.synchronize(dev)
            out.append(a.elapsed_time(b) * 1e3 / iters)
        return dict(us_per_call_median=float(np.median(out)), us_per_call_all=[round(v, 1) for v in out])

    def peak(call):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        call()
        torch.cuda.synchronize(dev)
        return int(torch.cuda.max_memory_allocated(dev) - held)

    def both(module, step, iters, warm=5):
        """step(native) runs one forward + backward and leaves the gradients in .grad (set to None in front of it)."""
        res, grads = {}, {}
        for native in (True, False):
            step(native)
            grads[native] = {n: p.grad.detach().clone() for n, p in module.named_parameters() if p.grad is not None}
        top = max(float(g.abs().max()) for g in grads[False].values())
        res['worst_grad_diff_over_largest_grad'] = max(float((grads[True][n] - g).abs().max()) for n, g in grads[False].items()) / top
        for name, native in (('native', True), ('torch', False)):
            call = lambda native=native: step(native)
            res[name] = dict(timed(call, iters, warm), peak_bytes_above_inputs=peak(call))
        res['torch_over_native'] = res['torch']['us_per_call_median'] / res['native']['us_per_call_median']
        return res

    result = dict(iters=args.iters, repeats=args.repeats, block=[], device=torch.cuda.get_device_name(dev))
    enc = _TransformerEncoder(39, 200, 1, 100, 100).train()
    fill_parameters(enc, 7)
    enc = enc.to(dev)
    for B in (8, 64, 512):
        x = torch.from_numpy(rng.standard_normal((200, B, 39)).astype(np.float32)).to(dev)
        x[100:, 1::2] = 0.0
        x.requires_grad_(True)
        gw = torch.from_numpy(rng.standard_normal((200, B, 39)).astype(np.float32)).to(dev)

        def step(native, x=x, gw=gw):
            enc.zero_grad(set_to_none=True)
            x.grad = None
            torch.autograd.backward(enc(x, native=native), gw)

        result['block'].append(dict(T=200, B=B, **both(enc, step, args.iters if B < 512 else max(args.iters // 4, 5))))

    pool = _SelfAttn(200).train()
    fill_parameters(pool, 8)
    pool = pool.to(dev)
    y = torch.from_numpy(rng.standard_normal((40, 512, 200)).astype(np.float32)).to(dev).requires_grad_(True)
    gp = torch.from_numpy(rng.standard_normal((512, 200)).astype(np.float32)).to(dev)

    def pool_step(native):
        pool.zero_grad(set_to_none=True)
        y.grad = None
        torch.autograd.backward(pool(y, native=native), gp)

    result['pooling'] = dict(T=40, B=512, H=200, **both(pool, pool_step, args.iters))

    B = 512
    inp = torch.from_numpy(rng.standard_normal((200, B, 39)).astype(np.float32)).to(dev)
    lens = rng.integers(20, 201, B)
    lens[0] = 200
    for b in range(B):
        inp[int(lens[b]):, b] = 0.0
    gl = torch.from_numpy(rng.standard_normal((B, 20)).astype(np.float32)).to(dev)
    result['heads'] = {}
    for name, cls, seed in (('transformer', TransformerHead, 9), ('hrnn_att', HRNNAttHead, 10)):
        head = cls().train()
        fill_parameters(head, seed)
        for m in head.modules():
            if isinstance(m, torch.nn.GRU):
                m.dropout = 0.0                              # all dropout off: both steps see the same network
        head = head.to(dev)

        def head_step(native, head=head):
            head.zero_grad(set_to_none=True)
            lo = head(inp, lens, dropout=False, native_enc=True, native_attn=native)[0]
            torch.autograd.backward(lo, gl)

        result['heads'][name] = dict(T=200, B=B, native_enc=True, **both(head, head_step, max(args.iters // 10, 3), warm=2))
        del head
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
