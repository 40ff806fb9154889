#!/usr/bin/env python3
"""Times the native attention blocks (csrc/kernels_attn.h) against the torch routes they stand beside, in one process:

  (a) block    _TransformerEncoder(39, 200, 1, 100, 100) at T = 200, B = 8 / 64 / 512: ``native=True`` (dsp_attn_forward, three
               launches) against ``native=False`` (the torch chain, which holds [B, T, T] tensors), each with the peak of
               torch.cuda.max_memory_allocated over a call above what is held in front of it;
  (b) pooling  _SelfAttn(200) on [40, 512, 200], both ways;
  (c) head     TransformerHead end to end at T = 200, B = 512 (dropout off, native_enc=True both times), native_attn both ways.

Device events around --iters back-to-back calls after a warm-up, medians over --repeats groups.  Prints one JSON document and,
with --out, writes it there (profiles/attn_kbench.json).  Every pair is compared before it is timed.

    python tools/kbench_attn.py [--iters 200] [--repeats 5] [--out profiles/attn_kbench.json]
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
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from features import _native as nat
    from features.classifier import TransformerHead, _SelfAttn, _TransformerEncoder, fill_parameters
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    rng = np.random.default_rng(0)

    def timed(call, iters):
        for _ in range(10):
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
        r = call()
        torch.cuda.synchronize(dev)
        del r
        return int(torch.cuda.max_memory_allocated(dev) - held)

    def both(make, iters):
        res = {}
        with torch.no_grad():
            got, want = make(True)(), make(False)()
            got, want = (got[0], want[0]) if isinstance(got, tuple) else (got, want)
            res['max_abs_diff'] = float((got - want).abs().max())
            res['max_abs_ref'] = float(want.abs().max())
            for name, native in (('native', True), ('torch', False)):
                call = make(native)
                res[name] = dict(timed(call, iters), peak_bytes_above_inputs=peak(call))
        res['torch_over_native'] = res['torch']['us_per_call_median'] / res['native']['us_per_call_median']
        return res

    result = dict(iters=args.iters, repeats=args.repeats, block=[], device=torch.cuda.get_device_name(dev))
    enc = _TransformerEncoder(39, 200, 1, 100, 100).eval()
    fill_parameters(enc, 7)
    enc = enc.to(dev)
    for B in (8, 64, 512):
        x = torch.from_numpy(rng.standard_normal((200, B, 39)).astype(np.float32)).to(dev)
        x[100:, 1::2] = 0.0
        r = both(lambda native, x=x: (lambda: enc(x, native=native)), args.iters if B < 512 else max(args.iters // 4, 10))
        result['block'].append(dict(T=200, B=B, **r))

    pool = _SelfAttn(200).eval()
    fill_parameters(pool, 8)
    pool = pool.to(dev)
    y = torch.from_numpy(rng.standard_normal((40, 512, 200)).astype(np.float32)).to(dev)
    result['pooling'] = dict(T=40, B=512, H=200, **both(lambda native: (lambda: pool(y, native=native)), args.iters))

    head = TransformerHead().eval()
    fill_parameters(head, 9)
    head = head.to(dev)
    B = 512
    inp = torch.from_numpy(rng.standard_normal((200, B, 39)).astype(np.float32)).to(dev)
    lens = rng.integers(20, 201, B)
    lens[0] = 200
    for b in range(B):
        inp[int(lens[b]):, b] = 0.0
    result['head'] = dict(T=200, B=B, native_enc=True,
                          **both(lambda native: (lambda: head(inp, lens, dropout=False, native_enc=True, native_attn=native)),
                                 max(args.iters // 10, 5)))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
