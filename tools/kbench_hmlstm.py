#!/usr/bin/env python3
"""Timing of the HM-LSTM forward (features/classifier.py::HMLSTM): the native call (dsp_hmlstm_forward, one persistent HIP
launch) against the torch step loop on the same device in the same process, alternating, at the reference's sizes
(200, [200, 200]), T = 200, B in {8, 64, 512}; and the whole HMRNNHead at B = 512 next to RNNHead.

    python tools/kbench_hmlstm.py [--out profiles/hmlstm_kbench.json] [--rounds 5]
    python tools/kbench_hmlstm.py --kernel-only B      # one warm-up and ten native calls, for a rocprofv3 --kernel-trace run
    python tools/kbench_hmlstm.py --scan-seeds          # CPU only: the seeds of tests/test_gpu_hmlstm.py::LOOP_CASES

Times are device-event times around calls on one stream, median over the rounds (min and max are kept beside it); every
shape is warmed up first.  The operation count is 2 (4H+1) (I + H2 + H1 + H1 + H2) per column and step.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np
import torch


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _stats(v):
    v = sorted(v)
    return {'median_ms': v[len(v) // 2], 'min_ms': v[0], 'max_ms': v[-1]}


def scan_seeds():
    """For every (B, T, shape) of the GPU test's table: the first seed from its base whose torch-loop run on the CPU leaves
    out at most 0.25 % of the decisions under the guard rule."""
    import hmrnn_cases as hc
    import test_gpu_hmlstm as tg
    from features.classifier import HMLSTM, fill_parameters
    for B, T, shape, _ in tg.LOOP_CASES:
        I, sizes = tg.SHAPES[shape]
        for seed in range(20260700, 20260700 + 200):
            torch.manual_seed(0)
            m = HMLSTM(1.0, I, list(sizes)).eval()
            fill_parameters(m, seed)
            x = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((T, B, I)).astype(np.float32))
            with torch.no_grad():
                zh = m.run(x, native=False).z_hat.numpy()
            share = hc.left_out_share(hc.cuts(zh), T)
            if share <= 0.0025:
                print(f"    ({B}, {T}, '{shape}', {seed}),   # left out {share:.4f}, boundary rates "
                      f"{(zh[:, 0] > 0.5).mean():.2f} / {(zh[:, 1] > 0.5).mean():.2f}", flush=True)
                break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--kernel-only', type=int, default=0, metavar='B')
    ap.add_argument('--scan-seeds', action='store_true')
    args = ap.parse_args()
    if args.scan_seeds:
        return scan_seeds()
    from features.classifier import HMLSTM, HMRNNHead, RNNHead, fill_parameters
    dev = torch.device('cuda', 0)
    I, sizes, T = 200, [200, 200], 200
    torch.manual_seed(0)
    m = HMLSTM(1.0, I, sizes).eval()
    fill_parameters(m, 1)
    m = m.to(dev)
    rng = np.random.default_rng(2)
    flop_col_step = 2 * ((4 * sizes[0] + 1) * (I + sizes[1] + sizes[0]) + (4 * sizes[1] + 1) * (sizes[0] + sizes[1]))
    if args.kernel_only:
        x = torch.from_numpy(rng.standard_normal((T, args.kernel_only, I)).astype(np.float32)).to(dev)
        with torch.no_grad():
            for _ in range(11):
                m.run(x, native=True)
        torch.cuda.synchronize()
        return
    res = {'shape': {'input_size': I, 'sizes': sizes, 'T': T}, 'hmlstm': {}, 'heads': {}}
    with torch.no_grad():
        for B in (8, 64, 512):
            x = torch.from_numpy(rng.standard_normal((T, B, I)).astype(np.float32)).to(dev)
            nat = lambda: m.run(x, native=True)
            seq_free = lambda: m._run_native(x, None, None, want_seq=False)      # state and z_hat only
            loop = lambda: m.run(x, native=False)
            nat(); seq_free(); loop()
            torch.cuda.synchronize()
            tn, ts, tl = [], [], []
            for _ in range(args.rounds):                                          # alternating
                tn.append(_time(nat, 5)); tl.append(_time(loop, 1)); ts.append(_time(seq_free, 5))
            flop = flop_col_step * B * T
            r = {'native': _stats(tn), 'native_no_sequence_outputs': _stats(ts), 'torch_loop': _stats(tl)}
            r['native_tflops'] = flop / (r['native']['median_ms'] * 1e-3) / 1e12
            r['speedup'] = r['torch_loop']['median_ms'] / r['native']['median_ms']
            res['hmlstm'][str(B)] = r
            print(f"B {B:4d}: native {r['native']['median_ms']:.3f} ms ({r['native_tflops']:.2f} TFLOP/s fp32), without sequence "
                  f"outputs {r['native_no_sequence_outputs']['median_ms']:.3f} ms, torch loop {r['torch_loop']['median_ms']:.2f} ms "
                  f"-> x{r['speedup']:.1f}", flush=True)
        # whole heads at B = 512 on [200, 512, 39]
        B = 512
        inp = torch.from_numpy(rng.standard_normal((T, B, 39)).astype(np.float32)).to(dev)
        len0 = rng.integers(20, T + 1, B)
        len0[0] = T
        torch.manual_seed(0)
        hm, rn = HMRNNHead().eval().to(dev), RNNHead().eval().to(dev)
        runs = {'HMRNNHead_native': lambda: hm(inp, len0, dropout=True, native=True),
                'HMRNNHead_torch_loop': lambda: hm(inp, len0, dropout=True, native=False),
                'RNNHead': lambda: rn(inp, len0)}
        for f in runs.values():
            f()
        torch.cuda.synchronize()
        ts = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, f in runs.items():
                ts[k].append(_time(f, 1 if 'loop' in k else 3))
        for k in runs:
            res['heads'][k] = _stats(ts[k])
            print(f"{k} (B = 512): {res['heads'][k]['median_ms']:.2f} ms", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
