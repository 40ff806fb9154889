#!/usr/bin/env python3
"""Timing of the bidirectional GRU encoder (features/classifier.py::_DynEnc): the native call (dsp_bigru_forward, one HIP
launch per layer plus the direction sum) against the nn.GRU path (sort, pack, MIOpen, unpack, sum, unsort) on the same device
in the same process, alternating, at 39 -> 200 with 1, 2 and 3 layers, T = 200, B in {8, 64, 512}, with all lengths 200 and
with ragged lengths (the voiced burst of configs[4]: 0.5 .. 0.9 of a 1 .. 2 s clip at 100 frames per second, capped at 200);
and RNNHead and HMRNNHead at B = 512 with the native encoder and without it.

    python tools/kbench_bigru.py [--out profiles/bigru_kbench.json] [--rounds 5]
    python tools/kbench_bigru.py --kernel-only B [--layers L]   # one warm-up and ten native calls, for a rocprofv3 --kernel-trace run

Times are device-event times around calls on one stream, median over the rounds (min and max are kept beside it); every
shape is warmed up first.  A direction of a layer multiplies 3 H (in + H) weights per column and step (in = 39, then 2 H).
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


def ragged_lengths(rng, B, T):
    n = (rng.uniform(0.5, 0.9, B) * rng.uniform(1.0, 2.0, B) * 100).astype(np.int64)
    return np.clip(n, 1, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--kernel-only', type=int, default=0, metavar='B')
    ap.add_argument('--layers', type=int, default=2)
    args = ap.parse_args()
    from features.classifier import _DynEnc, HMRNNHead, RNNHead, fill_parameters
    dev = torch.device('cuda', 0)
    I, H, T = 39, 200, 200
    rng = np.random.default_rng(2)

    def encoder(layers):
        torch.manual_seed(0)
        enc = _DynEnc(I, H, layers).eval()
        fill_parameters(enc, 1)
        return enc.to(dev)

    if args.kernel_only:
        enc = encoder(args.layers)
        x = torch.from_numpy(rng.standard_normal((T, args.kernel_only, I)).astype(np.float32)).to(dev)
        with torch.no_grad():
            for _ in range(11):
                enc.run(x, np.full(args.kernel_only, T), native=True)
        torch.cuda.synchronize()
        return
    res = {'shape': {'input_size': I, 'hidden': H, 'T': T}, 'encoder': {}, 'heads': {}}
    with torch.no_grad():
        for layers in (1, 2, 3):
            enc = encoder(layers)
            mac_col_step = 2 * 3 * H * ((I + H) + (layers - 1) * (2 * H + H))          # both directions
            for B in (8, 64, 512):
                x = torch.from_numpy(rng.standard_normal((T, B, I)).astype(np.float32)).to(dev)
                for kind, lens in (('full', np.full(B, T)), ('ragged', ragged_lengths(rng, B, T))):
                    nat = lambda: enc.run(x, lens, native=True)
                    gru = lambda: enc.run(x, lens, native=False)
                    nat(); gru()
                    torch.cuda.synchronize()
                    tn, tg = [], []
                    for _ in range(args.rounds):                                          # alternating
                        tn.append(_time(nat, 3)); tg.append(_time(gru, 3))
                    r = {'native': _stats(tn), 'nn_gru': _stats(tg), 'mean_len': float(lens.mean())}
                    r['speedup'] = r['nn_gru']['median_ms'] / r['native']['median_ms']
                    r['native_ahead_beyond_ranges'] = r['native']['max_ms'] < r['nn_gru']['min_ms']
                    if kind == 'full':
                        r['native_tflops'] = 2 * mac_col_step * B * T / (r['native']['median_ms'] * 1e-3) / 1e12
                        r['native_us_per_step_and_layer'] = r['native']['median_ms'] * 1e3 / (T * layers)
                    res['encoder'][f'layers{layers}_B{B}_{kind}'] = r
                    print(f"layers {layers} B {B:4d} {kind:6s}: native {r['native']['median_ms']:.3f} ms "
                          f"[{r['native']['min_ms']:.3f}, {r['native']['max_ms']:.3f}], nn.GRU {r['nn_gru']['median_ms']:.3f} ms "
                          f"[{r['nn_gru']['min_ms']:.3f}, {r['nn_gru']['max_ms']:.3f}] -> x{r['speedup']:.2f}", flush=True)
        # whole heads at B = 512 on [200, 512, 39]
        B = 512
        inp = torch.from_numpy(rng.standard_normal((T, B, I)).astype(np.float32)).to(dev)
        len0 = ragged_lengths(rng, B, T)
        len0[0] = T
        torch.manual_seed(0)
        hm, rn = HMRNNHead().eval().to(dev), RNNHead().eval().to(dev)
        runs = {'RNNHead_native_enc': lambda: rn(inp, len0, native_enc=True),
                'RNNHead_nn_gru': lambda: rn(inp, len0, native_enc=False),
                'HMRNNHead_native_enc': lambda: hm(inp, len0, dropout=True, native=True, native_enc=True),
                'HMRNNHead_nn_gru': lambda: hm(inp, len0, dropout=True, native=True, native_enc=False)}
        for f in runs.values():
            f()
        torch.cuda.synchronize()
        ts = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, f in runs.items():
                ts[k].append(_time(f, 3))
        for k in runs:
            res['heads'][k] = _stats(ts[k])
            print(f"{k} (B = 512, ragged): {res['heads'][k]['median_ms']:.2f} ms "
                  f"[{res['heads'][k]['min_ms']:.2f}, {res['heads'][k]['max_ms']:.2f}]", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
