#!/usr/bin/env python3
"""Times the raw-clips-to-labels path of features/ensemble.py::EnsembleBatch with a seeded HMRNNHead, every native flag on:

  (a) replay   ``capture(...).replay()``: front end, head with the lengths on the device, pre-emphasised trim, pitch features
               and gate as ONE HIP graph, nothing synchronised;
  (b) run      ``run()``, the eager call as it was before ``capture`` existed: it downloads len0 and the endpoints between
               the front end and the head (one host synchronisation per batch);
  (c) free     ``run(sync_free=True)``: the eager launches of (a) without the graph

at B = 1, 32, 512 (the stored 16 kHz chirps of tests/ensemble_cases.py, repeated), and ``dsp_head_pool_batch`` at
[200, 512, 200] against the torch expression it replaces (``y[:rows].sum(0) / n || y[:rows].max(0).values``).

Every figure is the median of --iters back-to-back calls, each between two device events, after --warmup calls; (a) and
(b) give the same labels (checked).  Writes profiles/ensemble_graph_kbench.json and prints it as one JSON line.

    python tools/kbench_ensemble_graph.py [--iters 200] [--warmup 10] [--batches 1,32,512]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def median_us(torch, dev, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize(dev)
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batches', default='1,32,512')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ensemble_graph_kbench.json'))
    args = ap.parse_args()
    import torch
    from ensemble_cases import PAIRS, THRESHOLDS, make_clips
    from features import _native as nat
    from features.classifier import HMRNNHead, fill_parameters
    from features.ensemble import EnsembleBatch, PitchSVM
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ensemble_golden.npz')) as z:
        models = [{k: z[f'svm{p[0]}{p[1]}/{k}'] for k in ('scale', 'support_vectors', 'dual_coef', 'intercept', 'gamma', 'classes')}
                  for p in PAIRS]
    rules = [(p, t, PitchSVM.from_arrays(m['support_vectors'], m['dual_coef'], m['intercept'], m['gamma'], m['classes'], scale=m['scale']))
             for p, t, m in zip(PAIRS, THRESHOLDS, models)]
    head = HMRNNHead().to(dev).eval()
    fill_parameters(head, 3)
    stored, rate = make_clips()
    res = {'iters': args.iters, 'warmup': args.warmup, 'head': 'HMRNNHead, native=True, native_enc=True, dropout=False', 'ensemble': {}}
    with torch.no_grad():
        for B in (int(v) for v in args.batches.split(',')):
            clips = [stored[i % len(stored)] for i in range(B)]
            so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
            buf = torch.from_numpy(np.concatenate(clips)).to(dev)
            eb = EnsembleBatch(rate, head, rules)
            g = eb.capture(buf, so, dropout=False)
            run = lambda: eb.run(buf, so, dropout=False, native=True, native_enc=True)
            free = lambda: eb.run(buf, so, sync_free=True, dropout=False)
            same = bool(torch.equal(g.replay().pred, run().pred))
            row = {'seconds_of_audio': float(so[-1]) / rate, 'same_labels': same,
                   'replay_us': median_us(torch, dev, g.replay, args.iters, args.warmup),
                   'run_us': median_us(torch, dev, run, args.iters, args.warmup),
                   'sync_free_us': median_us(torch, dev, free, args.iters, args.warmup)}
            row['run_over_replay'] = row['run_us'] / row['replay_us']
            res['ensemble'][str(B)] = row
            del g
        # the pooling at the head's largest shape, lengths spread over [20, 200], rows = max(len)
        T, B, H = 200, 512, 200
        rng = np.random.default_rng(0)
        lens = rng.integers(20, T + 1, B).astype(np.int32)
        lens[0] = T
        y = torch.from_numpy(rng.standard_normal((T, B, H)).astype(np.float32)).to(dev)
        y *= (torch.arange(T, device=dev)[:, None] < torch.from_numpy(lens).to(dev)[None, :]).unsqueeze(2)      # zero rows behind each end
        d_len = torch.from_numpy(lens).to(dev)
        d_rows = torch.tensor([T], dtype=torch.int32, device=dev)
        n = d_len.to(torch.float32).unsqueeze(1)
        feat = torch.empty(B, 2 * H, dtype=torch.float32, device=dev)
        lib, st = nat.load(), torch.cuda.current_stream(dev).cuda_stream
        native = lambda: nat.check(lib.dsp_head_pool_batch(y.data_ptr(), T, B, H, d_len.data_ptr(), d_rows.data_ptr(), feat.data_ptr(),
                                                           2 * H, 0, H, st))
        chain = lambda: torch.cat([y.sum(0) / n, y.max(0).values], dim=1)
        native()
        want = chain()
        err = float((feat - want).abs().max()) / max(1.0, float(want.abs().max()))
        active = int(lens.astype(np.int64).sum()) * H * 4
        pool = {'shape': [T, B, H], 'native_us': median_us(torch, dev, native, args.iters, args.warmup),
                'torch_us': median_us(torch, dev, chain, args.iters, args.warmup), 'max_err_vs_torch': err,
                'bytes_read_native': active, 'bytes_read_torch_at_least': 2 * T * B * H * 4}
        pool['torch_over_native'] = pool['torch_us'] / pool['native_us']
        pool['native_read_GBps'] = active / pool['native_us'] / 1e3
        res['pool'] = pool
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
