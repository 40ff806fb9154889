#!/usr/bin/env python3
"""Times get_batch_full's device path on a batch that mixes 44.1 kHz and 48 kHz clips (interleaved, 1-2 s each,
device-resident int16), at B = 32 (the reference's cfg.batch_size) and B = 512:

  (a) mixed       MixedRateFeatureBatch.run: one sub-pipeline per rate, gathered clips, rows placed in the shared tensor;
  (b) workaround  what a caller writes without it, from the single-rate classes alone: the clips of each rate grouped on
                  the device with torch indexing, two ModelFeatureBatch.run calls, index_copy_ into a shared tensor;
  (c) graph       the replay of MixedRateFeatureBatch.capture.

(a) and (b) produce the same lengths and rows within 5e-5 (checked).  Device events around --iters back-to-back calls, the
three routes alternating inside every repeat, medians over --repeats.  (a) and (b) end each call with their host
synchronisation, (c) has none.  Prints one JSON line and writes it to --out.

    python tools/kbench_mixed.py [--batches 32,512] [--iters 200] [--repeats 5] [--out profiles/mixed_rate_kbench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dsp-speech-recognition_amd'))


def make_clip(rng, rate):
    """int16 background noise with one voiced burst over the middle of the clip, 1-2 s."""
    n = int(rng.uniform(1.0, 2.0) * rate)
    t = np.arange(n) / rate
    x = 40.0 * rng.standard_normal(n)
    lo, hi = int(0.2 * n), int(0.8 * n)
    f0 = rng.uniform(110.0, 240.0)
    burst = sum(a * np.sin(2 * np.pi * f0 * k * t[lo:hi] + rng.uniform(0, 6.28)) for k, a in ((1, 1.0), (2, 0.5), (3, 0.3), (7, 0.2)))
    x[lo:hi] += 6000.0 * np.hanning(hi - lo) * burst
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def bench_batch(B, iters, repeats):
    import torch
    from features import _native as nat
    from features.model_glue import MixedRateFeatureBatch, ModelFeatureBatch
    dev = torch.device('cuda', nat.current_device())
    rng = np.random.default_rng(B)
    rates = [44100 if b % 2 == 0 else 48000 for b in range(B)]
    clips = [make_clip(rng, r) for r in rates]
    so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
    waves = torch.from_numpy(np.concatenate(clips)).to(dev)

    mixed = MixedRateFeatureBatch()

    def route_a():
        return mixed.run(waves, so, rates)

    # (b): per rate, the sample indices of its clips (built once: a caller would cache them with the batch shape too)
    per_rate = []
    for rate in (44100, 48000):
        idx = [b for b in range(B) if rates[b] == rate]
        sample_idx = torch.from_numpy(np.concatenate([np.arange(so[b], so[b + 1]) for b in idx])).to(dev)
        sub_so = np.concatenate(([0], np.cumsum([so[b + 1] - so[b] for b in idx]))).astype(np.int64)
        per_rate.append((ModelFeatureBatch(rate), torch.tensor(idx, device=dev), sample_idx, sub_so, idx))

    def route_b():
        inp = torch.empty((200, B, 39), dtype=torch.float32, device=dev)
        len0 = np.empty(B, dtype=np.int32)
        for mfb, d_idx, sample_idx, sub_so, idx in per_rate:
            sub_inp, sub_len, _ = mfb.run(waves[sample_idx], sub_so)
            inp.index_copy_(1, d_idx, sub_inp)
            len0[idx] = sub_len
        return inp, len0

    graph = mixed.capture(waves, so, rates)

    def route_c():
        return graph.replay()

    inp_a, len_a, _ = route_a()
    inp_b, len_b = route_b()
    inp_c, len_c = route_c()
    torch.cuda.synchronize(dev)
    scale = float(inp_b.abs().max())
    same = bool(np.array_equal(len_a, len_b) and np.array_equal(len_a, len_c.cpu().numpy())
                and float((inp_a - inp_b).abs().max()) <= 5e-5 * scale and float((inp_c - inp_b).abs().max()) <= 5e-5 * scale)

    routes = (('mixed', route_a), ('workaround', route_b), ('graph', route_c))
    for _, f in routes:
        for _ in range(10):
            f()
    torch.cuda.synchronize(dev)
    gpu = {name: [] for name, _ in routes}
    wall = {name: [] for name, _ in routes}
    for _ in range(repeats):
        for name, f in routes:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            a.record()
            for _ in range(iters):
                f()
            b.record()
            torch.cuda.synchronize(dev)
            wall[name].append((time.perf_counter() - t0) * 1e6 / iters)
            gpu[name].append(a.elapsed_time(b) * 1e3 / iters)
    out = dict(batch=B, seconds_of_audio=round(sum(len(c) / r for c, r in zip(clips, rates)), 1), results_agree=same)
    for name, _ in routes:
        out[name + '_us_per_call_events_median'] = round(float(np.median(gpu[name])), 1)
        out[name + '_us_per_call_wall_median'] = round(float(np.median(wall[name])), 1)
        out[name + '_us_per_call_events_all'] = [round(v, 1) for v in gpu[name]]
    out['workaround_over_mixed'] = round(out['workaround_us_per_call_events_median'] / out['mixed_us_per_call_events_median'], 3)
    out['mixed_over_graph'] = round(out['mixed_us_per_call_events_median'] / out['graph_us_per_call_events_median'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='32,512')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mixed_rate_kbench.json'))
    args = ap.parse_args()
    from features import _native as nat
    nat.require_device()
    result = dict(iters=args.iters, repeats=args.repeats, shapes=[bench_batch(int(b), args.iters, args.repeats)
                                                                  for b in args.batches.split(',')])
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(json.dumps(result, indent=1) + '\n')
    return 0 if all(s['results_agree'] for s in result['shapes']) else 1


if __name__ == '__main__':
    sys.exit(main())
