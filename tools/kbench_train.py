#!/usr/bin/env python3
"""Times one training step -- front end on raw clips with the endpoint jitter, head, cross-entropy, backward, an eager Adam
step -- of ``HMRNNHead`` and ``TransformerHead`` (seeded weights, training mode, both F.dropout calls on) three ways:

  (1) host     the route with the lengths on the host and every native flag on: ``ModelFeatureBatch.run`` downloads len0 (one
               synchronisation), the head runs with ``native=True / native_enc=True / native_attn=True``, and every step
               rebuilds the native handles because the optimiser wrote the parameters;
      host_keep  the same step with the optimiser working on a shadow copy of the parameters, so that the handles stay:
               (1) minus this is what the handle re-creation costs;
  (2) run      ``TrainBatch.run`` + ``backward``: lengths on the device, handles repacked in place, nothing synchronised;
  (3) replay   ``TrainBatch.capture(...).replay()``: refresh, front end, forward, loss and backward as ONE HIP graph

at B = 32 (the reference's cfg.batch_size) and B = 512, on the stored 16 kHz chirps of tests/ensemble_cases.py, repeated.

The host route takes the jitter as a host array and uploads it on every step (16 bytes per clip, pageable memory), which is
what that route does in a training loop; the device routes read a jitter already on the device.  ``capture`` serves the head / size
pairs of ``features.train.CAPTURE_VERIFIED``, which hold the defaults here.

Every figure is a host clock around --iters back-to-back steps that end in a device synchronise, divided by --iters, after
--warmup steps; the routes are timed one after the other in each of --rounds rounds and the median round is reported (all
rounds are kept in the JSON).  Writes --out (default profiles/train_kbench.json) and prints it as one JSON line.

    python tools/kbench_train.py [--iters 20] [--warmup 3] [--rounds 3] [--batches 32,512] [--heads hmrnn,transformer]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def per_step_us(torch, dev, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', default='32,512')
    ap.add_argument('--heads', default='hmrnn,transformer')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_kbench.json'))
    args = ap.parse_args()
    import torch
    from ensemble_cases import make_clips
    from features import _native as nat
    from features.classifier import HMRNNHead, TransformerHead, fill_parameters
    from features.model_glue import ModelFeatureBatch
    from features.train import TrainBatch
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    stored, rate = make_clips()
    kinds = {'hmrnn': (HMRNNHead, dict(native=True, native_enc=True)), 'transformer': (TransformerHead, dict(native_enc=True, native_attn=True))}
    res = {'iters': args.iters, 'warmup': args.warmup, 'rounds': args.rounds, 'optimizer': 'torch.optim.Adam(lr=1e-4), eager',
           'clock': 'host clock around iters steps ending in a device synchronise', 'steps': {}}
    for kind in args.heads.split(','):
        cls, host_kw = kinds[kind]
        for B in (int(v) for v in args.batches.split(',')):
            torch.manual_seed(0)
            head = cls().train()
            fill_parameters(head, 3)
            head = head.to(dev)
            params = list(head.parameters())
            opt = torch.optim.Adam(params, lr=1e-4)
            shadow = [p.detach().clone() for p in params]
            opt_shadow = torch.optim.Adam(shadow, lr=1e-4)
            clips = [stored[i % len(stored)] for i in range(B)]
            so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
            buf = torch.from_numpy(np.concatenate(clips)).to(dev)
            labels = torch.from_numpy(np.random.default_rng(B).integers(0, 20, B).astype(np.int64)).to(dev)
            mfb, tb = ModelFeatureBatch(rate), TrainBatch(rate, head)
            jitter = tb.draw_jitter(B, random.Random(B))
            d_jit = torch.from_numpy(jitter).to(dev)

            def host(keep=False):
                inp, len0, _ = mfb.run(buf, so, jitter=jitter)
                loss = torch.nn.functional.cross_entropy(head(inp, len0, **host_kw)[0], labels)
                opt.zero_grad()
                loss.backward()
                if keep:                                     # the same Adam arithmetic on tensors the handles do not watch
                    for s, p in zip(shadow, params):
                        s.grad = p.grad
                    opt_shadow.step()
                else:
                    opt.step()

            def run():
                out = tb.run(buf, so, labels, d_jit)
                opt.zero_grad()
                out.loss.backward()
                opt.step()

            rounds = {'host_us': [], 'host_keep_us': [], 'run_us': [], 'replay_us': []}
            for _ in range(args.rounds):
                rounds['host_us'].append(per_step_us(torch, dev, host, args.iters, args.warmup))
                rounds['host_keep_us'].append(per_step_us(torch, dev, lambda: host(True), args.iters, args.warmup))
                rounds['run_us'].append(per_step_us(torch, dev, run, args.iters, args.warmup))
            opt.zero_grad()
            g = tb.capture(buf, so, labels, d_jit)

            def replay():
                g.replay()
                opt.step()

            for _ in range(args.rounds):
                rounds['replay_us'].append(per_step_us(torch, dev, replay, args.iters, args.warmup))
            row = {k: float(np.median(v)) for k, v in rounds.items()}
            row['handle_rebuild_us'] = row['host_us'] - row['host_keep_us']
            row['host_over_run'] = row['host_us'] / row['run_us']
            row['host_over_replay'] = row['host_us'] / row['replay_us']
            row['seconds_of_audio'] = float(so[-1]) / rate
            row['rounds'] = rounds
            res['steps'][f'{kind}_B{B}'] = row
            print(f'{kind} B={B}: ' + ', '.join(f'{k}={v:.0f}' for k, v in row.items() if k.endswith('_us')), flush=True)
            del g
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
