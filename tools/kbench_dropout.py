#!/usr/bin/env python3
"""Times the reproducible dropout (csrc/kernels_dropout.h, features/dropout.py) against the torch launches it replaces:

  multipliers  ``dsp_dropout_multipliers`` at [1, 200, B, 400] (enc1 of HRNNHead: 2 H = 400), unbounded and bounded at 90 rows,
               against ``(torch.rand(..) < keep).to(float32) / keep`` -- four launches over all 200 rows;
  apply        ``device_dropout`` (forward, no gradient) at [200, B, 200] (HMRNNHead's encoder output), [200, B, 39] (the
               Transformer head's attention output) and [B, 20] (the logits) against ``F.dropout``;
  steps        one training step -- ``TrainBatch.run`` + ``backward`` + an eager ``torch.optim.Adam`` step, and a graph replay +
               the same Adam step -- of ``HRNNHead`` and ``HMRNNHead`` with every dropout on, each with ``rng=`` and with torch's
               draws.  A recorded step with torch's draws that fails is written down as its error, not worked around.

at B = 32 and 512.  Device events round --iters back-to-back calls after --warmup, the median of --rounds rounds with the spread
(max - min); the arms of a comparison alternate inside each round.  bytes_per_s counts what the algorithm must move: 4 bytes per
multiplier written (the rows behind a bound included: they are stored as zeros), 8 per element applied.  Writes --out (default
profiles/dropout_kbench.json) and prints it as one JSON line.

    python tools/kbench_dropout.py [--iters 50] [--step-iters 10] [--warmup 3] [--rounds 3] [--batches 32,512] [--sections multipliers,apply,steps]
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def event_us(torch, dev, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def compare(torch, dev, arms, iters, warmup, rounds):
    """arms: name -> callable.  -> {name_us, name_spread_us, rounds}: the arms alternate inside each round."""
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            times[name].append(event_us(torch, dev, fn, iters, warmup))
    row = {'rounds': times}
    for name, v in times.items():
        row[name + '_us'] = float(np.median(v))
        row[name + '_spread_us'] = float(max(v) - min(v))
    return row


def verdict(native_us, torch_us):
    return 'ahead' if native_us < torch_us else 'NOT ahead'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--step-iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', default='32,512')
    ap.add_argument('--sections', default='multipliers,apply,steps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dropout_kbench.json'))
    args = ap.parse_args()
    import torch
    from ensemble_cases import make_clips
    from features import _native as nat
    from features.classifier import HMRNNHead, HRNNHead, fill_parameters
    from features.dropout import DeviceRng, device_dropout
    from features.train import TrainBatch
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    batches = [int(v) for v in args.batches.split(',')]
    sections = set(args.sections.split(','))
    rng = DeviceRng(1234, dev)
    res = {'iters': args.iters, 'step_iters': args.step_iters, 'warmup': args.warmup, 'rounds': args.rounds,
           'clock': 'device events round iters back-to-back calls; median of the rounds, spread = max - min', 'multipliers': {}, 'apply': {},
           'steps': {}}

    if 'multipliers' in sections:
        T, C, p = 200, 400, 0.2
        keep = 1.0 - p
        for B in batches:
            rows = torch.tensor([90], dtype=torch.int32, device=dev)
            arms = {'native': lambda: rng.multipliers(1, T, B, C, p, 8), 'native_rows90': lambda: rng.multipliers(1, T, B, C, p, 8, rows),
                    'torch': lambda: (torch.rand(1, T, B, C, device=dev) < keep).to(torch.float32) / keep}
            row = compare(torch, dev, arms, args.iters, args.warmup, args.rounds)
            n = T * B * C
            row['elements'] = n
            for name in ('native', 'native_rows90'):
                row[name + '_bytes_per_s'] = 4 * n / (row[name + '_us'] * 1e-6)
                row[name + '_verdict'] = verdict(row[name + '_us'], row['torch_us'])
            row['native_drawn_per_s'] = n / (row['native_us'] * 1e-6)
            res['multipliers'][f'B{B}'] = row
            print(f'multipliers [1, {T}, {B}, {C}]: ' + ', '.join(f'{k}={v:.1f}' for k, v in row.items() if k.endswith('_us')), flush=True)

    if 'apply' in sections:
        for B in batches:
            for shape in ((200, B, 200), (200, B, 39), (B, 20)):
                p = 0.5 if shape[-1] == 39 else 0.2
                x = torch.randn(*shape, device=dev)
                with torch.no_grad():
                    arms = {'native': lambda: device_dropout(x, p, rng, 0), 'torch': lambda: torch.nn.functional.dropout(x, p)}
                    row = compare(torch, dev, arms, args.iters, args.warmup, args.rounds)
                row['elements'] = x.numel()
                row['native_bytes_per_s'] = 8 * x.numel() / (row['native_us'] * 1e-6)
                row['native_verdict'] = verdict(row['native_us'], row['torch_us'])
                res['apply']['x'.join(str(v) for v in shape)] = row
                print(f'apply {list(shape)} p={p}: ' + ', '.join(f'{k}={v:.1f}' for k, v in row.items() if k.endswith('_us')), flush=True)

    if 'steps' in sections:
        stored, rate = make_clips()
        for name, cls in (('hrnn', HRNNHead), ('hmrnn', HMRNNHead)):
            for B in batches:
                torch.manual_seed(0)
                head = cls().train()
                fill_parameters(head, 3)
                head = head.to(dev)
                opt = torch.optim.Adam(list(head.parameters()), lr=1e-4)
                clips = [stored[i % len(stored)] for i in range(B)]
                so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
                buf = torch.from_numpy(np.concatenate(clips)).to(dev)
                labels = torch.from_numpy(np.random.default_rng(B).integers(0, 20, B).astype(np.int64)).to(dev)
                tb = TrainBatch(rate, head)
                d_jit = torch.from_numpy(tb.draw_jitter(B, random.Random(B))).to(dev)
                kws = {'rng': dict(dropout=True, rng=rng), 'torch': dict(dropout=True)}

                def eager(kw):
                    out = tb.run(buf, so, labels, d_jit, **kw)
                    opt.zero_grad()
                    out.loss.backward()
                    opt.step()

                arms, notes = {'eager_rng': lambda: eager(kws['rng']), 'eager_torch': lambda: eager(kws['torch'])}, {}
                opt.zero_grad()
                graphs = {}
                for which, kw in kws.items():
                    try:
                        graphs[which] = tb.capture(buf, so, labels, d_jit, **kw)
                    except Exception as e:                         # a result to write down, not something to work around here
                        notes[f'replay_{which}'] = f'capture failed: {type(e).__name__}: {str(e)[:300]}'
                        torch.cuda.synchronize(dev)

                def replay(g):
                    g.replay()
                    opt.step()

                for which, g in graphs.items():
                    arms[f'replay_{which}'] = (lambda g=g: replay(g))
                row = compare(torch, dev, arms, args.step_iters, args.warmup, args.rounds)
                for which, g in graphs.items():
                    loss = float(g.replay().loss)
                    notes.setdefault(f'replay_{which}', f'replays; loss after the timed steps {loss:.6g} ({"finite" if np.isfinite(loss) else "NOT finite"})')
                row['notes'] = notes
                row['eager_verdict'] = verdict(row['eager_rng_us'], row['eager_torch_us'])
                if 'replay_rng_us' in row and 'replay_torch_us' in row:
                    row['replay_verdict'] = verdict(row['replay_rng_us'], row['replay_torch_us'])
                res['steps'][f'{name}_B{B}'] = row
                print(f'{name} B={B}: ' + ', '.join(f'{k}={v:.0f}' for k, v in row.items() if k.endswith('_us')) + f' {notes}', flush=True)
                del graphs, arms

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
