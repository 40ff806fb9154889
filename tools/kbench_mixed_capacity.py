#!/usr/bin/env python3
"""Mixed-rate batches through one recorded step, measured (features/train.py: ``MixedRateTrainBatch``) ->
profiles/mixed_capacity_kbench.json.

  epoch     8 batches of 44.1 / 48 kHz clips whose lengths AND rate assignments change every batch, through ONE mixed capacity
            graph -- per batch a device copy of the clips, the offsets, rates, labels and jitter into the captured buffers and a
            replay -- against what the parent commit offers for that epoch: ``MixedRateFeatureBatch.run`` with its plan per batch
            (group_by_rate, a pipeline layout and its uploads per group, the synchronise of the results), then the head with the
            lengths on the device, the loss, the backward and ``DeviceAdam.step()``, eager.
  grouping  a replay of the mixed capacity graph against a replay of the single-rate capacity graph (``TrainBatch``) on ONE-RATE
            batches of the same clips: what the grouping launch, the gather, the endpoint scatter and a whole group of pad clips
            cost; and the mixed graph on the same clips with the rates interleaved (two real groups).

Device events round --iters replays (grouping) or round the epoch with a host clock beside it (one synchronise at the end);
every figure is the median of --rounds rounds with the spread (max - min), all rounds kept."""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from kbench_capacity import _brief, _epoch_rows, _event_us, _heads, _offsets, _stats      # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'mixed_capacity_kbench.json')
TABLE = (44100, 48000)
CASES = (('transformer', 32), ('hmrnn', 512))


def _pool():
    """28 stored clips of 0.9 s, 14 per rate (tests/golden_cases.py: an int16 background and one voiced burst)."""
    from golden_cases import make_signal
    return {r: [make_signal(('vad', 3000 + 20 * j + i, int(0.9 * r), r, 0.6)) for i in range(14)] for j, r in enumerate(TABLE)}


def _epoch_batches(pool, B, n=8):
    """n batches of B clips; batch k has its own rate assignment and its own length vector (prefixes of 60 - 100 % of the stored
    clips, 0.54 - 0.9 s)."""
    out = []
    for k in range(n):
        rng = np.random.default_rng(50 * B + k)
        rates = np.array([TABLE[int(i)] for i in rng.integers(0, 2, B)], dtype=np.int32)
        clips = []
        for i, r in enumerate(rates.tolist()):
            c = pool[r][(i + 3 * k) % 14]
            clips.append(c[:int((0.60 + 0.05 * ((7 * i + 3 * k) % 9)) * len(c)) + k])
        out.append((clips, rates))
    return out


def _logits_of(out):
    return out[0] if isinstance(out, (tuple, list)) else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    import torch
    from features import _native as nat
    from features.model_glue import MixedRateFeatureBatch
    from features.optim import DeviceAdam
    from features.train import MixedRateTrainBatch, TrainBatch
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    pool = _pool()
    kw = {'dropout': False}
    res = {'epoch': {}, 'grouping': {},
           'clock': ('device events round the replays; epoch: device events and a host clock round the 8 batches, one synchronise at the '
                     'end; median of the rounds, spread = max - min'),
           'not_measured': ['the ensemble over mixed-rate capacity batches (out of scope)', 'sample types other than int16',
                            'rate tables of more than two rates', 'B other than 32 (TransformerHead) and 512 (HMRNNHead)']}
    for kind, B in CASES:
        tag = f'{kind}_B{B}'
        batches8 = _epoch_batches(pool, B)
        cap = max(sum(len(c) for c in b[0]) for b in batches8)
        head_g, head_e = _heads(torch, dev)[kind](True), _heads(torch, dev)[kind](True)
        tb = MixedRateTrainBatch(TABLE, head_g)
        staged = []
        for k, (clips, rates) in enumerate(batches8):
            so, jit = _offsets(clips), tb.draw_jitter(rates, random.Random(B + k))
            staged.append(dict(w=torch.from_numpy(np.concatenate(clips)).to(dev), d_so=torch.from_numpy(so).to(dev), so=so,
                               d_rates=torch.from_numpy(rates).to(dev), rates=rates, jit=jit, d_jit=torch.from_numpy(jit).to(dev),
                               lab=torch.from_numpy(((np.arange(B) + 7 * k) % 20).astype(np.int64)).to(dev)))
        cbuf = torch.zeros(cap, dtype=torch.int16, device=dev)
        cbuf[:staged[0]['w'].numel()] = staged[0]['w']
        lab = staged[0]['lab'].clone()
        opt_g = DeviceAdam(list(head_g.parameters()), lr=1e-4)
        opt_e = DeviceAdam(list(head_e.parameters()), lr=1e-4)
        g = tb.capture(cbuf, staged[0]['so'], staged[0]['rates'], lab, staged[0]['d_jit'].clone(), optimizer=opt_g, capacity=cap, **kw)
        parent = MixedRateFeatureBatch()

        def through_graph():
            for s in staged:
                cbuf[:s['w'].numel()].copy_(s['w'])
                g.sample_offsets.copy_(s['d_so'])
                g.rates.copy_(s['d_rates'])
                lab.copy_(s['lab'])
                g.jitter.copy_(s['d_jit'])
                g.replay()

        def through_parent():
            for s in staged:
                for p in opt_e.params:
                    p.grad = None
                inp, len0, _ = parent.run(s['w'], s['so'], s['rates'], jitter=s['jit'])
                d_len = torch.from_numpy(np.asarray(len0, dtype=np.int32)).to(dev)
                logits = _logits_of(head_e(inp, d_len, device_len=True, device_grad=True, **kw))
                torch.nn.functional.cross_entropy(logits, s['lab']).backward()
                opt_e.step()
        row = _epoch_rows(torch, dev, {'mixed_capacity_graph': through_graph, 'eager_plan_per_batch': through_parent}, args.rounds, cap)
        row['graph_over_eager_wall'] = row['mixed_capacity_graph']['wall']['median_us'] / row['eager_plan_per_batch']['wall']['median_us']
        res['epoch'][tag] = row
        print(f'epoch {tag}: {json.dumps(_brief(row))}', flush=True)
        assert int(g.status.cpu()[0]) == 0
        del g, staged, through_graph, through_parent

        # ---- the cost of the grouping, the gather and the pads: one-rate batches of the same clips ----
        clips, _ = batches8[0]
        so, flat = _offsets(clips), np.concatenate(clips)
        total = int(so[-1])
        labels = torch.from_numpy(np.random.default_rng(B).integers(0, 20, B).astype(np.int64)).to(dev)
        keep, graphs = [], {}
        for name in ('single_rate_capacity', 'mixed_one_rate', 'mixed_interleaved'):
            head = _heads(torch, dev)[kind](True)         # every graph trains its own copy: the recorded Adam step writes the parameters
            opt = DeviceAdam(list(head.parameters()), lr=1e-4)
            buf = torch.from_numpy(flat).to(dev)
            if name == 'single_rate_capacity':
                t1 = TrainBatch(48000, head)
                jit = torch.from_numpy(t1.draw_jitter(B, random.Random(B))).to(dev)
                gr = t1.capture(buf, so, labels, jit, optimizer=opt, capacity=total, **kw)
            else:
                t2 = MixedRateTrainBatch(TABLE, head)
                rates = np.full(B, 48000, dtype=np.int32) if name == 'mixed_one_rate' else np.array([TABLE[i % 2] for i in range(B)], dtype=np.int32)
                jit = torch.from_numpy(t2.draw_jitter(rates, random.Random(B))).to(dev)
                gr = t2.capture(buf, so, rates, labels, jit, optimizer=opt, capacity=total, **kw)
            keep.append((head, opt, buf, jit, gr))
            graphs[name] = gr.replay
        times = {name: [] for name in graphs}
        for _ in range(args.rounds):
            for name, fn in graphs.items():
                times[name].append(_event_us(torch, dev, fn, args.iters, args.warmup))
        row = {name: _stats(v) for name, v in times.items()}
        for name in ('mixed_one_rate', 'mixed_interleaved'):
            row[name]['minus_single_rate_us'] = row[name]['median_us'] - row['single_rate_capacity']['median_us']
        row['samples'] = total
        res['grouping'][tag] = row
        print(f'grouping {tag}: ' + ', '.join(f'{k}={v["median_us"]:.0f} (+-{v["spread_us"]:.0f})' for k, v in row.items() if isinstance(v, dict)),
              flush=True)
        del keep, graphs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
