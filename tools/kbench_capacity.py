#!/usr/bin/env python3
"""The capacity layout measured (features/pipeline.py: ``CapacityLayout``); the sections ``tools/kbench_train.py --routes capacity``
and ``tools/kbench_ensemble.py --capacity`` run and merge into profiles/capacity_layout_kbench.json.

  padding   a replay of the graph recorded with ``capacity=`` (1.0 x, 1.25 x and 2 x the batch's samples) against a replay of the
            exact-shape graph on the same clips: ``EnsembleBatch`` and ``TrainBatch`` (the whole step, ``DeviceAdam`` inside), each
            with ``HMRNNHead`` and ``TransformerHead``, B = 32 and 512.  At 1.0 x the difference is the two added launches
            (dsp_batch_offsets_batch, dsp_layout_refresh) and the grids sized by the bound instead of the true frame count.
  epoch     8 batches with 8 different length vectors (prefixes of the stored clips) through ONE capacity graph -- per batch a
            device copy of the clips, the offsets (and labels, jitter) into the captured buffers and a replay -- against the
            route without it: the eager sync-free ``run`` on the exact layout of every batch, which has to be built per length
            vector (the classes keep four; eight vectors in turn never hit).

Device events round --iters replays (padding) or round the epoch, host clock beside it for the epoch (one synchronise at the
end); every figure is the median of --rounds rounds with the spread (max - min), all rounds kept."""
import json
import os
import random
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'profiles', 'capacity_layout_kbench.json')
FACTORS = (1.0, 1.25, 2.0)


def _event_us(torch, dev, fn, iters, warmup):
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


def _stats(v):
    return {'median_us': float(np.median(v)), 'spread_us': float(max(v) - min(v)), 'rounds': [float(x) for x in v]}


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


def _epoch_batches(stored, B, n=8):
    """n batches of B clips, every one with its own length vector: prefixes between 60 % and 100 % of the stored clips."""
    out = []
    for k in range(n):
        clips = []
        for i in range(B):
            c = stored[(i + 3 * k) % len(stored)]
            clips.append(c[:int((0.60 + 0.05 * ((7 * i + 3 * k) % 9)) * len(c)) + k])
        out.append(clips)
    return out


def merge(section, rows, out=OUT):
    """Read-modify-write of the JSON: ``section`` ('ensemble' or 'train') is replaced, the other kept."""
    res = {}
    if os.path.exists(out):
        with open(out) as fh:
            res = json.load(fh)
    res[section] = rows
    res['clock'] = ('device events round the replays; epoch: device events and a host clock round the 8 batches, one synchronise at '
                    'the end; median of the rounds, spread = max - min')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    return res


def _heads(torch, dev):
    from features.classifier import HMRNNHead, TransformerHead, fill_parameters

    def make(cls, train):
        torch.manual_seed(0)
        head = cls()
        head = head.train() if train else head.eval()
        fill_parameters(head, 3)
        return head.to(dev)
    return {'hmrnn': lambda train: make(HMRNNHead, train), 'transformer': lambda train: make(TransformerHead, train)}


def _rules():
    from ensemble_cases import PAIRS, THRESHOLDS
    from features.ensemble import PitchSVM
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ensemble_golden.npz')) as z:
        models = [{k: z[f'svm{p[0]}{p[1]}/{k}'] for k in ('scale', 'support_vectors', 'dual_coef', 'intercept', 'gamma', 'classes')}
                  for p in PAIRS]
    return [(p, t, PitchSVM.from_arrays(m['support_vectors'], m['dual_coef'], m['intercept'], m['gamma'], m['classes'], scale=m['scale']))
            for p, t, m in zip(PAIRS, THRESHOLDS, models)]


def _padding_rows(torch, dev, graphs, iters, warmup, rounds):
    """graphs: name -> replay callable, 'exact' among them; timed in turn in every round."""
    times = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, fn in graphs.items():
            times[name].append(_event_us(torch, dev, fn, iters, warmup))
    row = {name: _stats(v) for name, v in times.items()}
    for name in graphs:
        if name != 'exact':
            row[name]['minus_exact_us'] = row[name]['median_us'] - row['exact']['median_us']
    return row


def ensemble_section(batches=(32, 512), heads=('hmrnn', 'transformer'), iters=20, warmup=3, rounds=3, epoch=True):
    import torch
    from ensemble_cases import make_clips
    from features import _native as nat
    from features.ensemble import EnsembleBatch
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    stored, rate = make_clips()
    rules = _rules()
    res = {'padding': {}, 'epoch': {}}
    with torch.no_grad():
        for kind in heads:
            head = _heads(torch, dev)[kind](False)
            for B in batches:
                eb = EnsembleBatch(rate, head, rules)
                clips = [stored[i % len(stored)] for i in range(B)]
                so, flat = _offsets(clips), np.concatenate(clips)
                total = int(so[-1])
                keep, graphs = [], {}
                buf = torch.from_numpy(flat).to(dev)
                g = eb.capture(buf, so, dropout=False)
                keep.append((buf, g))
                graphs['exact'] = g.replay
                for f in FACTORS:
                    cap = int(f * total)
                    cbuf = torch.zeros(cap, dtype=torch.int16, device=dev)
                    cbuf[:total] = buf
                    gc = eb.capture(cbuf, so, capacity=cap, dropout=False)
                    keep.append((cbuf, gc))
                    graphs[f'capacity_{f}x'] = gc.replay
                row = _padding_rows(torch, dev, graphs, iters, warmup, rounds)
                row['samples'] = total
                res['padding'][f'{kind}_B{B}'] = row
                print(f'ensemble padding {kind} B={B}: ' + ', '.join(f'{k}={v["median_us"]:.0f} (+-{v["spread_us"]:.0f})' for k, v in row.items()
                                                                         if isinstance(v, dict)), flush=True)
                del keep, graphs
                if not epoch:
                    continue
                batches8 = _epoch_batches(stored, B)
                cap = max(sum(len(c) for c in b) for b in batches8)
                staged = [(torch.from_numpy(np.concatenate(b)).to(dev), torch.from_numpy(_offsets(b)).to(dev), _offsets(b)) for b in batches8]
                cbuf = torch.zeros(cap, dtype=torch.int16, device=dev)
                cbuf[:staged[0][0].numel()] = staged[0][0]
                gc = eb.capture(cbuf, staged[0][2], capacity=cap, dropout=False)
                eager = EnsembleBatch(rate, head, rules)

                def through_graph():
                    for w, d_so, _ in staged:
                        cbuf[:w.numel()].copy_(w)
                        gc.sample_offsets.copy_(d_so)
                        gc.replay()

                def through_eager():
                    for w, _, so_h in staged:
                        eager.run(w, so_h, sync_free=True, dropout=False)
                res['epoch'][f'{kind}_B{B}'] = _epoch_rows(torch, dev, {'capacity_graph': through_graph, 'eager_fresh_layouts': through_eager},
                                                           rounds, cap)
                print(f'ensemble epoch {kind} B={B}: {json.dumps(_brief(res["epoch"][f"{kind}_B{B}"]))}', flush=True)
                del gc, staged
    return res


def _epoch_rows(torch, dev, routes, rounds, cap):
    ev, wall = {k: [] for k in routes}, {k: [] for k in routes}
    for fn in routes.values():          # one untimed epoch each: handles, arenas, the allocator's blocks
        fn()
    torch.cuda.synchronize(dev)
    for _ in range(rounds):
        for name, fn in routes.items():
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            wall[name].append((time.perf_counter() - t0) * 1e6)
            ev[name].append(e0.elapsed_time(e1) * 1e3)
    row = {name: {'event': _stats(ev[name]), 'wall': _stats(wall[name])} for name in routes}
    row['batches'], row['capacity_samples'] = 8, int(cap)
    return row


def _brief(row):
    return {k: {'event_us': round(v['event']['median_us']), 'wall_us': round(v['wall']['median_us']), 'wall_spread_us': round(v['wall']['spread_us'])}
            for k, v in row.items() if isinstance(v, dict)}


def train_section(batches=(32, 512), heads=('hmrnn', 'transformer'), iters=20, warmup=3, rounds=3, epoch=True):
    import torch
    from ensemble_cases import make_clips
    from features import _native as nat
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    stored, rate = make_clips()
    res = {'padding': {}, 'epoch': {}}
    for kind in heads:
        for B in batches:
            clips = [stored[i % len(stored)] for i in range(B)]
            so, flat = _offsets(clips), np.concatenate(clips)
            total = int(so[-1])
            labels = torch.from_numpy(np.random.default_rng(B).integers(0, 20, B).astype(np.int64)).to(dev)
            keep, graphs = [], {}
            # every graph trains its own copy of the head: the recorded Adam step writes the parameters
            for name, cap in [('exact', None)] + [(f'capacity_{f}x', int(f * total)) for f in FACTORS]:
                head = _heads(torch, dev)[kind](True)
                tb = TrainBatch(rate, head)
                jit = torch.from_numpy(tb.draw_jitter(B, random.Random(B))).to(dev)
                buf = torch.zeros(total if cap is None else cap, dtype=torch.int16, device=dev)
                buf[:total] = torch.from_numpy(flat).to(dev)
                opt = DeviceAdam(list(head.parameters()), lr=1e-4)
                g = tb.capture(buf, so, labels, jit, optimizer=opt, **({} if cap is None else {'capacity': cap}))
                keep.append((head, tb, jit, buf, opt, g))
                graphs[name] = g.replay
            row = _padding_rows(torch, dev, graphs, iters, warmup, rounds)
            row['samples'] = total
            res['padding'][f'{kind}_B{B}'] = row
            print(f'train padding {kind} B={B}: ' + ', '.join(f'{k}={v["median_us"]:.0f} (+-{v["spread_us"]:.0f})' for k, v in row.items()
                                                                  if isinstance(v, dict)), flush=True)
            del keep, graphs
            if not epoch:
                continue
            batches8 = _epoch_batches(stored, B)
            cap = max(sum(len(c) for c in b) for b in batches8)
            head_g, head_e = _heads(torch, dev)[kind](True), _heads(torch, dev)[kind](True)
            tb_g, tb_e = TrainBatch(rate, head_g), TrainBatch(rate, head_e)
            staged = [(torch.from_numpy(np.concatenate(b)).to(dev), torch.from_numpy(_offsets(b)).to(dev), _offsets(b),
                       torch.from_numpy(((np.arange(B) + 7 * k) % 20).astype(np.int64)).to(dev),
                       torch.from_numpy(tb_g.draw_jitter(B, random.Random(B + k))).to(dev)) for k, b in enumerate(batches8)]
            cbuf = torch.zeros(cap, dtype=torch.int16, device=dev)
            cbuf[:staged[0][0].numel()] = staged[0][0]
            lab, jit = staged[0][3].clone(), staged[0][4].clone()
            opt_g = DeviceAdam(list(head_g.parameters()), lr=1e-4)
            opt_e = DeviceAdam(list(head_e.parameters()), lr=1e-4)
            gc = tb_g.capture(cbuf, staged[0][2], lab, jit, optimizer=opt_g, capacity=cap)

            def through_graph():
                for w, d_so, _, l, j in staged:
                    cbuf[:w.numel()].copy_(w)
                    gc.sample_offsets.copy_(d_so)
                    lab.copy_(l)
                    jit.copy_(j)
                    gc.replay()

            def through_eager():
                for w, _, so_h, l, j in staged:
                    for p in opt_e.params:
                        p.grad = None
                    out = tb_e.run(w, so_h, l, j)
                    out.loss.backward()
                    opt_e.step()
            res['epoch'][f'{kind}_B{B}'] = _epoch_rows(torch, dev, {'capacity_graph': through_graph, 'eager_fresh_layouts': through_eager},
                                                       rounds, cap)
            print(f'train epoch {kind} B={B}: {json.dumps(_brief(res["epoch"][f"{kind}_B{B}"]))}', flush=True)
            del gc, staged
    return res
