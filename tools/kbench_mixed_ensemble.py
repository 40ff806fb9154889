#!/usr/bin/env python3
"""The ensemble over mixed-rate capacity batches, measured (features/ensemble.py: ``MixedRateCapacityEnsembleBatch``;
features/fit.py: ``Trainer`` over the mixed-rate pair) -> profiles/mixed_ensemble_kbench.json.

  epoch     a validation epoch of 8 batches of 44.1 / 48 kHz clips whose lengths AND rate assignments change every batch, through
            ONE mixed capacity ensemble graph -- per batch a device copy of the clips, the offsets, rates and labels into the
            captured buffers and a replay -- against what the parent commit offers for that epoch:
            ``MixedRateEnsembleBatch.run(sync_free=True)`` with its plan per batch.  Both score into a ``Metrics`` block.
  pads      a replay of the mixed graph on a ONE-RATE batch (the other group: B pad clips through the whole pitch tail) against a
            replay of the single-rate ``EnsembleBatch`` capacity graph of the same clips.
  scatter   the two ``dsp_scatter_group_rows_batch`` launches against the ``index_copy_`` pairs they stand in for (two groups).
  fit       one ``Trainer.fit`` epoch (train + validation, ``HMRNNHead``, B = 5, 12 + 7 clips) on mixed data against the loop written
            out: eager ``MixedRateTrainBatch.run(capacity=)`` + ``DeviceAdam.step()``, the eager exact-shape ensemble, NumPy metrics.

Device events round --iters replays, or round the epoch with a host clock beside it (one synchronise at the end); every figure is
the median of --rounds rounds with the spread (max - min), all rounds kept; a cell is "ahead" where the candidate's median is
below the baseline's by more than both spreads together, else "NOT ahead"."""
import argparse
import ctypes
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from kbench_capacity import _brief, _epoch_rows, _event_us, _heads, _offsets, _rules, _stats      # noqa: E402
from kbench_mixed_capacity import TABLE, _epoch_batches, _pool                                     # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'mixed_ensemble_kbench.json')
CASES = (('transformer', 32), ('hmrnn', 512))


def _verdict(cand, base):
    """'ahead' / 'NOT ahead' of two ``_stats`` rows, spreads counted."""
    return 'ahead' if cand['median_us'] + cand['spread_us'] + base['spread_us'] < base['median_us'] else 'NOT ahead'


def _fit_rows(torch, dev, rounds):
    """One epoch of ``Trainer.fit`` on mixed data against the loop written out; host clock, the epoch's one download included."""
    import metrics_emul as me
    from features.ensemble import MixedRateCapacityEnsembleBatch, MixedRateEnsembleBatch
    from features.fit import Trainer
    from features.optim import DeviceAdam
    from features.train import MixedRateTrainBatch
    from golden_cases import make_signal
    B, kw = 5, {'dropout': False}

    def clip(i, seed):
        rate = TABLE[i % 2]
        return make_signal(('vad', seed + i, int((0.5 + 0.06 * (i % 6)) * rate) + 3 * i, rate, 0.6)), rate
    train, val = [clip(i, 1200) for i in range(12)], [clip(i + 1, 1300) for i in range(7)]
    rng = np.random.default_rng(12)
    tlab, vlab = rng.integers(0, 20, 12).astype(np.int64), rng.integers(0, 20, 7).astype(np.int64)
    cap = int(sum(sorted((len(c) for c, _ in train + val), reverse=True)[:B]))

    def trainer_epoch(state={}):
        if not state:
            head = _heads(torch, dev)['hmrnn'](True)
            opt = DeviceAdam(list(head.parameters()), lr=1e-4)
            state['t'] = Trainer(MixedRateTrainBatch(TABLE, head), MixedRateCapacityEnsembleBatch(TABLE, head, []), opt, 20,
                                 wrong_capacity=64, head_kwargs=kw, jitter_rng=random.Random(7))
        state['t'].fit((train, tlab), (val, vlab), 1e-4, epochs=1, batch_size=B, capacity=cap)

    def hand_epoch(state={}):
        if not state:
            head = _heads(torch, dev)['hmrnn'](True)
            state.update(head=head, opt=DeviceAdam(list(head.parameters()), lr=1e-4), tb=MixedRateTrainBatch(TABLE, head),
                         eb=MixedRateEnsembleBatch(head, []), buf=torch.zeros(cap, dtype=torch.int16, device=dev), rng=random.Random(7))
        head, opt, tb, eb, buf = state['head'], state['opt'], state['tb'], state['eb'], state['buf']
        opt.reset()
        opt.set_lr(1e-4)
        head.train()
        order = list(range(12))
        random.Random(0).shuffle(order)
        st = me.State(20, 64)
        for s in range(0, 12, B):
            idx = order[s:s + B]
            clips, rates = [train[i][0] for i in idx], [train[i][1] for i in idx]
            flat = np.concatenate(clips)
            buf[:len(flat)].copy_(torch.from_numpy(flat))
            for p in opt.params:
                p.grad = None
            res = tb.run(buf, _offsets(clips), rates, tlab[idx], tb.draw_jitter(rates, state['rng']), capacity=cap, loss='native', **kw)
            res.loss.backward()
            opt.step()
            st.update(res.logits.detach().cpu().numpy().astype(np.float64), tlab[idx])
        st.result()
        head.eval()
        order = list(range(7))
        random.Random(0).shuffle(order)
        sv = me.State(20, 64)
        with torch.no_grad():
            for s in range(0, 7, B):
                idx = order[s:s + B]
                clips, rates = [val[i][0] for i in idx], [val[i][1] for i in idx]
                res = eb.run(torch.from_numpy(np.concatenate(clips)).to(dev), _offsets(clips), rates, sync_free=True, **kw)
                sv.update(res.logits.cpu().numpy().astype(np.float64), vlab[idx], res.pred.cpu().numpy())
        sv.result()
        head.train()
    routes = {'trainer_fit': trainer_epoch, 'loop_written_out': hand_epoch}
    wall = {k: [] for k in routes}
    for fn in routes.values():
        fn()
    for _ in range(rounds):
        for name, fn in routes.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            wall[name].append((time.perf_counter() - t0) * 1e6)
    row = {name: _stats(v) for name, v in wall.items()}
    row['verdict'] = _verdict(row['trainer_fit'], row['loop_written_out'])
    row['note'] = ('one epoch, 12 training clips (2 full batches of 5 and a partial one of 2) and 7 validation clips; the Trainer records its two '
                   'graphs anew in every epoch of an HMRNNHead (adjust_param), and a fit of ONE epoch includes both recordings')
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--sections', default='epoch,pads,scatter,fit')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    sections = args.sections.split(',')
    import torch
    from features import _native as nat
    from features.ensemble import EnsembleBatch, MixedRateCapacityEnsembleBatch, MixedRateEnsembleBatch
    from features.metrics import Metrics
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    pool, rules, kw = _pool(), _rules(), {'dropout': False}
    res = {'epoch': {}, 'pads': {}, 'scatter': {}, 'fit': {},
           'clock': ('device events round the replays; epoch: device events and a host clock round the 8 batches, one synchronise at the '
                     'end; fit: a host clock round one epoch; median of the rounds, spread = max - min'),
           'not_measured': ['sample types other than int16', 'rate tables of more than two rates',
                            'B other than 32 (TransformerHead) and 512 (HMRNNHead)', 'the optional use_pitch / use_timefeat streams']}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            res.update({k: v for k, v in json.load(fh).items() if k in ('epoch', 'pads', 'scatter', 'fit')})
    for kind, B in CASES:
        tag = f'{kind}_B{B}'
        batches8 = _epoch_batches(pool, B)
        cap = max(sum(len(c) for c in b[0]) for b in batches8)
        head = _heads(torch, dev)[kind](False)
        with torch.no_grad():
            if 'epoch' in sections:
                eb, parent = MixedRateCapacityEnsembleBatch(TABLE, head, rules), MixedRateEnsembleBatch(head, rules)
                staged = []
                for k, (clips, rates) in enumerate(batches8):
                    so = _offsets(clips)
                    staged.append(dict(w=torch.from_numpy(np.concatenate(clips)).to(dev), d_so=torch.from_numpy(so).to(dev), so=so,
                                       d_rates=torch.from_numpy(rates).to(dev), rates=rates,
                                       lab=torch.from_numpy(((np.arange(B) + 7 * k) % 20).astype(np.int64)).to(dev)))
                cbuf = torch.zeros(cap, dtype=torch.int16, device=dev)
                cbuf[:staged[0]['w'].numel()] = staged[0]['w']
                lab = staged[0]['lab'].clone()
                m_g, m_e = Metrics(20, 4096, dev), Metrics(20, 4096, dev)
                g = eb.capture(cbuf, staged[0]['so'], staged[0]['rates'], capacity=cap, labels=lab, metrics=m_g, **kw)

                def through_graph():
                    for s in staged:
                        cbuf[:s['w'].numel()].copy_(s['w'])
                        g.sample_offsets.copy_(s['d_so'])
                        g.rates.copy_(s['d_rates'])
                        lab.copy_(s['lab'])
                        g.replay()

                def through_parent():
                    for s in staged:
                        parent.run(s['w'], s['so'], s['rates'], sync_free=True, labels=s['lab'], metrics=m_e, **kw)
                row = _epoch_rows(torch, dev, {'mixed_capacity_ensemble_graph': through_graph, 'eager_plan_per_batch': through_parent},
                                  args.rounds, cap)
                row['graph_over_eager_wall'] = (row['mixed_capacity_ensemble_graph']['wall']['median_us'] /
                                                row['eager_plan_per_batch']['wall']['median_us'])
                row['verdict'] = _verdict(row['mixed_capacity_ensemble_graph']['wall'], row['eager_plan_per_batch']['wall'])
                res['epoch'][tag] = row
                print(f'epoch {tag}: {json.dumps(_brief(row))} {row["verdict"]}', flush=True)
                assert int(g.status.cpu()[0]) == 0
                del g, staged, through_graph, through_parent
            if 'pads' in sections:
                clips = [pool[48000][(i + 3) % 14][:int((0.60 + 0.05 * ((7 * i) % 9)) * len(pool[48000][0]))] for i in range(B)]
                so, flat = _offsets(clips), np.concatenate(clips)
                total = int(so[-1])
                buf1, buf2 = torch.from_numpy(flat).to(dev), torch.from_numpy(flat).to(dev)
                g1 = EnsembleBatch(48000, head, rules).capture(buf1, so, capacity=total, **kw)
                g2 = MixedRateCapacityEnsembleBatch(TABLE, head, rules).capture(buf2, so, np.full(B, 48000, dtype=np.int32), capacity=total, **kw)
                graphs = {'single_rate_capacity_graph': g1.replay, 'mixed_graph_one_rate': g2.replay}
                times = {name: [] for name in graphs}
                for _ in range(args.rounds):
                    for name, fn in graphs.items():
                        times[name].append(_event_us(torch, dev, fn, args.iters, args.warmup))
                row = {name: _stats(v) for name, v in times.items()}
                row['pads_cost_us'] = row['mixed_graph_one_rate']['median_us'] - row['single_rate_capacity_graph']['median_us']
                row['verdict'] = _verdict(row['mixed_graph_one_rate'], row['single_rate_capacity_graph'])
                row['samples'] = total
                res['pads'][tag] = row
                print(f'pads {tag}: ' + ', '.join(f'{k}={v["median_us"]:.0f} (+-{v["spread_us"]:.0f})' for k, v in row.items() if isinstance(v, dict)) +
                      f' {row["verdict"]}', flush=True)
                del g1, g2, graphs
            if 'scatter' in sections:
                # two groups that interleave: the launches for feat [B, 5] fp64 and aux [B, 9] int32 against index_copy_ on real slots
                lib, st = nat.load(), torch.cuda.current_stream(dev).cuda_stream
                member = np.arange(B) % 2
                cols = [np.full(B, -1, dtype=np.int32) for _ in range(2)]
                for gi in range(2):
                    idx = np.nonzero(member == gi)[0]
                    cols[gi][:len(idx)] = idx
                d_cols = [torch.from_numpy(c).to(dev) for c in cols]
                feat_g = [torch.randn(B, 5, dtype=torch.float64, device=dev) for _ in range(2)]
                aux_g = [torch.randint(0, 100, (B, 9), dtype=torch.int32, device=dev) for _ in range(2)]
                feat, aux = torch.zeros(B, 5, dtype=torch.float64, device=dev), torch.zeros(B, 9, dtype=torch.int32, device=dev)
                VP = ctypes.c_void_p * 2
                p_feat, p_aux, p_col = VP(*[t.data_ptr() for t in feat_g]), VP(*[t.data_ptr() for t in aux_g]), VP(*[t.data_ptr() for t in d_cols])
                pos = [torch.from_numpy(np.nonzero(member == gi)[0].astype(np.int64)).to(dev) for gi in range(2)]

                def scatter():
                    nat.check(lib.dsp_scatter_group_rows_batch(p_feat, p_col, B, 2, 40, feat.data_ptr(), st))
                    nat.check(lib.dsp_scatter_group_rows_batch(p_aux, p_col, B, 2, 36, aux.data_ptr(), st))

                def index_copy():
                    for gi in range(2):
                        n = pos[gi].numel()
                        feat.index_copy_(0, pos[gi], feat_g[gi][:n])
                        aux.index_copy_(0, pos[gi], aux_g[gi][:n])
                scatter()
                a = (feat.clone(), aux.clone())
                index_copy()
                assert torch.equal(a[0], feat) and torch.equal(a[1], aux)
                times = {'scatter_two_launches': [], 'index_copy_four_launches': []}
                for _ in range(args.rounds):
                    times['scatter_two_launches'].append(_event_us(torch, dev, scatter, 10 * args.iters, args.warmup))
                    times['index_copy_four_launches'].append(_event_us(torch, dev, index_copy, 10 * args.iters, args.warmup))
                row = {name: _stats(v) for name, v in times.items()}
                row['verdict'] = _verdict(row['scatter_two_launches'], row['index_copy_four_launches'])
                row['note'] = 'eager launches, host-bound at this size: the figure is launch overhead, not kernel time'
                res['scatter'][tag] = row
                print(f'scatter {tag}: ' + ', '.join(f'{k}={v["median_us"]:.1f} (+-{v["spread_us"]:.1f})' for k, v in row.items() if isinstance(v, dict)) +
                      f' {row["verdict"]}', flush=True)
    if 'fit' in sections:
        res['fit']['hmrnn_B5'] = _fit_rows(torch, dev, args.rounds)
        r = res['fit']['hmrnn_B5']
        print(f'fit: trainer {r["trainer_fit"]["median_us"] / 1e3:.1f} ms (+-{r["trainer_fit"]["spread_us"] / 1e3:.1f}), loop written out '
              f'{r["loop_written_out"]["median_us"] / 1e3:.1f} ms (+-{r["loop_written_out"]["spread_us"] / 1e3:.1f}) {r["verdict"]}', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
