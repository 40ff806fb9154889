#!/usr/bin/env python3
"""``dsp_rows_colsum`` (features/wgrad.py: ``rows_colsum``) against the torch expression it replaces, eager and recorded.

    [200, 512, 200]              a.sum(0).sum(0)          (``_rows_sum``)
    [200, 32, 600] of 2 x 800    da[:, :, 1, :600].sum(0).sum(0)   (the strided slice behind the GRU biases)
    [200, 512]                   g_e.sum()                (a [T, B] buffer of scalars)

Device events around ``--inner`` back-to-back calls (eager) or replays of a graph that holds one call (recorded); each cell is
the median of ``--repeats`` such measurements with its spread (max - min), in microseconds per call.  The census of each recorded
graph is kept beside its time: it shows what the torch expression records.  One JSON object on stdout; ``--out FILE`` also writes
it to FILE.  Same process, same device, one cell after the other."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def _time(fn, inner, repeats, torch, dev):
    vals = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        vals.append(a.elapsed_time(b) * 1000.0 / inner)
    return {'median_us': round(statistics.median(vals), 2), 'spread_us': round(max(vals) - min(vals), 2)}


def _recorded(fn, torch, dev):
    from features.graphcheck import census
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    side.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=side):
        keep = fn()
    c = census(graph)
    graph.instantiate()
    return graph, keep, {'kernels': c.kernels, 'memsets': c.memsets, 'wide_memsets': c.wide_memsets,
                         'widest_memset_bytes': c.widest_memset_bytes, 'torch_reductions': len(c.torch_reductions()),
                         'roots': c.roots, 'max_fanout': c.max_fanout}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from features import _native as nat
    from features.wgrad import rows_colsum
    nat.require_device()
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    a = torch.randn(200, 512, 200, generator=g).to(dev)
    da = torch.randn(200, 32, 2, 800, generator=g).to(dev)
    ge = torch.rand(200, 512, generator=g).to(dev)
    sl = da[:, :, 1, :600]
    cells = {
        '[200,512,200] sum(0).sum(0)': (lambda: a.sum(0).sum(0), lambda: rows_colsum(a)),
        '[200,32,600] strided slice sum(0).sum(0)': (lambda: sl.sum(0).sum(0), lambda: rows_colsum(sl)),
        '[200,512] sum()': (lambda: ge.sum().reshape(1), lambda: rows_colsum(ge.unsqueeze(2))),
    }
    out = {'device': torch.cuda.get_device_name(dev), 'inner': args.inner, 'repeats': args.repeats, 'cells': {}}
    for name, (ref, ours) in cells.items():
        want, got = ref().double(), ours().double()
        err = float((got - want).abs().max() / want.abs().max())
        cell = {'rel_diff_to_torch': err}
        for who, fn in (('torch', ref), ('native', ours)):
            for _ in range(5):
                fn()
            cell[f'{who}_eager'] = _time(fn, args.inner, args.repeats, torch, dev)
            graph, keep, c = _recorded(fn, torch, dev)
            cell[f'{who}_recorded'] = dict(_time(graph.replay, args.inner, args.repeats, torch, dev), census=c)
            del graph, keep
        for mode in ('eager', 'recorded'):
            t, n = cell[f'torch_{mode}'], cell[f'native_{mode}']
            gap = t['median_us'] - n['median_us']
            cell[f'{mode}_verdict'] = 'ahead' if gap > max(t['spread_us'], n['spread_us']) else 'NOT ahead'
        out['cells'][name] = cell
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
