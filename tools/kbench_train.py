#!/usr/bin/env python3
"""Times one training step -- front end on raw clips with the endpoint jitter, head, cross-entropy, backward, an eager Adam
step -- of ``HMRNNHead`` and ``TransformerHead`` (seeded weights, training mode, both F.dropout calls on) three ways:

  (1) host     the route with the lengths on the host and every native flag on: ``ModelFeatureBatch.run`` downloads len0 (one
               synchronisation), the head runs with ``native=True / native_enc=True / native_attn=True``, and every step
               rebuilds the native handles because the optimiser wrote the parameters;
      host_keep  the same step with the optimiser working on a shadow copy of the parameters, so that the handles stay:
               (1) minus this is what the handle re-creation costs;
  (2) run      ``TrainBatch.run`` + ``backward``: lengths on the device, handles repacked in place, nothing synchronised;
  (3) replay   ``TrainBatch.capture(...).replay()``: refresh, front end, forward, loss and backward as ONE HIP graph, the eager
               Adam step behind it;
  (4) replay_adam  ``TrainBatch.capture(..., optimizer=DeviceAdam(...)).replay()``: the same graph with the native Adam step
               (csrc/kernels_optim.h) recorded behind the backward -- the whole step is one replay
  (5) run_wgrad / replay_wgrad  routes (2) and (3) with ``native_wgrad=True``: the products behind the GRU and HM-LSTM backward
               recurrences as native launches bounded by the row count on the device (csrc/kernels_wgrad.h) instead of torch's
               GEMMs, sums and ``cat`` copies over all 200 rows; timed in the same rounds as their plain twins

  (7) native_sums  (``--routes native_sums`` alone; not among the defaults) the whole recorded step with ``native_sums=True`` against
      the default device route, both with their graph census (``native_sums_section``).
  (6) capacity  (``--routes capacity`` alone; not among the defaults) the recorded step with ``capacity=`` against the exact-shape
               graph, and an epoch of 8 length vectors through ONE capacity graph against the eager route: tools/kbench_capacity.py,
               merged into profiles/capacity_layout_kbench.json

at B = 32 (the reference's cfg.batch_size) and B = 512, on the stored 16 kHz chirps of tests/ensemble_cases.py, repeated.

The host route takes the jitter as a host array and uploads it on every step (16 bytes per clip, pageable memory), which is
what that route does in a training loop; the device routes read a jitter already on the device.  ``capture`` serves the head / size
pairs of ``features.train.CAPTURE_VERIFIED``, which hold the defaults here.

Routes (3) and (4) are also timed with device events round the same --iters steps (``*_event_us``).  The ``adam`` section times
the optimiser step ALONE on each head's parameter list with random gradients, device events round --adam-iters back-to-back
steps: ``DeviceAdam.step()`` against ``torch.optim.Adam.step()`` in its default, ``foreach=False`` and ``fused=True`` forms, the
median of --rounds rounds with the spread (max - min), and the bytes per second ``DeviceAdam`` moves (28 bytes per parameter:
p, m, v read and written, g read); ``device_adam_graph`` is the native step per step of 20 recorded as one graph, i.e. its two
launches without the host side of ``step()``.

Every other figure is a host clock around --iters back-to-back steps that end in a device synchronise, divided by --iters, after
--warmup steps; the routes are timed one after the other in each of --rounds rounds and the median round is reported (all
rounds are kept in the JSON).  Writes --out (default profiles/train_kbench.json) and prints it as one JSON line.

    python tools/kbench_train.py [--iters 20] [--warmup 3] [--rounds 3] [--batches 32,512] [--heads hmrnn,transformer]
                                 [--routes host,host_keep,run,run_wgrad,replay,replay_wgrad,replay_adam,adam]
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


def per_step_event_us(torch, dev, fn, iters, warmup):
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


def adam_alone(torch, dev, head, iters, warmup, rounds):
    """The optimiser step alone on the head's parameter list, each optimiser on its own copy, random gradients."""
    from features.optim import DeviceAdam
    gen = torch.Generator(device='cpu').manual_seed(7)
    base = [p.detach().clone() for p in head.parameters() if p.requires_grad]
    grads = [(1e-2 * torch.randn(p.shape, generator=gen)).to(dev) for p in base]
    makers = {'device_adam': lambda ps: DeviceAdam(ps, lr=1e-4), 'torch_default': lambda ps: torch.optim.Adam(ps, lr=1e-4),
              'torch_foreach_false': lambda ps: torch.optim.Adam(ps, lr=1e-4, foreach=False),
              'torch_fused': lambda ps: torch.optim.Adam(ps, lr=1e-4, fused=True)}
    opts = {}
    for name, make in makers.items():
        ps = [p.clone().requires_grad_(True) for p in base]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opts[name] = make(ps)
    times = {name: [] for name in makers}
    for _ in range(rounds):
        for name, opt in opts.items():
            times[name].append(per_step_event_us(torch, dev, opt.step, iters, warmup))
    # ... and 20 native steps recorded as one graph: the two launches of a step without the host side of step()
    dopt = opts['device_adam']
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(20):
            dopt._launch([p.grad for p in dopt.params], False)
    times['device_adam_graph'] = [per_step_event_us(torch, dev, graph.replay, max(iters // 20, 1), warmup) / 20 for _ in range(rounds)]
    n = sum(p.numel() for p in base)
    row = {'tensors': len(base), 'parameters': n, 'bytes_per_step': 28 * n, 'rounds': times}
    for name, v in times.items():
        row[name + '_us'] = float(np.median(v))
        row[name + '_spread_us'] = float(max(v) - min(v))
    row['device_adam_bytes_per_s'] = 28 * n / (row['device_adam_us'] * 1e-6)
    row['device_adam_graph_bytes_per_s'] = 28 * n / (row['device_adam_graph_us'] * 1e-6)
    return row


def native_sums_section(torch, dev, stored, rate, args):
    """``--routes native_sums`` (alone; not among the defaults): the whole recorded step -- ``DeviceAdam`` inside, ``loss='native'``,
    dropout off -- on the device route as it is by default against the same step with ``native_sums=True``, at the sizes of
    ``CAPTURE_VERIFIED`` so that both record; device events, the median of --rounds rounds with the spread.  Both graphs are recorded
    with ``census=True``: the default route's census shows how many memset nodes and reductions of torch's the verified graphs
    carry.  -> the section, also written to ``--out``."""
    from features.classifier import HMRNNHead, TransformerHead, fill_parameters
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    kinds = {'hmrnn': HMRNNHead, 'transformer': TransformerHead}
    res = {'iters': args.iters, 'warmup': args.warmup, 'rounds': args.rounds, 'clock': 'device events around iters replays', 'steps': {}}
    brief = lambda c: {'kernels': c.kernels, 'memsets': c.memsets, 'wide_memsets': c.wide_memsets, 'widest_memset_bytes': c.widest_memset_bytes,
                       'memcpys': c.memcpys, 'torch_reductions': len(c.torch_reductions()), 'roots': c.roots, 'max_fanout': c.max_fanout}
    for kind in args.heads.split(','):
        for B in (int(v) for v in args.batches.split(',')):
            clips = [stored[i % len(stored)] for i in range(B)]
            so = np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)
            buf = torch.from_numpy(np.concatenate(clips)).to(dev)
            labels = torch.from_numpy(np.random.default_rng(B).integers(0, 20, B).astype(np.int64)).to(dev)
            graphs, row = {}, {}
            for name, kw in (('default', {}), ('native_sums', {'native_sums': True})):
                torch.manual_seed(0)
                head = kinds[kind]().train()
                fill_parameters(head, 3)
                head = head.to(dev)
                tb = TrainBatch(rate, head)
                d_jit = torch.from_numpy(tb.draw_jitter(B, random.Random(B))).to(dev)
                graphs[name] = tb.capture(buf, so, labels, d_jit, optimizer=DeviceAdam(list(head.parameters()), lr=1e-4), loss='native',
                                          census=True, dropout=False, **kw)
                row[f'{name}_census'] = brief(graphs[name].census)
            rounds = {}
            for _ in range(args.rounds):
                for name, g in graphs.items():
                    rounds.setdefault(name, []).append(per_step_event_us(torch, dev, g.replay, args.iters, args.warmup))
            for name, v in rounds.items():
                row[f'{name}_event_us'], row[f'{name}_spread_us'] = float(np.median(v)), float(max(v) - min(v))
            gap = row['default_event_us'] - row['native_sums_event_us']
            row['verdict'] = 'ahead' if gap > max(row['default_spread_us'], row['native_sums_spread_us']) else 'NOT ahead'
            res['steps'][f'{kind}_B{B}'] = row
            print(f'{kind} B={B}: default {row["default_event_us"]:.0f} us, native_sums {row["native_sums_event_us"]:.0f} us: {row["verdict"]}', flush=True)
            del graphs
    res['epoch_B48'] = epoch_section(torch, dev, stored, rate, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    return res


def epoch_section(torch, dev, stored, rate, args):
    """An epoch of 8 batches at batch size 48 -- a size outside ``CAPTURE_VERIFIED`` -- through ``Trainer.fit``: with
    ``native_sums=True`` (one recorded capacity graph) against the eager ``run(capacity=)`` fallback that size gets without it.  Host
    clock around ``fit`` of one epoch, a first (recording) epoch left out; the median of --rounds epochs and the spread, in ms."""
    from features.classifier import TransformerHead, fill_parameters
    from features.ensemble import EnsembleBatch
    from features.fit import Trainer
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    B, N = 48, 8 * 48
    clips = [stored[i % len(stored)] for i in range(N)]
    labels = np.random.default_rng(48).integers(0, 20, N).astype(np.int64)
    feat = [(c, rate) for c in clips]
    val = ([(c, rate) for c in clips[:B]], labels[:B])
    out = {}
    for name, sums in (('eager_fallback', False), ('native_sums_graph', True)):
        torch.manual_seed(0)
        head = TransformerHead().train()
        fill_parameters(head, 3)
        head = head.to(dev)
        trainer = Trainer(TrainBatch(rate, head), EnsembleBatch(rate, head, []), DeviceAdam(list(head.parameters()), lr=1e-4), 20,
                          head_kwargs={'dropout': False}, jitter_rng=random.Random(7))
        times = []

        def on_epoch(entry):
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter())
        torch.cuda.synchronize(dev)
        times.append(time.perf_counter())
        trainer.fit((feat, labels), val, 1e-4, epochs=args.rounds + 1, early_stop=args.rounds + 2, batch_size=B, on_epoch=on_epoch, native_sums=sums)
        ms = [1e3 * (b - a) for a, b in zip(times[1:-1], times[2:])]        # (the first epoch records / warms up)
        out[f'{name}_ms'], out[f'{name}_spread_ms'] = float(np.median(ms)), float(max(ms) - min(ms))
        out[f'{name}_train_graphs'] = trainer.train_graphs
    gap = out['eager_fallback_ms'] - out['native_sums_graph_ms']
    out['verdict'] = 'ahead' if gap > max(out['eager_fallback_spread_ms'], out['native_sums_graph_spread_ms']) else 'NOT ahead'
    out['note'] = 'TransformerHead, 8 batches of 48 stored clips and one validation batch per epoch'
    print(f"epoch at B=48: eager fallback {out['eager_fallback_ms']:.1f} ms, native_sums graph {out['native_sums_graph_ms']:.1f} ms: {out['verdict']}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--adam-iters', type=int, default=200)
    ap.add_argument('--batches', default='32,512')
    ap.add_argument('--heads', default='hmrnn,transformer')
    ap.add_argument('--routes', default='host,host_keep,run,run_wgrad,replay,replay_wgrad,replay_adam,adam',
                    help='the routes to time (the others stay out of the JSON)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_kbench.json'))
    args = ap.parse_args()
    import torch
    from ensemble_cases import make_clips
    from features import _native as nat
    from features.classifier import HMRNNHead, TransformerHead, fill_parameters
    from features.model_glue import ModelFeatureBatch
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    stored, rate = make_clips()
    routes = set(args.routes.split(','))
    if 'capacity' in routes:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        import kbench_capacity
        rows = kbench_capacity.train_section(tuple(int(v) for v in args.batches.split(',')), tuple(args.heads.split(',')), args.iters,
                                             args.warmup, args.rounds)
        print(json.dumps({'train': kbench_capacity.merge('train', rows)['train']}))
        return
    if 'native_sums' in routes:
        print(json.dumps(native_sums_section(torch, dev, stored, rate, args), indent=1))
        return
    kinds = {'hmrnn': (HMRNNHead, dict(native=True, native_enc=True)), 'transformer': (TransformerHead, dict(native_enc=True, native_attn=True))}
    res = {'iters': args.iters, 'warmup': args.warmup, 'rounds': args.rounds, 'optimizer': 'torch.optim.Adam(lr=1e-4), eager',
           'clock': 'host clock around iters steps ending in a device synchronise; *_event_us and the adam section: device events',
           'adam': {}, 'steps': {}}
    for kind in args.heads.split(','):
        cls, host_kw = kinds[kind]
        torch.manual_seed(0)
        if 'adam' in routes:
            row = adam_alone(torch, dev, cls().to(dev), args.adam_iters, args.warmup, args.rounds)
            res['adam'][kind] = row
            print(f'{kind} Adam alone ({row["tensors"]} tensors, {row["parameters"]} parameters): '
                  + ', '.join(f'{k}={v:.1f}' for k, v in row.items() if k.endswith('_us')) + f', {row["device_adam_bytes_per_s"] / 1e12:.2f} TB/s eager, {row["device_adam_graph_bytes_per_s"] / 1e12:.2f} TB/s recorded', flush=True)
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

            def run(**kw):
                out = tb.run(buf, so, labels, d_jit, **kw)
                opt.zero_grad()
                out.loss.backward()
                opt.step()

            rounds = {}
            timed = lambda name, clock, fn: rounds.setdefault(name, []).append(clock(torch, dev, fn, args.iters, args.warmup))
            for _ in range(args.rounds):
                if 'host' in routes: timed('host_us', per_step_us, host)
                if 'host_keep' in routes: timed('host_keep_us', per_step_us, lambda: host(True))
                if 'run' in routes: timed('run_us', per_step_us, run)
                if 'run_wgrad' in routes: timed('run_wgrad_us', per_step_us, lambda: run(native_wgrad=True))
            opt.zero_grad()
            g = tb.capture(buf, so, labels, d_jit) if 'replay' in routes else None
            gw = tb.capture(buf, so, labels, d_jit, native_wgrad=True) if 'replay_wgrad' in routes else None

            def replay(graph=None):
                (g if graph is None else graph).replay()
                opt.step()

            # the same head goes on training under the native optimiser: one replay is the whole step
            g2 = tb.capture(buf, so, labels, d_jit, optimizer=DeviceAdam(params, lr=1e-4)) if 'replay_adam' in routes else None
            for _ in range(args.rounds):
                if g is not None:
                    timed('replay_us', per_step_us, replay)
                    timed('replay_event_us', per_step_event_us, replay)
                if gw is not None:
                    timed('replay_wgrad_us', per_step_us, lambda: replay(gw))
                    timed('replay_wgrad_event_us', per_step_event_us, lambda: replay(gw))
                if g2 is not None:
                    timed('replay_adam_us', per_step_us, g2.replay)
                    timed('replay_adam_event_us', per_step_event_us, g2.replay)
            row = {k: float(np.median(v)) for k, v in rounds.items()}
            ratio = lambda a, b: row[a] / row[b] if a in row and b in row else None
            if 'host_us' in row and 'host_keep_us' in row:
                row['handle_rebuild_us'] = row['host_us'] - row['host_keep_us']
            for name, (a, b) in {'host_over_run': ('host_us', 'run_us'), 'host_over_replay': ('host_us', 'replay_us'),
                                 'replay_over_replay_adam': ('replay_us', 'replay_adam_us'), 'run_over_run_wgrad': ('run_us', 'run_wgrad_us'),
                                 'replay_over_replay_wgrad': ('replay_us', 'replay_wgrad_us'), 'host_over_run_wgrad': ('host_us', 'run_wgrad_us')}.items():
                if ratio(a, b) is not None:
                    row[name] = ratio(a, b)
            row['spreads'] = {k: float(max(v) - min(v)) for k, v in rounds.items()}
            row['seconds_of_audio'] = float(so[-1]) / rate
            row['rounds'] = rounds
            res['steps'][f'{kind}_B{B}'] = row
            print(f'{kind} B={B}: ' + ', '.join(f'{k}={v:.0f}' for k, v in row.items() if k.endswith('_us')), flush=True)
            del g, gw, g2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
