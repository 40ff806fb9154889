#!/usr/bin/env python3
"""Times the device-side loss / metrics (csrc/kernels_loss.h, features/metrics.py, features/fit.py) against what they replace:

  call     ``dsp_xent_metrics_batch`` for the loss and its gradient at [32, 20] and [512, 20] -- the raw call (``xent``) and the
           autograd pair (``cross_entropy`` + ``backward``) -- against ``F.cross_entropy`` forward + backward on the same logits,
           eager and as a recorded pair (one HIP graph each);
  update   ``Metrics.update(logits, labels, pred)`` against the route it replaces: download ``pred`` and ``labels``, NumPy
           accuracy + ``np.add.at``;
  epoch    an epoch of 8 batches (new clips, lengths, labels, jitter each) through ``Trainer``'s recorded step with ONE
           ``result()`` at its end, against (a) the hand-written eager loop and (b) the capacity graph with torch's loss, both
           with ``loss.item()`` after every step as model.py:150 reads it: ``TransformerHead`` B = 32, ``HMRNNHead`` B = 512;
  val      a validation epoch of 8 batches through ``EnsembleBatch``'s capacity graph with ``labels=, metrics=`` and one
           ``result()``, against the same graph with ``pred`` downloaded per batch and scored in NumPy.

Clocks as found.  ``call`` / ``update``: device events round --iters back-to-back calls after --warmup; ``epoch`` / ``val``: host
clock round one epoch between two synchronisations (the downloads are the point).  Median of --rounds rounds with the spread
(max - min); the arms alternate inside each round.  Writes --out (default profiles/metrics_kbench.json) and prints it as one
JSON line.

    python tools/kbench_metrics.py [--iters 50] [--warmup 3] [--rounds 3] [--sections call,update,epoch,val]
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

N_BATCHES = 8


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


def host_us(torch, dev, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e6 / iters


def compare(torch, dev, arms, iters, warmup, rounds, clock=event_us):
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            times[name].append(clock(torch, dev, fn, iters, warmup))
    row = {'rounds': times}
    for name, v in times.items():
        row[name + '_us'] = float(np.median(v))
        row[name + '_spread_us'] = float(max(v) - min(v))
    return row


def verdict(a, b):
    return 'ahead' if a < b else 'NOT ahead'


def record_pair(torch, dev, make):
    """One HIP graph of ``make()`` (forward + backward of a loss), after a warm call on the capture stream."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.autograd.set_multithreading_enabled(False):         # every recorded launch comes from the capturing thread
        with torch.cuda.stream(side):
            make()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            keep = make()
    return g, keep


def cut(stored, B, k):
    out = []
    for i in range(B):
        c = stored[(i + 3 * k) % len(stored)]
        out.append(c[:int((0.60 + 0.05 * ((7 * i + 3 * k) % 5)) * len(c)) + (7 * i + k) % 97])
    return out


def offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


def make_head(torch, C, kind, dev, train):
    torch.manual_seed(0)
    head = getattr(C, kind)()
    head = head.train() if train else head.eval()
    C.fill_parameters(head, 3)
    for m in head.modules():
        if isinstance(m, C._DynEnc):
            m.gru.dropout = 0.0
    return head.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--sections', default='call,update,epoch,val')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metrics_kbench.json'))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from ensemble_cases import make_clips
    from features import _native as nat
    from features import classifier as C
    from features import fit, metrics as M
    from features.ensemble import EnsembleBatch
    from features.optim import DeviceAdam
    from features.train import TrainBatch
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    sections = set(args.sections.split(','))
    res = {'iters': args.iters, 'warmup': args.warmup, 'rounds': args.rounds,
           'clock': 'call / update: device events round iters back-to-back calls; epoch / val: host clock round one epoch between two '
                    'synchronisations; median of the rounds, spread = max - min; clocks as found',
           'call': {}, 'update': {}, 'epoch': {}, 'val': {}}

    if 'call' in sections:
        for B, Cn in ((32, 20), (512, 20)):
            rng = np.random.default_rng(B)
            x = torch.from_numpy((3 * rng.standard_normal((B, Cn))).astype(np.float32)).to(dev).requires_grad_(True)
            lab = torch.from_numpy(rng.integers(0, Cn, B).astype(np.int64)).to(dev)

            def native_pair():
                loss = M.cross_entropy(x, lab)
                return loss, torch.autograd.grad(loss, x, grad_outputs=M.unit_grad(dev))[0]

            def torch_pair():
                loss = F.cross_entropy(x, lab)
                return loss, torch.autograd.grad(loss, x)[0]
            g_native, keep_n = record_pair(torch, dev, native_pair)
            g_torch, keep_t = record_pair(torch, dev, torch_pair)
            arms = {'native_call': lambda: M.xent(x.detach(), lab, want=('loss', 'dlogits')), 'native_autograd': native_pair,
                    'torch': torch_pair, 'native_recorded': g_native.replay, 'torch_recorded': g_torch.replay}
            row = compare(torch, dev, arms, args.iters, args.warmup, args.rounds)
            row['eager_verdict'] = verdict(row['native_autograd_us'], row['torch_us'])
            row['recorded_verdict'] = verdict(row['native_recorded_us'], row['torch_recorded_us'])
            res['call'][f'{B}x{Cn}'] = row
            print(f'call [{B}, {Cn}]: ' + ', '.join(f'{k}={v:.1f}' for k, v in row.items() if k.endswith('_us')), flush=True)

    if 'update' in sections:
        for B, Cn in ((32, 20), (512, 20)):
            rng = np.random.default_rng(B + 1)
            x = torch.from_numpy((3 * rng.standard_normal((B, Cn))).astype(np.float32)).to(dev)
            lab = torch.from_numpy(rng.integers(0, Cn, B).astype(np.int64)).to(dev)
            pred = x.argmax(dim=1).to(torch.int32)
            m = M.Metrics(Cn, 4096, dev)
            conf, tally = np.zeros((Cn, Cn), dtype=np.int64), [0, 0]

            def download():
                p, y = pred.cpu().numpy(), lab.cpu().numpy()
                tally[0] += int((p == y).sum())
                tally[1] += len(y)
                np.add.at(conf, (y, p), 1)
            row = compare(torch, dev, {'native': lambda: m.update(x, lab, pred), 'download_numpy': download}, args.iters, args.warmup,
                          args.rounds)
            row['verdict'] = verdict(row['native_us'], row['download_numpy_us'])
            res['update'][f'{B}x{Cn}'] = row
            print(f'update [{B}, {Cn}]: ' + ', '.join(f'{k}={v:.1f}' for k, v in row.items() if k.endswith('_us')), flush=True)

    stored, rate = make_clips()
    configs = (('TransformerHead', 32), ('HMRNNHead', 512))

    if 'epoch' in sections:
        for kind, B in configs:
            head = make_head(torch, C, kind, dev, True)
            tb, eb = TrainBatch(rate, head), EnsembleBatch(rate, head, [])
            opt = DeviceAdam(list(head.parameters()), lr=1e-4)
            trainer = fit.Trainer(tb, eb, opt, 20, head_kwargs={'dropout': False})
            clips = [c for k in range(N_BATCHES) for c in cut(stored, B, k)]
            labels = np.random.default_rng(B).integers(0, 20, len(clips)).astype(np.int64)
            ph = fit._Phase(([(c, rate) for c in clips], labels), 'train')
            cap = int(sum(sorted((len(c) for c in clips), reverse=True)[:B]))
            batches = [list(range(k * B, (k + 1) * B)) for k in range(N_BATCHES)]
            sink = []

            def trainer_epoch():
                opt.reset()
                opt.set_lr(1e-4)
                trainer.train_metrics.reset()
                for idx in batches:
                    trainer._train_step(ph, idx, B, cap, np.int16, torch.int16, True)
                sink.append(trainer.train_metrics.result().loss)

            def eager_epoch():
                opt.reset()
                opt.set_lr(1e-4)
                for idx in batches:
                    flat, so, lab = trainer._flat(ph, idx, np.int16)
                    jitter = tb.draw_jitter(B, trainer.jitter_rng)
                    for p in opt.params:
                        p.grad = None
                    out = tb.run(flat, so, lab, jitter, dropout=False)
                    out.loss.backward()
                    opt.step()
                    sink.append(out.loss.item())
            # (b) the capacity graph with torch's loss, its buffers written as Trainer writes its own
            buf = torch.zeros(cap, dtype=torch.int16, device=dev)
            lab_d = torch.zeros(B, dtype=torch.int64, device=dev)
            jit_d = torch.zeros((B, 2), dtype=torch.int64, device=dev)
            flat0, so0, _ = trainer._flat(ph, batches[0], np.int16)
            buf[:len(flat0)].copy_(torch.from_numpy(flat0))
            g = tb.capture(buf, so0, lab_d, jit_d, optimizer=opt, capacity=cap, dropout=False)

            def graph_item_epoch():
                opt.reset()
                opt.set_lr(1e-4)
                for idx in batches:
                    flat, so, lab = trainer._flat(ph, idx, np.int16)
                    jitter = tb.draw_jitter(B, trainer.jitter_rng)
                    buf[:len(flat)].copy_(torch.from_numpy(flat))
                    lab_d.copy_(torch.from_numpy(lab))
                    jit_d.copy_(torch.from_numpy(jitter))
                    g.sample_offsets.copy_(torch.from_numpy(so))
                    sink.append(g.replay().loss.item())
            row = compare(torch, dev, {'trainer_graph': trainer_epoch, 'eager_item': eager_epoch, 'torch_loss_graph_item': graph_item_epoch},
                          1, 1, args.rounds, clock=host_us)
            row['batches'], row['capacity'] = N_BATCHES, cap
            row['verdict_vs_eager'] = verdict(row['trainer_graph_us'], row['eager_item_us'])
            row['verdict_vs_graph_item'] = verdict(row['trainer_graph_us'], row['torch_loss_graph_item_us'])
            res['epoch'][f'{kind}_B{B}'] = row
            print(f'epoch {kind} B={B}: ' + ', '.join(f'{k}={v:.0f}' for k, v in row.items() if k.endswith('_us')), flush=True)
            del g, trainer, ph

    if 'val' in sections:
        for kind, B in configs:
            head = make_head(torch, C, kind, dev, False)
            eb = EnsembleBatch(rate, head, [])
            m = M.Metrics(20, 4096, dev)
            sets = [cut(stored, B, k) for k in range(N_BATCHES)]
            cap = max(sum(len(c) for c in s) for s in sets)
            flats = [(np.concatenate(s), offsets(s), np.random.default_rng(k).integers(0, 20, B).astype(np.int64)) for k, s in enumerate(sets)]
            buf = torch.zeros(cap, dtype=torch.int16, device=dev)
            lab_d = torch.zeros(B, dtype=torch.int64, device=dev)
            buf[:len(flats[0][0])].copy_(torch.from_numpy(flats[0][0]))
            with torch.no_grad():
                g_m = eb.capture(buf, flats[0][1], capacity=cap, labels=lab_d, metrics=m, dropout=False)
                g_p = eb.capture(buf, flats[0][1], capacity=cap, dropout=False)
            sink = []

            def metrics_epoch():
                m.reset()
                for flat, so, lab in flats:
                    buf[:len(flat)].copy_(torch.from_numpy(flat))
                    lab_d.copy_(torch.from_numpy(lab))
                    g_m.sample_offsets.copy_(torch.from_numpy(so))
                    g_m.replay()
                sink.append(m.result().accuracy)

            def download_epoch():
                conf, right = np.zeros((20, 20), dtype=np.int64), 0
                for flat, so, lab in flats:
                    buf[:len(flat)].copy_(torch.from_numpy(flat))
                    g_p.sample_offsets.copy_(torch.from_numpy(so))
                    p = g_p.replay().pred.cpu().numpy()
                    right += int((p == lab).sum())
                    np.add.at(conf, (lab, p), 1)
                sink.append(right / (B * len(flats)))
            row = compare(torch, dev, {'metrics_graph': metrics_epoch, 'download_per_batch': download_epoch}, 1, 1, args.rounds, clock=host_us)
            row['batches'], row['capacity'] = N_BATCHES, cap
            row['verdict'] = verdict(row['metrics_graph_us'], row['download_per_batch_us'])
            res['val'][f'{kind}_B{B}'] = row
            print(f'val {kind} B={B}: ' + ', '.join(f'{k}={v:.0f}' for k, v in row.items() if k.endswith('_us')), flush=True)
            del g_m, g_p

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
