#!/usr/bin/env python3
"""Times the native speaker discriminator (csrc/kernels_adv.h, features/adversarial.py) against the torch chain it replaces:

  loss   ``AdvHRNNHead.speaker_loss`` forward + backward on a pooled feature of [32, 400] and [512, 400] -- the native node
         (``dsp_adv_disc_train`` + a backward from ``unit_grad`` that launches nothing) against
         ``F.cross_entropy(d2(tanh(d1(gradient_reverse(feat, gamma)))), speakers)`` + ``backward`` on the same device -- eager and
         as a recorded pair (one HIP graph each);
  step   one ``AdvTrainBatch`` step (front end, both GRU levels, both losses, backward; no optimiser) with ``native_disc=True``
         against ``native_disc=False``, eager, at B = 32 and B = 512.

Clocks as found.  Device events round --iters back-to-back calls after --warmup; median of --rounds rounds with the spread
(max - min); the arms alternate inside each round.  Writes --out (default profiles/adv_kbench.json) and prints it as one JSON
line.

    python tools/kbench_adv.py [--iters 30] [--warmup 3] [--rounds 3] [--sections loss,step]
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from kbench_metrics import compare, cut, offsets, record_pair, verdict  # noqa: E402


def make_head(torch, C, dev):
    torch.manual_seed(0)
    head = C.AdvHRNNHead().train()
    C.fill_parameters(head, 3)
    for m in head.modules():
        if isinstance(m, C._DynEnc):
            m.gru.dropout = 0.0
    return head.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--sections', default='loss,step')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'adv_kbench.json'))
    args = ap.parse_args()
    import torch
    from ensemble_cases import make_clips
    from features import classifier as C
    from features import metrics as M
    from features.train import AdvTrainBatch
    dev = torch.device('cuda', 0)
    sections = args.sections.split(',')
    res = {'iters': args.iters, 'warmup': args.warmup, 'rounds': args.rounds,
           'clock': 'device events round iters back-to-back calls; median of the rounds, spread = max - min; clocks as found'}
    head = make_head(torch, C, dev)
    M.unit_grad(dev)

    if 'loss' in sections:
        res['loss'] = {}
        for B in (32, 512):
            rng = np.random.default_rng(B)
            feat = torch.from_numpy(rng.uniform(-1, 1, (B, 400)).astype(np.float32)).to(dev).requires_grad_(True)
            spk = torch.from_numpy(rng.integers(0, 35, B).astype(np.int64)).to(dev)

            def pair(native):
                def fn():
                    feat.grad = None
                    head.zero_grad(set_to_none=True)
                    r = head.speaker_loss(feat, spk, native=native)
                    if native:
                        M.backward(r.loss)
                    else:
                        r.loss.backward()
                    return r.loss, feat.grad
                return fn
            arms = {'native': pair(True), 'torch': pair(False)}
            graphs = {k: record_pair(torch, dev, fn) for k, fn in arms.items()}
            arms.update({k + '_recorded': g.replay for k, (g, _) in graphs.items()})
            row = compare(torch, dev, arms, args.iters, args.warmup, args.rounds)
            row['eager_verdict'] = verdict(row['native_us'], row['torch_us'])
            row['recorded_verdict'] = verdict(row['native_recorded_us'], row['torch_recorded_us'])
            res['loss'][f'{B}x400'] = row

    if 'step' in sections:
        res['step'] = {}
        stored, rate = make_clips()
        for B in (32, 512):
            tb = AdvTrainBatch(rate, head)
            clips = cut(stored, B, 1)
            rng = np.random.default_rng(B)
            flat = torch.from_numpy(np.concatenate(clips)).to(dev)
            so = offsets(clips)
            lab = torch.from_numpy(rng.integers(0, 20, B).astype(np.int64)).to(dev)
            spk = torch.from_numpy(rng.integers(0, 35, B).astype(np.int64)).to(dev)
            jit = torch.from_numpy(tb.draw_jitter(B, random.Random(B))).to(dev)

            def step(native):
                def fn():
                    head.zero_grad(set_to_none=True)
                    out = tb.run(flat, so, lab, spk, jit, loss='native', native_disc=native, dropout=False)
                    AdvTrainBatch.backward(out)
                return fn
            row = compare(torch, dev, {'native_disc': step(True), 'torch_disc': step(False)}, max(3, args.iters // 3), args.warmup, args.rounds)
            row['verdict'] = verdict(row['native_disc_us'], row['torch_disc_us'])
            res['step'][f'B{B}'] = row

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
