#!/usr/bin/env python3
"""Times the ensemble's last step at B = 512 with the two fitted pitch SVMs of tests/golden/ensemble_golden.npz and about a
quarter of the clips gated:

  (a) device   dsp_ensemble_decide_batch on device-resident logits [B, 20] and pitch features [B, 5]: one launch;
  (b) host     the route it replaces, in the same process: download the logits and the features, run the gate on the host
               (tests/ensemble_ref.py: NumPy softmax / arg-max, the SVM per gated clip), upload the labels [B].

Both produce the same labels (checked).  Prints one JSON line; medians over --repeats groups of --iters calls, the host
route synchronised per call (it cannot be otherwise), the device call timed between two events around each group.

    python tools/kbench_ensemble.py [--batch 512] [--iters 200] [--repeats 7]

``--capacity`` times something else instead: ``EnsembleBatch.capture(..., capacity=)`` against the exact-shape graph at B = 32 and
512 with both heads, and an epoch of 8 length vectors through ONE capacity graph against the eager sync-free route
(tools/kbench_capacity.py; device events, --capacity-iters replays, median of 3 rounds), merged into
profiles/capacity_layout_kbench.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--capacity', action='store_true')
    ap.add_argument('--capacity-iters', type=int, default=20)
    ap.add_argument('--capacity-batches', default='32,512')
    args = ap.parse_args()
    if args.capacity:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        import kbench_capacity
        rows = kbench_capacity.ensemble_section(tuple(int(v) for v in args.capacity_batches.split(',')), iters=args.capacity_iters)
        print(json.dumps({'ensemble': kbench_capacity.merge('ensemble', rows)['ensemble']}))
        return 0
    import torch
    import ensemble_ref as ref
    from ensemble_cases import N_CLASSES, PAIRS, THRESHOLDS
    from features import _native as nat
    from features.ensemble import PitchSVM, ensemble_decide
    nat.require_device()
    dev = torch.device('cuda', nat.current_device())
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ensemble_golden.npz')) as z:
        gold = {k: z[k] for k in z.files}
    models = []
    for pair in PAIRS:
        name = f'svm{pair[0]}{pair[1]}'
        models.append({k: gold[f'{name}/{k}'] for k in ('scale', 'support_vectors', 'dual_coef', 'intercept', 'gamma', 'classes')})
    svms = [PitchSVM.from_arrays(m['support_vectors'], m['dual_coef'], m['intercept'], m['gamma'], m['classes'], scale=m['scale'])
            for m in models]
    rules = list(zip(PAIRS, THRESHOLDS, svms))
    rules_host = list(zip(PAIRS, THRESHOLDS, models))
    # a quarter of the clips: one of the four gated labels at a confidence below both thresholds; the rest confident
    rng = np.random.default_rng(0)
    B = args.batch
    logits = rng.uniform(-0.05, 0.05, (B, N_CLASSES))
    top = rng.integers(0, N_CLASSES, B)
    conf = rng.uniform(0.85, 0.99, B)
    gated = rng.random(B) < 0.25
    top[gated] = rng.choice([0, 1, 6, 7], int(gated.sum()))
    conf[gated] = rng.uniform(0.3, 0.65, int(gated.sum()))
    logits[np.arange(B), top] = np.log((N_CLASSES - 1) * conf / (1 - conf))
    logits = logits.astype(np.float32)
    feat = gold['svm01/queries'][rng.integers(0, len(gold['svm01/queries']), B)]
    d_logits, d_feat = torch.from_numpy(logits).to(dev), torch.from_numpy(np.ascontiguousarray(feat)).to(dev)

    def device_call():
        return ensemble_decide(d_logits, rules, d_feat)

    def host_call():
        lg, ft = d_logits.cpu().numpy(), d_feat.cpu().numpy()
        pred, _, _ = ref.gate(lg, rules_host, ft)
        return torch.from_numpy(pred).to(dev)

    pred_d, _, used_d, _ = device_call()
    pred_h = host_call()
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(pred_d, pred_h))
    n_gated = int((used_d != 0).sum())

    def time_device():
        for _ in range(20):
            device_call()
        out = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.iters):
                device_call()
            b.record()
            torch.cuda.synchronize(dev)
            out.append((a.elapsed_time(b) * 1e3 / args.iters, (time.perf_counter() - t0) * 1e6 / args.iters))
        return out

    def time_host():
        for _ in range(3):
            host_call()
        out = []
        n = max(args.iters // 10, 5)
        for _ in range(args.repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                host_call()
            torch.cuda.synchronize(dev)
            out.append((time.perf_counter() - t0) * 1e6 / n)
        return out

    dev_t, host_t = time_device(), time_host()
    print(json.dumps(dict(
        batch=B, n_classes=N_CLASSES, n_gated=n_gated, n_sv=[s.n_sv for s in svms], labels_equal=same,
        device_us_per_call_gpu_median=float(np.median([t[0] for t in dev_t])),
        device_us_per_call_wall_median=float(np.median([t[1] for t in dev_t])),
        device_us_per_call_gpu_all=[round(t[0], 2) for t in dev_t],
        host_route_us_per_call_wall_median=float(np.median(host_t)), host_route_us_per_call_wall_all=[round(t, 1) for t in host_t],
        iters=args.iters, repeats=args.repeats)))
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
