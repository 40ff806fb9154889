#!/usr/bin/env python3
"""Time per frame of MFCC through the generic kernel on a dense batch of one-second clips: the NFFT sizes
dsp_plan_create_ex(DSP_PLAN_ANY_NFFT) adds (mixed radix: 400, 1200; chirp-z: 1103, 4093) beside the next larger old size
under dsp_debug_force_generic (512, 1536, 4096), and the old path's own figures (NFFT 1024, forced-generic 512).

One process, events around `reps` launches, `rounds` rounds: median and spread (min .. max) per size.  Run it on this commit
and on its parent (sizes the parent refuses are skipped there) to set the figures side by side.

    python tools/kbench_anyfft.py [--batch 4096] [--reps 20] [--rounds 7] [--sizes 512,1024] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (nfft, samplerate): a 25 ms window at the rate that makes the size natural; one second of audio per clip
CASES = ((400, 16000), (512, 16000), (1024, 16000), (1200, 48000), (1103, 44100), (1536, 48000), (4093, 48000), (4096, 48000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--json', default='')
    ap.add_argument('--sizes', default='', help='comma-separated subset of the NFFT sizes (default: all eight)')
    args = ap.parse_args()
    from features import _native as nat
    from features.batch import FeaturePlan
    dev = torch.device('cuda', 0)
    lib = nat.load()
    st = torch.cuda.current_stream(dev)
    B = args.batch
    res = {}
    nat.check(lib.dsp_debug_force_generic(1))
    only = {int(v) for v in args.sizes.split(',') if v}
    for nfft, rate in CASES:
        if only and nfft not in only:
            continue
        try:
            plan = FeaturePlan(samplerate=rate, winlen=0.025, winstep=0.01, numcep=13, nfilt=26, nfft=nfft, preemph=0.97,
                               ceplifter=22, appendEnergy=True, winfunc=np.hamming)
        except nat.DspError as e:
            print(f'nfft {nfft}: refused ({e})')
            continue
        route = plan.plan.transform() if hasattr(plan.plan, 'transform') else (0, 0)
        lay = plan.layout(np.empty((B, rate), dtype=np.float32))
        T = lay.total_frames
        g = torch.Generator(device=dev).manual_seed(nfft)
        waves = 0.25 * torch.randn((B, rate), device=dev, generator=g)
        out = torch.empty((T, 13), device=dev)

        def run():
            nat.check(lib.dsp_features_batch(plan.plan.handle, waves.data_ptr(), nat.WAVE_F32, None, None, B, T, rate,
                                             nat.OUT_MFCC, out.data_ptr(), 13, None, st.cuda_stream))
        for _ in range(3):
            run()
        times = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            for _ in range(args.reps):
                run()
            e1.record(st)
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / args.reps * 1e6 / T)        # ns per frame
        res[str(nfft)] = dict(route=route[0], conv_len=route[1], rate=rate, frames=int(T), ns_per_frame_median=float(np.median(times)),
                              ns_per_frame_min=float(np.min(times)), ns_per_frame_max=float(np.max(times)))
        print(f'nfft {nfft:5d} route {route[0]} conv {route[1]:5d}: {np.median(times):8.2f} ns/frame (min {np.min(times):8.2f}, max {np.max(times):8.2f}), '
              f'{T} frames, generic kernel')
        del waves, out
    nat.check(lib.dsp_debug_force_generic(0))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
