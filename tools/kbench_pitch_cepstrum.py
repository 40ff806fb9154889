#!/usr/bin/env python3
"""Cepstral pitch features (pitch.pitch_feature) against the autocorrelation tracker (pitch.pitch_detect_sr), both from
device-resident 44.1 kHz clips at 512-sample frames:

    python tools/kbench_pitch_cepstrum.py [--batch 1024] [--iters 20] [--out profiles/pitch_cepstrum_timing.txt]

The clips are SURVEY 8d's class C as bench.py's model_path builds them (noise background, one Hann-shaped tone burst,
1 - 2 s), from a fixed seed, whole and untrimmed.  Reported: the median of hipEvent-timed calls of
pitch_features_device and of pitch_tracks_device, and -- on the same decimated frames, with the launch grid at the exact
frame count -- the two per-frame kernels alone (dsp_pitch_cepstrum_batch, dsp_pitch_scores_batch) and the two trackers,
and dsp_pitch_scores_batch at 300-sample frames of the same decimated clips, the kernel the model path runs.
Per-kernel times: one `rocprofv3 --kernel-trace --stats -- python tools/kbench_pitch_cepstrum.py` run.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd')):
    sys.path.insert(0, p)
import numpy as np
import torch


def class_c_clips(batch, rate, seed=9):
    rng = np.random.default_rng(seed)
    clips = []
    for _ in range(batch):
        n = int(rng.uniform(1.0, 2.0) * rate)
        x = rng.normal(0, 30, n)
        blen = int(rng.uniform(0.5, 0.9) * n)
        b0 = int(rng.integers(0, n - blen))
        t = np.arange(blen) / rate
        x[b0:b0 + blen] += 8000 * np.sin(2 * np.pi * rng.uniform(100, 300) * t) * np.hanning(blen)
        clips.append(np.clip(np.round(x), -32768, 32767).astype(np.float32))
    return clips


def median_us(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    from features import _native as nat
    from features import pitch as gp
    lib = nat.load()
    dev = torch.device('cuda', 0)
    rate, L, S, B = 44100, 512, 100, args.batch
    clips = class_c_clips(B, rate)
    so = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    x = torch.from_numpy(np.concatenate(clips)).to(dev)
    d_so = torch.from_numpy(so).to(dev)
    n = int(so[-1])
    st = torch.cuda.current_stream(dev).cuda_stream

    us_feat = median_us(lambda: gp.pitch_features_device(x.data_ptr(), d_so.data_ptr(), B, n, rate, stream=st), args.iters)
    us_sr = median_us(lambda: gp.pitch_tracks_device(x.data_ptr(), d_so.data_ptr(), B, n, rate, L, S, stream=st), args.iters)
    r = gp.pitch_features_device(x.data_ptr(), d_so.data_ptr(), B, n, rate, stream=st)
    torch.cuda.synchronize()
    valid = int(np.sum(r.aux.download((B, 9), np.int32)[:, 8]))
    frames = int(r.frame_off.download((B + 1,), np.int64)[-1])

    # the kernels alone, on the same 10 kHz frames, grids at the exact frame count
    d_fo = r.frame_off.ptr
    d_x10 = nat.SCRATCH.get('pitch_x10', 4).ptr
    d_so10 = nat.SCRATCH.get('pitch_so10', 4).ptr
    rows = torch.empty((frames, L), device=dev)
    amp = torch.empty(frames, dtype=torch.float64, device=dev)
    scores = torch.empty((frames, 180), device=dev)
    pitch = torch.empty(frames, dtype=torch.float64, device=dev)
    seg = torch.empty(frames, dtype=torch.float64, device=dev)
    feat = torch.empty((B, 5), dtype=torch.float64, device=dev)
    aux = torch.empty((B, 9), dtype=torch.int32, device=dev)
    t_cep, t_sr = gp._device_taps(L, 10000, 1000).ptr, gp._device_taps(L, 10000).ptr
    ck = nat.check
    us = {
        'dsp_pitch_cepstrum_batch (pitch_cepstrum_kernel<512>)': median_us(lambda: ck(lib.dsp_pitch_cepstrum_batch(
            d_x10, d_so10, d_fo, B, frames, 0, L, S, t_cep, 1, rows.data_ptr(), amp.data_ptr(), st)), args.iters),
        'dsp_pitch_scores_batch (pitch_scores_kernel_v2<4>)': median_us(lambda: ck(lib.dsp_pitch_scores_batch(
            d_x10, d_so10, d_fo, B, frames, 0, L, S, t_sr, 1, 20, 200, scores.data_ptr(), st)), args.iters),
        'dsp_pitch_cepstrum_track_batch (pitch_cepstrum_track_kernel<float, 512>)': median_us(lambda: ck(
            lib.dsp_pitch_cepstrum_track_batch(rows.data_ptr(), 0, d_fo, B, L, 3, pitch.data_ptr(), None, st)), args.iters),
        'dsp_pitch_track_batch (pitch_track_kernel)': median_us(lambda: ck(lib.dsp_pitch_track_batch(
            scores.data_ptr(), d_fo, B, 180, 20, 2, pitch.data_ptr(), st)), args.iters),
    }
    ck(lib.dsp_pitch_cepstrum_track_batch(rows.data_ptr(), 0, d_fo, B, L, 3, pitch.data_ptr(), None, st))
    us['dsp_pitch_feature_batch (pitch_feature_kernel)'] = median_us(lambda: ck(lib.dsp_pitch_feature_batch(
        pitch.data_ptr(), amp.data_ptr(), d_fo, B, seg.data_ptr(), feat.data_ptr(), aux.data_ptr(), st)), args.iters)
    k_cep, k_sr = list(us.values())[0], list(us.values())[1]
    # the model path's frame length on the same decimated clips, with frame offsets of its own
    fo300 = torch.empty(B + 1, dtype=torch.int64, device=dev)
    ck(lib.dsp_resample_layout_batch(d_so10, B, 10000, 0, 300, S, None, fo300.data_ptr(), st))
    frames300 = int(fo300[-1])
    scores300, t_sr300 = torch.empty((frames300, 180), device=dev), gp._device_taps(300, 10000).ptr
    us300 = median_us(lambda: ck(lib.dsp_pitch_scores_batch(
        d_x10, d_so10, fo300.data_ptr(), B, frames300, 0, 300, S, t_sr300, 1, 20, 200, scores300.data_ptr(), st)), args.iters)
    lines = [
        f'{B} class-C clips at {rate} Hz ({n} samples, device resident) -> {frames} frames of {L} at 10 kHz; '
        f'median of {args.iters} hipEvent-timed calls',
        f'pitch_features_device (decimate + cepstrum rows + tracker + feature tail): {us_feat:9.1f} us per call '
        f'= {us_feat / B:.2f} us per clip ({valid} of {B} clips valid)',
        f'pitch_tracks_device   (decimate + autocorrelation scores + tracker)     : {us_sr:9.1f} us per call '
        f'= {us_sr / B:.2f} us per clip',
    ] + [f'{k:76s}: {v:9.1f} us = {v / frames * 1e3:8.2f} ns per frame' for k, v in us.items()] + [
        f"{'dsp_pitch_scores_batch at L = 300 (pitch_scores_kernel_v2<3>)':76s}: {us300:9.1f} us = "
        f'{us300 / frames300 * 1e3:8.2f} ns per frame ({frames300} frames)',
        f'cepstrum rows kernel / autocorrelation scores kernel, per frame: {k_cep / k_sr:.3f} x (margin 1.5 x)']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
