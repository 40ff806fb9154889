#!/usr/bin/env python3
"""Generate tests/golden/pitch_cepstrum_golden.npz by running the ACTUAL reference (features/pitch.py: pitch_detect,
pitch_feature and their helpers) on tests/pitch_cepstrum_cases.py.

Like make_golden.py this runs only where the reference checkout exists (default /root/reference; override with
REFERENCE_ROOT); nothing of the reference is copied: it is imported from where it lies, called on seeded synthetic
inputs, and only numbers are stored.

    python tests/golden/make_pitch_golden.py     # rewrites pitch_cepstrum_golden.npz (+ pitch_cepstrum_manifest.json)

Besides storing the outputs it
  1. asserts that the reference raises on no case but `one_frame`;
  2. repeats every case with the per-frame arithmetic (clip, FIR, FFT, log, inverse FFT) in single precision and the
     tracker in double, and writes into the manifest how many frames of the track differ;
  3. refuses a chirp whose single-precision track differs (pick another seed in pitch_cepstrum_cases.CHIRP_SEEDS),
so the GPU tests' caps on track mismatches are backed by the reference's own arithmetic.
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = os.environ.get('REFERENCE_ROOT', '/root/reference')


def load_reference():
    os.environ.setdefault('MPLBACKEND', 'Agg')
    os.chdir(tempfile.mkdtemp(prefix='refscratch_'))        # the reference's config module creates ./log/ at import
    sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import features.pitch as rp                         # noqa: the reference module
    return rp


def run_reference(rp, sig, rate):
    import numpy as np
    s = rp.downsampling(sig, rate, 10000)
    frames = rp.to_frames(s, 10000, 0.0512, 0.01)
    rows = np.array([rp.pitch_detect_frame(rp.center_clip(f, False), 10000, 'male') for f in frames])
    scores = np.array([rp.peak_score(r) for r in rp.smooth(rows)], dtype=np.int32)
    pitch = np.array(rp.robust_max_pitch(scores))
    chk, _ = rp.pitch_detect(sig, rate)
    assert np.array_equal(pitch, np.array(chk)), 'the stepwise call differs from pitch_detect'
    out = dict(rows=rows, scores=scores, pitch=pitch, n_frames=np.int64(len(frames)))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            feat = rp.pitch_feature(sig, rate)
    except ValueError:
        out['raises'] = np.int64(1)
        return out
    p = rp.sub_endpoint_detect(frames)
    p_bias = 5 if p > 15 else 0
    s1, i1 = rp.find_smooth_subsequence(list(pitch[p_bias:p]), bias=p_bias)
    s2, i2 = rp.find_smooth_subsequence(list(pitch[p:]), bias=p)
    out.update(raises=np.int64(0), p=np.int64(p), seg1=np.array(s1), seg2=np.array(s2), idx1=np.array(i1, dtype=np.int64),
               idx2=np.array(i2, dtype=np.int64), feat=np.array(feat, dtype=np.float64))
    return out


def single_precision_track(rp, sig, rate):
    """The reference's per-frame arithmetic in single precision, its tracker in double -> (pitch, scores)."""
    import numpy as np
    s = rp.downsampling(sig, rate, 10000)
    frames = rp.to_frames(s, 10000, 0.0512, 0.01).astype(np.float32)
    L = frames.shape[1]
    Hd = np.zeros(L)
    Hd[int(L * 50 / 10000):int(L * 1000 / 10000)] = 1
    h = (2 * np.pi * np.hamming(L) * np.fft.ifft(Hd, L)).astype(np.complex64)
    rows = []
    for f in frames:
        pos = f[f >= 0]
        med = np.median(pos) if len(pos) else np.float32(np.nan)
        c = np.where(f > med, f - med, np.where(f < -med, f + med, np.float32(0))).astype(np.float32)
        y = np.convolve(c.astype(np.complex64), h)[:L]
        X = np.fft.fft(y)
        assert X.dtype == np.complex64
        rows.append(np.abs(np.fft.ifft(np.log(np.abs(X)))).astype(np.float64))
    scores = np.array([rp.peak_score(r) for r in rp.smooth(np.array(rows))], dtype=np.int32)
    return np.array(rp.robust_max_pitch(scores)), scores


def main():
    sys.path.insert(0, TESTS)
    import numpy as np
    from pitch_cepstrum_cases import CASES, ROWS_CASES, make_input

    rp = load_reference()
    out, manifest, differing = {}, {}, []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for case in CASES:
            sig, rate = make_input(case)
            res = run_reference(rp, sig, rate)
            assert bool(res['raises']) == (case['name'] == 'one_frame'), (case['name'], 'raises', res['raises'])
            p32, s32 = single_precision_track(rp, sig, rate)
            n_diff = int(np.sum(p32 != res['pitch']))
            n_rows = int(np.sum(np.any(s32 != res['scores'], axis=1)))
            if case['kind'] == 'chirp' and n_diff:
                differing.append(case['name'])
            if case['name'] not in ROWS_CASES:
                res.pop('rows')
            manifest[case['name']] = dict(seed=case['seed'], rate=rate, dtype=str(sig.dtype), n_samples=int(len(sig)),
                                          n_frames=int(res['n_frames']), fp32_track_frames_differing=n_diff,
                                          fp32_score_rows_differing=n_rows,
                                          arrays={k: [list(np.shape(v)), str(np.asarray(v).dtype)] for k, v in res.items()})
            for k, v in res.items():
                out[f"{case['name']}/{k}"] = v
            print(case['name'], rate, sig.dtype, 'frames', int(res['n_frames']), 'fp32 track diff', n_diff, 'score rows', n_rows,
                  'feat', res.get('feat'))
    if differing:
        raise SystemExit(f'single-precision track differs on {differing}: pick other seeds for them')
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    assert len(buf.getvalue()) < (1 << 20), len(buf.getvalue())
    path = os.path.join(HERE, 'pitch_cepstrum_golden.npz')
    with open(path, 'wb') as f:
        f.write(buf.getvalue())
    total = sum(m['n_frames'] for n, m in manifest.items() if n.startswith('chirp'))
    with open(os.path.join(HERE, 'pitch_cepstrum_manifest.json'), 'w') as f:
        json.dump({'numpy': np.__version__, 'chirp_frames': total, 'cases': manifest}, f, indent=1, sort_keys=True)
    print(f'wrote {path}: {len(CASES)} cases, {len(out)} arrays, {len(buf.getvalue()) / 1e6:.2f} MB, {total} chirp frames')


if __name__ == '__main__':
    main()
