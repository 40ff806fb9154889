#!/usr/bin/env python3
"""Generate tests/golden/anyfft_golden.npz: the ACTUAL reference's mfcc, fbank, powspec, magspec and logpowspec at NFFT sizes
that are neither 2^k nor 3 2^k (tests/anyfft_cases.py: GOLDEN), on short seeded clips.

Like make_cancel_golden.py this runs only where the reference checkout exists (the same default place; override with
REFERENCE_ROOT); nothing of the reference is copied: it is imported from where it lies, called on the clips, and only
numbers are stored.  tests/test_anyfft_host.py pins oracle.dsp_oracle to this file, tests/test_gpu_anyfft.py the public
functions.

    python tests/golden/make_anyfft_golden.py
"""
import io
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402  (REFERENCE_ROOT, or the default checkout)


def main():
    sys.path.insert(0, TESTS)
    sys.path.insert(0, os.path.dirname(TESTS))
    import numpy as np
    import anyfft_cases as ac
    os.environ.setdefault('MPLBACKEND', 'Agg')
    os.chdir(tempfile.mkdtemp(prefix='refscratch_'))        # the reference's config module creates ./log/ at import
    sys.path.insert(0, REF)
    import features as ref                                   # noqa: the reference package
    from features import sigproc as refsig
    out = {}
    for cfg in ac.GOLDEN:
        nfft = cfg[0]
        kw = ac.golden_kw(*cfg)
        x = ac.golden_clip(*cfg).astype(np.float64)
        fr = ac.golden_frames(x, *cfg)
        fb_kw = {k: kw[k] for k in ('samplerate', 'winlen', 'winstep', 'nfilt', 'nfft', 'lowfreq', 'highfreq', 'preemph')}
        feat, energy = ref.fbank(x, winfunc=np.hamming, **fb_kw)
        out[f'{nfft}/mfcc'] = np.asarray(ref.mfcc(x, winfunc=np.hamming, **kw), dtype=np.float64)
        out[f'{nfft}/fbank'] = np.asarray(feat, dtype=np.float64)
        out[f'{nfft}/energy'] = np.asarray(energy, dtype=np.float64)
        out[f'{nfft}/powspec'] = np.asarray(refsig.powspec(fr, nfft), dtype=np.float64)
        out[f'{nfft}/magspec'] = np.asarray(refsig.magspec(fr, nfft), dtype=np.float64)
        out[f'{nfft}/logpowspec'] = np.asarray(refsig.logpowspec(fr, nfft), dtype=np.float64)
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    assert len(buf.getvalue()) < (1 << 20), len(buf.getvalue())
    path = os.path.join(HERE, 'anyfft_golden.npz')
    with open(path, 'wb') as f:
        f.write(buf.getvalue())
    print(f'wrote {path}: {len(ac.GOLDEN)} sizes, {len(buf.getvalue()) / 1e3:.0f} KB')


if __name__ == '__main__':
    main()
