#!/usr/bin/env python3
"""Generate tests/golden/cancel_golden.npz: the engineered clips of tests/cancel_cases.py and the ACTUAL reference's
base.mfcc of them.

Like make_golden.py this runs only where the reference checkout exists (the same default place; override with
REFERENCE_ROOT); nothing of the reference is copied: it is imported from where it lies, called on the clips, and only
numbers are stored.  The oracle has to be right to 1e-6 of a bin at these frames, so tests/test_cancel_cases_host.py pins
oracle.dsp_oracle.mfcc to this file.

    python tests/golden/make_cancel_golden.py
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
    from cancel_cases import CASES, make_input, plan_kwargs
    os.environ.setdefault('MPLBACKEND', 'Agg')
    os.chdir(tempfile.mkdtemp(prefix='refscratch_'))        # the reference's config module creates ./log/ at import
    sys.path.insert(0, REF)
    import features as ref                                   # noqa: the reference package
    out = {}
    for case in CASES:
        x = make_input(case)
        kw, wf = plan_kwargs(case)
        out[f"{case['name']}/x"] = x
        out[f"{case['name']}/mfcc"] = np.asarray(ref.mfcc(x.astype(np.float64), winfunc=wf, **kw), dtype=np.float64)
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    assert len(buf.getvalue()) < (1 << 20), len(buf.getvalue())
    path = os.path.join(HERE, 'cancel_golden.npz')
    with open(path, 'wb') as f:
        f.write(buf.getvalue())
    print(f'wrote {path}: {len(CASES)} cases, {len(buf.getvalue()) / 1e3:.0f} KB')


if __name__ == '__main__':
    main()
