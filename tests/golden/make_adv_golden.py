#!/usr/bin/env python3
"""Generate tests/golden/adv_golden.npz by running the ACTUAL reference class adv_clf.AdvHRNN on the CPU of the build container
(cfg.cuda = False), on the input of tests/golden/rnn_golden.npz (B = 8).

Nothing of the reference is copied: it is imported from its checkout (REFERENCE_ROOT), its parameters are overwritten with seeded values
(features/classifier.py::fill_parameters), and only parameter names and outputs are stored.  The class as it stands cannot run
end to end on a current torch -- its ``rev`` is a legacy autograd Function and its ``forward`` calls ``HRNN.forward`` with a stale
signature -- so the real layers are called in the order of adv_clf.py:34-38 with ``rev`` as the identity (which is what it is in
the forward pass): ``ref.g(inp, len0, return_feature=True)`` with torch.nn.functional.dropout replaced by the identity for the
call's duration, then ``ref.d2(tanh(ref.d1(feat)))``.

    python tests/golden/make_adv_golden.py
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('REFERENCE_ROOT', '/root/reference')
SEED = 20261021


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(ROOT, 'dsp-speech-recognition_amd'))
    from features.classifier import fill_parameters
    sys.path.pop(0)
    for name in [n for n in sys.modules if n == 'features' or n.startswith('features.')]:
        del sys.modules[name]                              # the reference has a package of the same name
    g = np.load(os.path.join(HERE, 'rnn_golden.npz'))
    inp, len0 = torch.from_numpy(g['inp']), g['len0']
    os.environ.setdefault('MPLBACKEND', 'Agg')
    os.chdir(tempfile.mkdtemp(prefix='refscratch_'))      # the reference's config creates ./log/ at import
    sys.path.insert(0, REF)
    import config
    config.cfg.cuda = False
    import adv_clf
    torch.manual_seed(0)
    ref = adv_clf.AdvHRNN().eval()
    out = {'seed': np.int64(SEED), 'names': np.array(fill_parameters(ref, SEED))}
    real_dropout = F.dropout
    with torch.no_grad():
        F.dropout = lambda x, *a, **kw: x
        try:
            logits, feat = ref.g(inp, len0, return_feature=True)
        finally:
            F.dropout = real_dropout
        logits2 = ref.d2(torch.tanh(ref.d1(feat)))
    out['feat'], out['logits_nodrop'], out['logits2'] = feat.numpy(), logits.numpy(), logits2.numpy()
    np.savez_compressed(os.path.join(HERE, 'adv_golden.npz'), **out)
    for k, v in out.items():
        print(k, getattr(v, 'shape', v))


if __name__ == '__main__':
    main()
