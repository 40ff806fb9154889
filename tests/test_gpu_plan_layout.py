"""GPU parity of the compile-time plan layouts of the NFFT-512 kernels (kernels_fast512.h, F512Tag): the two standard
plans -- the metric plan (40 filters) and the reference's defaults (26 filters) -- run instantiations that hold the
layout fields of F512Params as constants; every other plan reads them from its arguments.  What can go wrong is a plan
taking a tag whose constants are not its own, or a tag's constants disagreeing with the table blob, so the cases are the
two tagged plans, plans that keep their tag because only run-time fields or table CONTENTS differ (preemph, ceplifter),
and the nearest neighbours that must not take one (another C, M, S, L, appendEnergy off).

Every case, fp32 and int16, at the smallest batches that reach each path:
  * the dense MFCC-only kernel at B = 3, N = 9360 (T = 57, flat grouping with a seam in every other group), into a
    NaN-filled buffer, two utterances against the oracle;
  * the fused MFCC + delta + delta-delta kernel at B = 2 x CUs (512 on an MI355X), N = 9360 -- the smallest batch
    fast512_launch_fused_t serves -- equal, bit for bit and into NaN-filled buffers, to the MFCC kernel followed by
    dsp_delta_batch, and two utterances against the oracle.  On a device with more CUs dsp_mfcc_delta_batch takes the
    two-kernel path itself and the comparison holds trivially, as in test_gpu_fused_delta_runs.py.
The bar against the oracle is the project's: normwise <= 1e-4 (TOL of the fused tests)."""
import numpy as np
import pytest

from conftest import normwise
from oracle import dsp_oracle

pytestmark = pytest.mark.gpu

CFG = dict(samplerate=16000, winlen=0.025, winstep=0.01, numcep=13, nfilt=40, nfft=512, lowfreq=0,
           highfreq=None, preemph=0.97, ceplifter=22, appendEnergy=True)
TOL = 1e-4
N = 9360

# name -> (overrides of CFG, frames per utterance)
CASES = {
    'metric_plan': ({}, 57),                                # tag 1
    'default_26_filters': (dict(nfilt=26), 57),             # tag 2
    'preemph_0.95': (dict(preemph=0.95), 57),               # tag 1: the coefficient is a run-time field
    'no_lifter': (dict(ceplifter=0), 57),                   # tag 1: same layout, other table contents
    'numcep_12': (dict(numcep=12), 57),                     # neighbours: no tag
    'nfilt_39': (dict(nfilt=39), 57),                       # ... fits the 40-filter block table, is not the metric plan
    'nfilt_25': (dict(nfilt=25), 57),
    'hop_120': (dict(winstep=0.0075), 76),
    'window_320': (dict(winlen=0.02), 58),
    'no_energy': (dict(appendEnergy=False), 57),
}

_PLANS = {}
_BATCHES = {}


def _plan(name):
    from features.batch import FeaturePlan
    if name not in _PLANS:
        cfg = dict(CFG, **CASES[name][0])
        _PLANS[name] = (FeaturePlan(winfunc=np.hamming, **cfg), cfg)
    return _PLANS[name]


def _batch(seed, B, dtype):
    """Made once per (seed, B, dtype) and shared by the cases; never written to."""
    key = (seed, B, np.dtype(dtype).name)
    if key not in _BATCHES:
        x = np.random.default_rng(seed).standard_normal((B, N))
        if dtype == np.int16:
            w = np.clip(np.round(3000 * x), -32768, 32767).astype(np.int16)
        else:
            w = (0.25 * x).astype(np.float32)
        _BATCHES[key] = w
    return _BATCHES[key]


def _wave_dtype(waves):
    from features import _native as nat
    return nat.WAVE_I16 if waves.dtype == np.int16 else nat.WAVE_F32


def _mfcc_only(plan, waves):
    """[B T, C] rows of the dense MFCC kernel, into a NaN-filled buffer."""
    import torch
    from features import _native as nat
    B = waves.shape[0]
    C = plan.C
    T = plan.layout(waves).total_frames // B
    dev = torch.device('cuda', 0)
    d_wave = torch.from_numpy(waves).to(dev)
    out = torch.full((B * T, C), float('nan'), device=dev)
    nat.check(nat.load().dsp_features_batch(plan.plan.handle, d_wave.data_ptr(), _wave_dtype(waves), None, None, B, B * T,
                                            N, nat.OUT_MFCC, out.data_ptr(), C, None, None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), T


def _fused_and_two_kernel(plan, waves, delta_n):
    """Rows of the fused launch and of the MFCC kernel + dsp_delta_batch, both into NaN-filled buffers."""
    import torch
    from features import _native as nat
    lib = nat.load()
    B = waves.shape[0]
    C = plan.C
    lay = plan.layout(waves)
    T = lay.total_frames // B
    dev = torch.device('cuda', 0)
    d_wave = torch.from_numpy(waves).to(dev)
    wd = _wave_dtype(waves)
    fused = torch.full((B * T, 3 * C), float('nan'), device=dev)
    plan.run_raw(d_wave.data_ptr(), wd, lay, fused.data_ptr(), delta_n, None)
    two = torch.full((B * T, 3 * C), float('nan'), device=dev)
    nat.check(lib.dsp_features_batch(plan.plan.handle, d_wave.data_ptr(), wd, None, None, B, B * T, N, nat.OUT_MFCC,
                                     two.data_ptr(), 3 * C, None, None))
    nat.check(lib.dsp_delta_batch(two.data_ptr(), 3 * C, None, B, B * T, T, C, delta_n, two.data_ptr() + C * 4, 3 * C,
                                  two.data_ptr() + 2 * C * 4, 3 * C, None))
    torch.cuda.synchronize()
    return fused.cpu().numpy(), two.cpu().numpy(), T


def _fused_batch():
    """2 x CUs utterances: the smallest batch the fused form serves on this device."""
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize('dtype', [np.float32, np.int16], ids=['fp32', 'int16'])
@pytest.mark.parametrize('name', list(CASES))
def test_dense_mfcc_only(name, dtype):
    plan, cfg = _plan(name)
    waves = _batch(301, 3, dtype)
    got, T = _mfcc_only(plan, waves)
    assert T == CASES[name][1], T
    assert got.shape == (3 * T, cfg['numcep']) and np.isfinite(got).all()
    for b in (0, 2):
        ref = dsp_oracle.mfcc(waves[b].astype(np.float64), winfunc=np.hamming, **cfg)
        err = normwise(got[b * T:(b + 1) * T], ref)
        print(f'{name} utterance {b}: normwise error against the oracle {err:.3e}')
        assert err <= TOL, (b, err)


@pytest.mark.parametrize('delta_n', [1, 2], ids=['N1', 'N2'])
@pytest.mark.parametrize('dtype', [np.float32, np.int16], ids=['fp32', 'int16'])
@pytest.mark.parametrize('name', list(CASES))
def test_fused_equals_two_kernel_path(name, dtype, delta_n):
    """Both sample types and both delta windows: the four fused instantiations of every tag run."""
    plan, cfg = _plan(name)
    B = _fused_batch()
    waves = _batch(302, B, dtype)
    fused, two, T = _fused_and_two_kernel(plan, waves, delta_n)
    assert T == CASES[name][1], T
    assert fused.shape == (B * T, 3 * cfg['numcep']) and np.isfinite(fused).all()
    assert np.array_equal(fused, two), np.argwhere(fused != two)[:8]
    for b in (1, B - 1):
        ref = dsp_oracle.mfcc_delta(waves[b].astype(np.float64), delta_n=delta_n, winfunc=np.hamming, **cfg)
        err = normwise(fused[b * T:(b + 1) * T], ref)
        print(f'{name} utterance {b}: normwise error against the oracle {err:.3e}')
        assert err <= TOL, (b, err)
