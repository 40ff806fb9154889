"""GPU parity of the fused MFCC + delta + delta-delta kernel's run structure (kernels_fast512.h, "Fused delta"): a wave
takes a contiguous run of frame groups of a workgroup that owns whole utterances, carries the last staged vector of a
group into the next one, and waits at the workgroup's barrier in its final, computation-free iteration.

Every case compares the fused launch, bit for bit and on outputs pre-filled with NaN, with the MFCC kernel followed by
dsp_delta_batch, and checks two utterances against the oracle.  The shapes are the smallest at which each path can go
wrong: the fused form needs >= 2 x CUs utterances (512 on the 256 CUs of an MI355X) and T >= 57 frames.  On a device
with more CUs, or for a plan the fused form does not serve, dsp_mfcc_delta_batch takes the two-kernel path itself and
the comparison holds trivially; on 256 CUs all shapes below qualify (fast512_launch_fused_t), S = 120 and C = 12 / 14
included."""
import numpy as np
import pytest

from conftest import normwise
from oracle import dsp_oracle

pytestmark = pytest.mark.gpu

CFG = dict(samplerate=16000, winlen=0.025, winstep=0.01, numcep=13, nfilt=40, nfft=512, lowfreq=0,
           highfreq=None, preemph=0.97, ceplifter=22, appendEnergy=True)
TOL = 1e-4

_PLANS = {}


def _plan(**over):
    from features.batch import FeaturePlan
    key = tuple(sorted(over.items()))
    if key not in _PLANS:
        _PLANS[key] = (FeaturePlan(winfunc=np.hamming, **dict(CFG, **over)), dict(CFG, **over))
    return _PLANS[key]


def _batch(seed, B, N, dtype):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        return np.clip(np.round(3000 * rng.standard_normal((B, N))), -32768, 32767).astype(np.int16)
    return (0.25 * rng.standard_normal((B, N))).astype(np.float32)


def _fused_and_two_kernel(plan, waves, delta_n):
    """Rows of the fused launch and of the MFCC kernel + dsp_delta_batch, both into NaN-filled buffers."""
    import torch
    from features import _native as nat
    lib = nat.load()
    B, N = waves.shape
    C = plan.C
    lay = plan.layout(waves)
    T = lay.total_frames // B
    dev = torch.device('cuda', 0)
    d_wave = torch.from_numpy(waves).to(dev)
    wd = nat.WAVE_I16 if waves.dtype == np.int16 else nat.WAVE_F32
    fused = torch.full((B * T, 3 * C), float('nan'), device=dev)
    plan.run_raw(d_wave.data_ptr(), wd, lay, fused.data_ptr(), delta_n, None)
    two = torch.full((B * T, 3 * C), float('nan'), device=dev)
    nat.check(lib.dsp_features_batch(plan.plan.handle, d_wave.data_ptr(), wd, None, None, B, B * T, N, nat.OUT_MFCC,
                                     two.data_ptr(), 3 * C, None, None))
    nat.check(lib.dsp_delta_batch(two.data_ptr(), 3 * C, None, B, B * T, T, C, delta_n, two.data_ptr() + C * 4, 3 * C,
                                  two.data_ptr() + 2 * C * 4, 3 * C, None))
    torch.cuda.synchronize()
    return fused.cpu().numpy(), two.cpu().numpy(), T


def _check(plan, cfg, waves, delta_n, T_expected, sampled):
    fused, two, T = _fused_and_two_kernel(plan, waves, delta_n)
    assert T == T_expected, T
    assert np.isfinite(fused).all()
    assert np.array_equal(fused, two), np.argwhere(fused != two)[:8]
    for b in sampled:
        ref = dsp_oracle.mfcc_delta(waves[b].astype(np.float64), delta_n=delta_n, winfunc=np.hamming, **cfg)
        err = normwise(fused[b * T:(b + 1) * T], ref)
        print(f'utterance {b}: normwise error against the oracle {err:.3e}')
        assert err <= TOL, (b, err)
    return fused


@pytest.fixture(scope='module')
def case1():
    """Case 1, computed once: 512 x 1 s, one utterance (13 groups) per workgroup on 8 waves."""
    plan, cfg = _plan()
    waves = _batch(201, 512, 16000, np.float32)
    fused = _check(plan, cfg, waves, 2, 99, (0, 511))
    return waves, fused


def test_one_utterance_per_workgroup_runs_of_one_and_two(case1):
    """13 groups on 8 waves: five waves carry the overlap vector into their second group, three have nothing to
    carry, and the utterance's last, partial group (slow staging) directly follows a carried one."""
    waves, fused = case1
    assert fused.shape == (512 * 99, 39)


def test_minimum_length_one_group_per_wave():
    """T = 57, the shortest the fused form takes: 8 groups on 8 waves, no carry anywhere; only the barrier of the
    final iteration stands between a wave's published first group and its predecessor's read.  int16, window 1."""
    plan, cfg = _plan()
    _check(plan, cfg, _batch(202, 512, 9360, np.int16), 1, 57, (3, 511))


def test_bench_shape_int16():
    """1024 x 1 s of int16: two utterances (25 groups) per workgroup, runs of 3 and 4 groups across the seam."""
    plan, cfg = _plan()
    _check(plan, cfg, _batch(203, 1024, 16000, np.int16), 2, 99, (1, 1022))


def test_seam_inside_a_run():
    """600 x 1.5 s (T = 149) on 512 workgroups of one and two utterances: runs of 2-3 groups in which a carried
    group, the slow-staged group that spans the seam and a freshly staged first group of the next utterance follow
    one another."""
    plan, cfg = _plan()
    _check(plan, cfg, _batch(204, 600, 24000, np.float32), 2, 149, (200, 599))


def test_hop_that_does_not_line_up_with_the_staging_rounds():
    """winstep 7.5 ms: S = 120, 8 S is no multiple of 256, so no staged vector of a group is a round of the next:
    the carry must stay off."""
    plan, cfg = _plan(winstep=0.0075)
    assert plan.S == 120
    _check(plan, cfg, _batch(205, 512, 16000, np.float32), 2, 131, (7, 510))


@pytest.mark.parametrize('numcep', [12, 14])
def test_even_row_widths(numcep):
    """C = 12 and 14 with the energy in column 0: every lane that stores writes a full pair (at C = 14 the lane of
    pair 6 too), rows are 36 and 42 floats wide."""
    plan, cfg = _plan(numcep=numcep)
    fused = _check(plan, cfg, _batch(206, 512, 16000, np.float32), 2, 99, (2, 509))
    assert fused.shape == (512 * 99, 3 * numcep)


@pytest.mark.parametrize('B,pos', [(512, 511), (1024, 700)])
def test_rows_do_not_depend_on_where_the_utterance_sits(case1, B, pos):
    """Sharding invariance: utterance 0 of case 1 as the last utterance of a 512-batch and as utterance 700 of a
    1024-batch (first of a two-utterance workgroup: another cut of the runs, other groups carried).  Same bits."""
    plan, cfg = _plan()
    waves1, fused1 = case1
    waves = _batch(207 + B, B, 16000, np.float32)
    waves[pos] = waves1[0]
    fused = _check(plan, cfg, waves, 2, 99, (pos, B - 1 if pos != B - 1 else 0))
    assert np.array_equal(fused[pos * 99:(pos + 1) * 99], fused1[:99])
