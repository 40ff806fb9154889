"""Mixed sample rates in one batch, the parts that need no GPU: the grouping of a batch by rate, the jitter order of
model.py:55-58, the declarations of the new entry points and their argument checks (every one returns before a launch)."""
import os
import random
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dsp_model_finalize_placed_batch', 'dsp_model_timefeat_placed_batch', 'dsp_model_pitchfeat_placed_batch',
       'dsp_gather_clips_batch')


@pytest.fixture(scope='module')
def nat():
    from features import _native
    _native.load()
    return _native


def test_grouping_by_rate():
    from features.model_glue import group_by_rate
    rates = [44100, 48000, 44100, 16000, 48000]
    groups = group_by_rate(rates)
    assert [g.rate for g in groups] == [44100, 48000, 16000]                        # order of first appearance
    assert [g.index.tolist() for g in groups] == [[0, 2], [1, 4], [3]]              # stable inside a group
    assert all(g.index.dtype == np.int32 for g in groups)
    assert sorted(np.concatenate([g.index for g in groups]).tolist()) == list(range(len(rates)))   # a partition of range(B)
    assert [g.contiguous for g in groups] == [False, False, True]
    groups = group_by_rate([48000, 48000, 44100])
    assert [(g.rate, g.index.tolist(), g.contiguous) for g in groups] == [(48000, [0, 1], True), (44100, [2], True)]
    groups = group_by_rate(np.array([22050] * 4))
    assert len(groups) == 1 and groups[0].index.tolist() == [0, 1, 2, 3] and groups[0].contiguous
    rng = np.random.default_rng(0)
    rates = rng.choice([16000, 44100, 48000], 40)
    groups = group_by_rate(rates)
    assert sorted(np.concatenate([g.index for g in groups]).tolist()) == list(range(40))
    for g in groups:
        assert np.all(rates[g.index] == g.rate) and np.all(np.diff(g.index) > 0)
        assert g.contiguous == (g.index.tolist() == list(range(g.index[0], g.index[-1] + 1)))


@pytest.mark.parametrize('seed', [0, 7, 1234])
def test_draw_jitter_consumes_the_generator_in_the_reference_order(seed):
    from features.model_glue import MixedRateFeatureBatch, ModelFeatureBatch
    rates = [44100, 48000, 44100, 16000, 48000]
    got = MixedRateFeatureBatch.draw_jitter(rates, random.Random(seed))
    gen = random.Random(seed)
    want = []
    for r in rates:                                        # model.py:55-58, clip by clip
        s_l = gen.randint(0, int(0.1 * r))
        s_r = gen.randint(0, int(0.1 * r))
        want.append([-s_l, s_r])
    assert got.dtype == np.int64 and got.shape == (5, 2) and got.tolist() == want
    assert np.all(got[:, 0] <= 0) and np.all(got[:, 1] >= 0)
    # one rate: the sequence of ModelFeatureBatch.draw_jitter (its constructor needs the device, the method does not)
    one = ModelFeatureBatch.draw_jitter(type('R', (), {'rate': 44100})(), 3, random.Random(seed))
    assert MixedRateFeatureBatch.draw_jitter([44100] * 3, random.Random(seed)).tolist() == one.tolist()


def test_entry_points_declared_exported_and_bound(nat):
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    lib = nat.load()
    for name in NEW:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
        assert name in nat.SIGNATURES and hasattr(lib, name)
        decl = re.search(name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        params = [p.strip() for p in decl.split(',')]
        assert len(params) == len(nat.SIGNATURES[name][1]), name                   # one ctypes type per C parameter
        for p, t in zip(params, nat.SIGNATURES[name][1]):
            if '*' in p:
                assert t is nat.c_vp, (name, p)
            elif p.startswith('int32_t'):
                assert t is nat.c_i32, (name, p)
            elif p.startswith('int64_t'):
                assert t is nat.c_i64, (name, p)
            else:
                assert p.startswith('int ') and t is nat.C.c_int, (name, p)
    for name in NEW[:3]:                                                           # the four placement arguments, in order
        decl = re.search(name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        tail = [p.strip() for p in decl.split(',')][-5:]
        assert tail == ['const int32_t* d_dst_col', 'int32_t n_cols', 'int32_t row_width', 'int32_t col_offset', 'void* stream']
    new_part = hdr[hdr.index('/* ---- mixed sample rates'):]
    for cite in ('model.py:114-135', 'reader.py:80', 'model.py:35-50', 'model.py:97-101', 'model.py:90-95'):
        assert cite in new_part, cite
    import features
    assert features.MixedRateFeatureBatch is features.model_glue.MixedRateFeatureBatch
    assert features.MixedRateEnsembleBatch is features.ensemble.MixedRateEnsembleBatch and callable(features.get_batch_full)


def _einval(nat, rc, what):
    msg = nat.load().dsp_last_error().decode()
    assert rc == nat.EINVAL and what in msg, (rc, msg, what)


def test_argument_checks_return_before_any_launch(nat):
    """On this machine there is no device: a check that let a call through would come back as a HIP error, not DSP_EINVAL.
    Under dsp_debug_host_dry_run the new entry points refuse what passed every check instead of launching it."""
    lib = nat.load()
    buf = np.zeros(64, dtype=np.float64)          # pointers that are only checked
    p = buf.ctypes.data
    C = 13
    nat.check(lib.dsp_debug_host_dry_run(1))
    try:
        def fin(mfcc=p, fo=p, seg=None, work=None, n=3, Cn=C, N=3, max_len=200, out=p, len0=p, col=p, n_cols=9, width=44, off=2):
            return lib.dsp_model_finalize_placed_batch(mfcc, Cn, fo, seg, work, n, Cn, N, max_len, out, len0, col, n_cols, width,
                                                       off, None)

        _einval(nat, fin(n_cols=2), 'n_cols')                       # n_cols < n_utt
        _einval(nat, fin(off=-1), 'col_offset')
        _einval(nat, fin(off=6), 'row_width')                       # 6 + 39 > 44
        _einval(nat, fin(width=38, off=0), 'row_width')
        _einval(nat, fin(width=0), 'row_width')
        _einval(nat, fin(out=None), 'NULL')
        _einval(nat, fin(len0=None), 'NULL')
        _einval(nat, fin(mfcc=None), 'NULL')
        _einval(nat, fin(fo=None), 'NULL')
        _einval(nat, fin(n=0), 'n_utt')
        _einval(nat, fin(seg=p), 'go together')                     # segments without the work buffer, and the reverse
        _einval(nat, fin(work=p), 'go together')
        _einval(nat, fin(N=0), 'N must be')                         # the existing checks of the unplaced entry points
        _einval(nat, fin(Cn=33, width=200), 'C <= 32')
        _einval(nat, fin(), 'dry_run')                              # everything valid: refused, not launched
        _einval(nat, fin(col=None, off=5), 'dry_run')               # identity columns, the last offset that fits
        _einval(nat, fin(seg=p, work=p), 'dry_run')

        def tf(amp=p, fo=p, n=3, L=1323, max_len=200, out=p, col=p, n_cols=9, width=44, off=41):
            return lib.dsp_model_timefeat_placed_batch(amp, fo, n, L, max_len, out, col, n_cols, width, off, None)

        def pf(pitch=p, fo=p, n=3, max_len=200, out=p, col=p, n_cols=9, width=44, off=39):
            return lib.dsp_model_pitchfeat_placed_batch(pitch, fo, n, max_len, out, col, n_cols, width, off, None)

        for f in (tf, pf):
            _einval(nat, f(n_cols=2), 'n_cols')
            _einval(nat, f(off=-3), 'col_offset')
            _einval(nat, f(off=43), 'row_width')                    # 43 + 2 > 44
            _einval(nat, f(out=None), 'NULL')
            _einval(nat, f(fo=None), 'NULL')
            _einval(nat, f(n=0), 'n_utt')
            _einval(nat, f(max_len=0), 'max_len')
            _einval(nat, f(off=42), 'dry_run')
            _einval(nat, f(col=None), 'dry_run')
        _einval(nat, tf(amp=None), 'NULL')
        _einval(nat, tf(L=0), 'frame_len')
        _einval(nat, pf(pitch=None), 'NULL')

        def gather(wave=p, dtype=nat.WAVE_I16, so=p, pick=p, n=3, dst=p, out=p):
            return lib.dsp_gather_clips_batch(wave, dtype, so, pick, n, dst, out, None)

        _einval(nat, gather(n=-1), 'n_pick')
        _einval(nat, gather(dtype=2), 'wave_dtype')
        _einval(nat, gather(dtype=-1), 'wave_dtype')
        _einval(nat, gather(out=None), 'NULL')
        _einval(nat, gather(wave=None), 'NULL')
        _einval(nat, gather(so=None), 'NULL')
        _einval(nat, gather(pick=None), 'NULL')
        _einval(nat, gather(dst=None), 'NULL')
        _einval(nat, gather(), 'dry_run')
        _einval(nat, gather(dtype=nat.WAVE_F32, n=0), 'dry_run')
    finally:
        nat.check(lib.dsp_debug_host_dry_run(0))


def test_run_rejects_bad_rates_before_any_device_work():
    from features.model_glue import MixedRateFeatureBatch, get_batch_full
    mr = MixedRateFeatureBatch()
    clips = [np.zeros(2000, dtype=np.int16), np.zeros(3000, dtype=np.int16)]
    flat, so = np.concatenate(clips), np.array([0, 2000, 5000])
    with pytest.raises(ValueError, match='3 rates for 2 clips'):
        mr.run(flat, so, [44100, 48000, 44100])
    with pytest.raises(ValueError, match='1 rates for 2 clips'):
        mr.run(clips, None, [44100])
    for bad in (0, -48000):
        with pytest.raises(ValueError, match='positive'):
            mr.run(flat, so, [44100, bad])
        with pytest.raises(ValueError, match='positive'):
            get_batch_full([(clips[0], 44100), (clips[1], bad)])
    with pytest.raises(ValueError, match='whole'):
        mr.run(clips, None, [44100.5, 48000])
    with pytest.raises(ValueError, match='sample_offsets'):
        mr.run(flat, None, [44100, 48000])
