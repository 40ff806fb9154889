"""Mixed sample rates in one batch on the device (features.model_glue.MixedRateFeatureBatch / get_batch_full,
features.ensemble.MixedRateEnsembleBatch; dsp_model_*_placed_batch, dsp_gather_clips_batch).

Bars, all the project's own: 1e-4 (normwise) against the oracle or a golden of the real reference; 5e-5 between two device
routes for the same clip (the bar of test_model_feature_batch_reads_the_clips_in_place: a gathered buffer can change a
clip's alignment and with it the in-place / copy route, and the fp64 atomic sums are order dependent); integers (len0,
endpoints, pred, used, valid) exact; pure copies and placements array_equal; softmax within 2^-24.

Not covered here: "run returns before queued device work ends".  run ends with the one host synchronisation that brings
len0 and the endpoints back, so it cannot return early by design, and the existing check
(test_pipeline_launch_does_not_wait_for_the_device) is written inline around VadMfccPipeline.launch: there is no helper to
reuse from a new file."""
import random

import numpy as np
import pytest

from conftest import normwise, record
from golden_cases import case_by_name, make_signal
from oracle import dsp_oracle

pytestmark = pytest.mark.gpu

SENT = np.float32(-7.5e33)               # never a result
SENT32 = np.int32(0x7fc0beef)
C = 13


@pytest.fixture(scope='module')
def env():
    import types

    import torch
    from features import _native as nat
    nat.require_device()
    return types.SimpleNamespace(nat=nat, lib=nat.load(), torch=torch, dev=torch.device('cuda', 0))


def _dev(env, a):
    return env.torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)


def _offsets(clips):
    return np.concatenate(([0], np.cumsum([len(c) for c in clips]))).astype(np.int64)


def _oracle_rows(clip, rate, jitter=None):
    (m0, m1, m2), n = dsp_oracle.model_pipeline(clip, rate, jitter=jitter)
    return np.concatenate([m0, m1, m2], axis=1)[:200], min(n, 200)


SIX_RATES = [44100, 48000, 44100, 48000, 48000, 44100]


@pytest.fixture(scope='module')
def six():
    """Six clips of 0.9-1.4 s interleaved 44.1 / 48 / 44.1 / 48 / 48 / 44.1 kHz, the oracle's rows per clip, and the rows of
    one ModelFeatureBatch run per rate on the sub-batches (host int16): computed once, shared, never changed."""
    import types

    from features.model_glue import ModelFeatureBatch
    secs = [0.9, 1.0, 1.1, 1.2, 1.3, 1.4]
    clips = [make_signal(('vad', 700 + i, int(s * r) + 37 * i + 1, r, 0.6)) for i, (s, r) in enumerate(zip(secs, SIX_RATES))]
    oracle = [_oracle_rows(c, r) for c, r in zip(clips, SIX_RATES)]
    B = len(clips)
    rows, len0, ends = np.zeros((200, B, 39), dtype=np.float32), np.zeros(B, dtype=np.int64), np.zeros((B, 2), dtype=np.int64)
    for rate in (44100, 48000):
        idx = [b for b in range(B) if SIX_RATES[b] == rate]
        sub = [clips[b] for b in idx]
        inp, l0, ep = ModelFeatureBatch(rate).run(np.concatenate(sub), _offsets(sub))
        rows[:, idx], len0[idx], ends[idx] = inp.cpu().numpy(), l0, ep
    for a in (rows, len0, ends):
        a.setflags(write=False)
    return types.SimpleNamespace(clips=clips, rates=SIX_RATES, so=_offsets(clips), flat=np.concatenate(clips), oracle=oracle,
                                 rows=rows, len0=len0, ends=ends)


def _check_against_per_rate(tag, six, inp, len0, ends, order=None):
    order = list(range(len(six.clips))) if order is None else order
    got = inp.cpu().numpy()
    assert got.shape == (200, len(order), 39) and np.isfinite(got).all()
    assert np.array_equal(len0, six.len0[order]) and np.array_equal(ends, six.ends[order])
    for k, b in enumerate(order):
        err = record(f'mixed_{tag}_vs_per_rate', normwise(got[:, k], six.rows[:, b]))
        assert err <= 5e-5, (tag, b, err)
    return got


# ---- 1: placement ----
T_LIST = [0, 1, 7, 199, 200, 201, 260]         # empty, shorter than the delta halo, either side of max_len
DST_COL = [3, 1, 7, 5, 2, 6, 4]                # a permutation of 1..7: columns 0 and 8 of the 9 stay untouched


def _placed_target(env, width=44, n_cols=9):
    out = env.torch.full((200, n_cols, width), float(SENT), dtype=env.torch.float32, device=env.dev)
    len0 = env.torch.full((n_cols,), int(SENT32), dtype=env.torch.int32, device=env.dev)
    return out, len0


def _check_placed(env, out, want, col_offset, what):
    """``want`` [200, n, w] sits at out[:, DST_COL, col_offset:col_offset + w]; everything else is the sentinel."""
    env.torch.cuda.synchronize(env.dev)
    got = out.cpu().numpy()
    w = want.shape[2]
    mask = np.zeros(got.shape, dtype=bool)
    for b, col in enumerate(DST_COL):
        assert np.array_equal(got[:, col, col_offset:col_offset + w], want[:, b]), (what, b)
        mask[:, col, col_offset:col_offset + w] = True
    assert np.all(got[~mask].view(np.int32) == SENT.view(np.int32)), f'{what}: an element outside the placed blocks was written'


def test_placement_is_exact_and_touches_nothing_else(env):
    torch, nat, lib = env.torch, env.nat, env.lib
    n = len(T_LIST)
    fo = np.concatenate(([0], np.cumsum(T_LIST))).astype(np.int64)
    rng = np.random.default_rng(11)
    d_cep = _dev(env, rng.standard_normal((int(fo[-1]), C)).astype(np.float32))
    d_fo, d_col = _dev(env, fo), _dev(env, np.array(DST_COL, dtype=np.int32))
    # the in-place source: segments [n, 2] and the unit-variance sums (sum x, sum x^2) at the start of the work buffer
    seg = np.stack([np.zeros(n, dtype=np.int64), 1000 + 100 * np.arange(n, dtype=np.int64)], axis=1)
    nsamp = (seg[:, 1] - seg[:, 0]).astype(np.float64)
    stats = np.stack([0.25 * nsamp, (2.0 + np.arange(n)) * nsamp], axis=1)
    d_seg, d_stats = _dev(env, seg), _dev(env, stats)
    for source in ('copy', 'in_place'):
        want = torch.empty((200, n, 3 * C), dtype=torch.float32, device=env.dev)
        want_len = torch.empty(n, dtype=torch.int32, device=env.dev)
        if source == 'copy':
            nat.check(lib.dsp_model_finalize_batch(d_cep.data_ptr(), C, d_fo.data_ptr(), n, C, 3, 200, want.data_ptr(),
                                                   want_len.data_ptr(), None))
            p_seg, p_work = None, None
        else:
            nat.check(lib.dsp_model_finalize_segments_batch(d_cep.data_ptr(), C, d_fo.data_ptr(), d_seg.data_ptr(), d_stats.data_ptr(),
                                                            n, C, 3, 200, want.data_ptr(), want_len.data_ptr(), None))
            p_seg, p_work = d_seg.data_ptr(), d_stats.data_ptr()
        out, len0 = _placed_target(env)
        nat.check(lib.dsp_model_finalize_placed_batch(d_cep.data_ptr(), C, d_fo.data_ptr(), p_seg, p_work, n, C, 3, 200, out.data_ptr(),
                                                      len0.data_ptr(), d_col.data_ptr(), 9, 44, 2, None))
        _check_placed(env, out, want.cpu().numpy(), 2, 'finalize/' + source)
        got_len, w_len = len0.cpu().numpy(), want_len.cpu().numpy()
        assert w_len.tolist() == [min(t, 200) for t in T_LIST]
        assert got_len[DST_COL].tolist() == w_len.tolist() and got_len[0] == SENT32 and got_len[8] == SENT32
        # NULL dst_col = identity: the unplaced call's bits in columns 0..n-1 of a wider tensor
        out, len0 = _placed_target(env)
        nat.check(lib.dsp_model_finalize_placed_batch(d_cep.data_ptr(), C, d_fo.data_ptr(), p_seg, p_work, n, C, 3, 200, out.data_ptr(),
                                                      len0.data_ptr(), None, 9, 44, 5, None))
        torch.cuda.synchronize(env.dev)
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :n, 5:44], want.cpu().numpy())
        assert np.all(got[:, n:].view(np.int32) == SENT.view(np.int32)) and np.all(got[:, :, :5].view(np.int32) == SENT.view(np.int32))
        assert len0.cpu().numpy()[:n].tolist() == w_len.tolist()
    # the two optional-stream kernels, the same way
    d_amp = _dev(env, rng.uniform(50.0, 900.0, int(fo[-1])))
    d_pitch = _dev(env, rng.uniform(60.0, 400.0, int(fo[-1])))
    want = torch.empty((200, n, 2), dtype=torch.float32, device=env.dev)
    nat.check(lib.dsp_model_timefeat_batch(d_amp.data_ptr(), d_fo.data_ptr(), n, 1323, 200, want.data_ptr(), None))
    out, _ = _placed_target(env)
    nat.check(lib.dsp_model_timefeat_placed_batch(d_amp.data_ptr(), d_fo.data_ptr(), n, 1323, 200, out.data_ptr(), d_col.data_ptr(),
                                                  9, 44, 41, None))
    _check_placed(env, out, want.cpu().numpy(), 41, 'timefeat')
    nat.check(lib.dsp_model_pitchfeat_batch(d_pitch.data_ptr(), d_fo.data_ptr(), n, 200, want.data_ptr(), None))
    out, _ = _placed_target(env)
    nat.check(lib.dsp_model_pitchfeat_placed_batch(d_pitch.data_ptr(), d_fo.data_ptr(), n, 200, out.data_ptr(), d_col.data_ptr(),
                                                   9, 44, 39, None))
    _check_placed(env, out, want.cpu().numpy(), 39, 'pitchfeat')


# ---- 2: gather ----
@pytest.mark.parametrize('dtype', [np.int16, np.float32])
def test_gather_is_a_copy(env, dtype):
    torch, nat, lib = env.torch, env.nat, env.lib
    lens = [1001, 777, 5, 4099, 12345]                     # odd lengths: every clip after the first starts at an odd offset
    so = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    picks = [3, 0, 4]
    dst_off = np.concatenate(([0], np.cumsum([lens[p] for p in picks]))).astype(np.int64)
    rng = np.random.default_rng(5)
    src = rng.integers(-30000, 30000, int(so[-1])).astype(dtype)
    code = nat.WAVE_I16 if dtype == np.int16 else nat.WAVE_F32
    sent = dtype(-12321)
    tdtype = torch.int16 if dtype == np.int16 else torch.float32
    d_so, d_pick, d_dst = _dev(env, so), _dev(env, np.array(picks, dtype=np.int32)), _dev(env, dst_off)
    want = np.concatenate([src[so[p]:so[p + 1]] for p in picks])
    guard = 64
    # (source shift, destination shift) in elements: equal misalignments (the 16-byte body) and unequal ones
    for s_shift, d_shift in ((0, 0), (1, 1), (2, 2), (3, 3), (1, 0), (0, 3), (2, 1), (3, 2)):
        d_src = torch.zeros(len(src) + s_shift, dtype=tdtype, device=env.dev)
        d_src[s_shift:].copy_(_dev(env, src))
        d_out = torch.full((guard + d_shift + len(want) + guard,), sent.item(), dtype=tdtype, device=env.dev)
        view_in, view_out = d_src[s_shift:], d_out[guard + d_shift:]
        nat.check(lib.dsp_gather_clips_batch(view_in.data_ptr(), code, d_so.data_ptr(), d_pick.data_ptr(), len(picks),
                                             d_dst.data_ptr(), view_out.data_ptr(), None))
        torch.cuda.synchronize(env.dev)
        got = d_out.cpu().numpy()
        lo = guard + d_shift
        assert np.array_equal(got[lo:lo + len(want)], want), (s_shift, d_shift)
        assert np.all(got[:lo] == sent) and np.all(got[lo + len(want):] == sent), (s_shift, d_shift)
    nat.check(lib.dsp_gather_clips_batch(view_in.data_ptr(), code, d_so.data_ptr(), d_pick.data_ptr(), 0, d_dst.data_ptr(),
                                         view_out.data_ptr(), None))          # n_pick = 0: nothing to do


# ---- 3: the real reference's rows ----
def test_two_rates_in_one_call_against_the_reference(golden):
    from features.model_glue import MixedRateFeatureBatch
    c44, c48 = case_by_name('model_feat_44k'), case_by_name('model_feat_48k')
    clips = [make_signal(c44['sig']), make_signal(c48['sig']), make_signal(('vad', 72, 17601, 16000, 0.6))]
    rates = [44100, 48000, 16000]
    inp, len0, ends = MixedRateFeatureBatch().run(clips, None, rates)
    got = inp.cpu().numpy()
    assert got.shape == (200, 3, 39)
    for b, name in enumerate(('model_feat_44k', 'model_feat_48k')):
        n = int(golden[f'{name}/len'][0])
        assert len0[b] == n
        for key, col in (('m0', 0), ('m1', 13), ('m2', 26)):
            err = record(f'mixed_{name}_{key}', normwise(got[:n, b, col:col + 13], golden[f'{name}/{key}'][:n]))
            assert err <= 1e-4, (name, key, err)
        assert not got[n:, b].any()
    ref, n = _oracle_rows(clips[2], 16000)
    assert len0[2] == n and record('mixed_16k_vs_oracle', normwise(got[:n, 2], ref[:n])) <= 1e-4
    for b, (c, r) in enumerate(zip(clips, rates)):               # endpoints in samples of each clip's own rate
        lo, hi = dsp_oracle.basic_endpoint_detection(c, r)
        assert (min(lo, len(c)), min(hi, len(c))) == tuple(ends[b])


# ---- 4: mixed equals per-rate ----
def test_mixed_equals_per_rate_host(six):
    from features.model_glue import MixedRateFeatureBatch
    mr = MixedRateFeatureBatch()
    inp, len0, ends = mr.run(six.flat, six.so, six.rates)
    got = _check_against_per_rate('host', six, inp, len0, ends)
    for b, (ref, n) in enumerate(six.oracle):
        assert len0[b] == n
        assert record('mixed_host_vs_oracle', normwise(got[:n, b], ref[:n])) <= 1e-4, b
        assert not got[n:, b].any()
    # 1323 / 441 and 1440 / 480: each clip's frame count comes from its own rate's framing (round half up)
    for b, (c, r) in enumerate(zip(six.clips, six.rates)):
        L, S = {44100: (1323, 441), 48000: (1440, 480)}[r]
        nsamp = int(ends[b, 1] - ends[b, 0])
        assert len0[b] == min(200, 1 if nsamp <= L else 1 + -(-(nsamp - L) // S))
    inp2, len2, ends2 = mr.run(six.clips, None, six.rates)       # the same batch as a list of clips, cached plan
    assert np.array_equal(len2, len0) and np.array_equal(ends2, ends)
    _check_against_per_rate('host_list', six, inp2, len2, ends2)


@pytest.mark.parametrize('form', ['gather', 'view', 'float32', 'channel'])
def test_mixed_equals_per_rate_device(env, six, form):
    from features.model_glue import MixedRateFeatureBatch, group_by_rate
    order = list(range(6))
    if form == 'view':                     # grouped by rate on the device: each group is a view with rebased offsets
        order = [0, 2, 5, 1, 3, 4]
    clips = [six.clips[b] for b in order]
    rates = [six.rates[b] for b in order]
    assert all(g.contiguous for g in group_by_rate(rates)) == (form == 'view')
    flat, so = np.concatenate(clips), _offsets(clips)
    if form == 'float32':
        waves = _dev(env, flat.astype(np.float32))
    elif form == 'channel':                # reader.py:80 takes sig[:, 0] of a stereo file
        waves = _dev(env, np.stack([flat, -flat], axis=1))[:, 0]
        assert not waves.is_contiguous()
    else:
        waves = _dev(env, flat)
    inp, len0, ends = MixedRateFeatureBatch().run(waves, so, rates)
    _check_against_per_rate('device_' + form, six, inp, len0, ends, order)


# ---- 5: one rate, and a group of one clip ----
def test_single_rate_and_single_clip_group(env):
    from features.model_glue import MixedRateFeatureBatch, ModelFeatureBatch
    clips = [make_signal(('vad', 720 + i, 40000 + 4001 * i, 44100, 0.6)) for i in range(4)]
    flat, so = np.concatenate(clips), _offsets(clips)
    want, wlen, wends = ModelFeatureBatch(44100).run(flat, so)
    mr = MixedRateFeatureBatch()
    for waves in (flat, _dev(env, flat)):
        inp, len0, ends = mr.run(waves, so, [44100] * 4)
        assert np.array_equal(len0, wlen) and np.array_equal(ends, wends)
        for b in range(4):
            assert record('mixed_single_rate', normwise(inp[:, b].cpu().numpy(), want[:, b].cpu().numpy())) <= 5e-5
    # exactly one 48 kHz clip among the four 44.1 kHz ones
    lone = make_signal(('vad', 730, 50001, 48000, 0.6))
    mixed = clips[:2] + [lone] + clips[2:]
    rates = [44100, 44100, 48000, 44100, 44100]
    l_inp, l_len, l_ends = ModelFeatureBatch(48000).run(lone, np.array([0, len(lone)]))
    for waves, so5 in ((mixed, None), (_dev(env, np.concatenate(mixed)), _offsets(mixed))):
        inp, len0, ends = mr.run(waves, so5, rates)
        assert inp.shape == (200, 5, 39)
        assert len0.tolist() == wlen[:2].tolist() + l_len.tolist() + wlen[2:].tolist()
        assert np.array_equal(ends, np.concatenate([wends[:2], l_ends, wends[2:]]))
        got = inp.cpu().numpy()
        for k, b in ((0, 0), (1, 1), (3, 2), (4, 3)):
            assert record('mixed_single_clip_group', normwise(got[:, k], want[:, b].cpu().numpy())) <= 5e-5
        assert record('mixed_single_clip_group', normwise(got[:, 2], l_inp[:, 0].cpu().numpy())) <= 5e-5


# ---- 6: the training path ----
def test_get_batch_full_training_path(golden):
    from features import get_batch_full
    case = case_by_name('model_feat_jitter_44k')
    clip = make_signal(case['sig'])
    other = make_signal(('vad', 78, 55001, 48000, 0.5))
    stereo = np.stack([other, other[::-1]], axis=1)                      # reader.py:80: sig[:, 0], a strided view
    inp, len0 = get_batch_full([(clip, 44100), (stereo[:, 0], 48000)], augment=True, rng=random.Random(case['kw']['seed']))
    assert isinstance(len0, np.ndarray) and len0.shape == (2,) and inp.is_cuda and inp.shape == (200, 2, 39)
    got = inp.cpu().numpy()
    n = int(golden['model_feat_jitter_44k/len'][0])
    assert len0[0] == n
    for key, col in (('m0', 0), ('m1', 13), ('m2', 26)):
        err = record('mixed_jitter_44k_' + key, normwise(got[:n, 0, col:col + 13], golden[f'model_feat_jitter_44k/{key}'][:n]))
        assert err <= 1e-4, (key, err)
    gen = random.Random(case['kw']['seed'])
    gen.randint(0, int(0.1 * 44100)), gen.randint(0, int(0.1 * 44100))   # clip 0's two draws
    jit = (gen.randint(0, int(0.1 * 48000)), gen.randint(0, int(0.1 * 48000)))
    ref, n1 = _oracle_rows(other, 48000, jitter=jit)
    assert len0[1] == n1 and record('mixed_jitter_48k_vs_oracle', normwise(got[:n1, 1], ref[:n1])) <= 1e-4
    # the test path of the same function: no jitter, other endpoints
    inp0, len00 = get_batch_full([(clip, 44100), (other, 48000)])
    ref0, n0 = _oracle_rows(other, 48000)
    assert len00[1] == n0 and normwise(inp0[:n0, 1].cpu().numpy(), ref0[:n0]) <= 1e-4


# ---- 7: optional streams ----
def test_optional_streams_at_three_rates():
    from features.model_glue import MixedRateFeatureBatch
    rates = [44100, 48000, 22050]
    clips = [make_signal(('vad', 740 + i, int((1.0 + 0.1 * i) * r) + 3, r, 0.6)) for i, r in enumerate(rates)]
    mr = MixedRateFeatureBatch()
    base, len_b, _ = mr.run(clips, None, rates)
    inp, len0, ends = mr.run(clips, None, rates, use_pitch=True, use_timefeat=True)
    assert inp.shape == (200, 3, 43) and np.array_equal(len0, len_b)
    got = inp.cpu().numpy()
    assert np.array_equal(got[:, :, :39], base.cpu().numpy())
    for b, (c, rate) in enumerate(zip(clips, rates)):
        lo, hi = dsp_oracle.basic_endpoint_detection(c, rate)
        assert (min(lo, len(c)), min(hi, len(c))) == tuple(ends[b])
        sound = dsp_oracle.model_endpoint_scale(c, lo, hi)
        a0, a1 = dsp_oracle.model_feature_extract_timespace(sound, rate)
        n0, n1 = min(len(a0), 200), min(len(a1), 200)
        assert record('mixed_timefeat', normwise(got[:n0, b, 41], a0[:n0, 0])) <= 1e-4
        assert not got[n0:, b, 41].any()                     # the stream's own frame count, zero padded beyond
        assert record('mixed_timefeat_diff', normwise(got[:n1, b, 42], a1[:n1, 0])) <= 1e-4 and not got[n1:, b, 42].any()
        p0, p1 = dsp_oracle.model_feature_extract_pitch(sound, rate)
        m0, m1 = min(len(p0), 200), min(len(p1), 200)
        same = np.isclose(got[:m0, b, 39], p0[:m0, 0], rtol=1e-5, atol=1e-6)
        assert same.mean() >= 0.98, (b, same.mean())         # fp32 clip vs fp64 clip: an arg-max may flip on a near tie
        assert not got[m0:, b, 39].any() and not got[m1:, b, 40].any()
        assert np.allclose(got[:m1, b, 40], got[1:m1 + 1, b, 39] - got[:m1, b, 39], rtol=0, atol=2e-6)
    only_amp, _, _ = mr.run(clips, None, rates, use_timefeat=True)
    assert only_amp.shape == (200, 3, 41) and np.array_equal(only_amp.cpu().numpy(), got[:, :, list(range(39)) + [41, 42]])


# ---- 8: graph ----
def test_graph_replays_on_new_data(env):
    torch = env.torch
    from features.model_glue import MixedRateFeatureBatch
    rates = [44100, 48000, 44100, 48000]
    lens = [int((0.9 + 0.1 * i) * r) + 5 for i, r in enumerate(rates)]
    clips_a = [make_signal(('vad', 750 + i, n, r, 0.6)) for i, (n, r) in enumerate(zip(lens, rates))]
    clips_b = [make_signal(('vad', 760 + i, n, r, 0.45)) for i, (n, r) in enumerate(zip(lens, rates))]
    so = _offsets(clips_a)
    buf = _dev(env, np.concatenate(clips_a))
    mr = MixedRateFeatureBatch()
    g = mr.capture(buf, so, rates)
    for clips in (clips_a, clips_b):
        buf.copy_(torch.from_numpy(np.concatenate(clips)))
        inp, len0 = g.replay()
        torch.cuda.synchronize(env.dev)
        eager, elen, _ = MixedRateFeatureBatch().run(_dev(env, np.concatenate(clips)), so, rates)
        assert np.array_equal(len0.cpu().numpy(), elen)
        for b in range(4):
            assert record('mixed_graph_vs_eager', normwise(inp[:, b].cpu().numpy(), eager[:, b].cpu().numpy())) <= 5e-5
    with pytest.raises(ValueError, match='contiguous'):
        mr.capture(_dev(env, np.stack([np.concatenate(clips_a)] * 2, axis=1))[:, 0], so, rates)
    with pytest.raises(TypeError, match='device tensor'):
        mr.capture(np.concatenate(clips_a), so, rates)


# ---- 9: ensemble ----
def _toy_svm(seed, classes, n_sv=40):
    from features.ensemble import PitchSVM
    rng = np.random.default_rng(seed)
    return PitchSVM.from_arrays(rng.standard_normal((n_sv, 5)), rng.uniform(-1, 1, n_sv), rng.uniform(-0.2, 0.2), 0.1, classes,
                                scale=rng.uniform(0.5, 2.0, 5), center=rng.standard_normal(5))


def test_ensemble_on_a_mixed_batch(env, six):
    torch = env.torch
    from features.classifier import HMRNNHead, fill_parameters
    from features.ensemble import REFERENCE_RULES, EnsembleBatch, MixedRateEnsembleBatch
    head = HMRNNHead().to(env.dev)
    fill_parameters(head, 3)
    # the reference's two rules, and two more so that more of the 20 labels are gated (a seeded head is far from confident)
    rules = [(pair, thr, _toy_svm(20 + k, pair)) for k, (pair, thr) in enumerate(REFERENCE_RULES)]
    rules += [((2, 3), 0.9, _toy_svm(30, (2, 3))), ((12, 13), 0.9, _toy_svm(31, (12, 13)))]
    with torch.no_grad():
        out = MixedRateEnsembleBatch(head, rules).run(six.flat, six.so, six.rates, dropout=False)
    B = len(six.clips)
    logits = out.logits
    assert tuple(logits.shape) == (B, 20) and bool(torch.isfinite(logits).all())
    assert np.array_equal(out.endpoints, six.ends) and np.array_equal(out.len0, six.len0)
    pred, used, valid = out.pred.cpu().numpy(), out.used.cpu().numpy(), out.valid.cpu().numpy()
    prob, feat = out.prob.cpu().numpy().astype(np.float64), out.feat.cpu().numpy()
    for rate in (44100, 48000):
        idx = [b for b in range(B) if six.rates[b] == rate]
        sub = [six.clips[b] for b in idx]
        per = EnsembleBatch(rate, lambda inp, len0, idx=idx: logits[idx], rules).run(np.concatenate(sub), _offsets(sub))
        assert np.array_equal(pred[idx], per.pred.cpu().numpy()) and np.array_equal(used[idx], per.used.cpu().numpy())
        p_valid = per.valid.cpu().numpy()
        assert np.array_equal(valid[idx], p_valid)
        err = record('mixed_ensemble_prob', float(np.max(np.abs(prob[idx] - per.prob.cpu().numpy().astype(np.float64)))))
        assert err <= 2.0 ** -24
        ok = p_valid != 0
        assert np.array_equal(feat[idx][ok], per.feat.cpu().numpy()[ok])
    want = torch.softmax(logits.double(), 1).cpu().numpy()
    assert float(np.max(np.abs(prob - want))) <= 2.0 ** -24
    # the same batch from the device, interleaved (the gather route)
    with torch.no_grad():
        out_d = MixedRateEnsembleBatch(head, rules).run(_dev(env, six.flat), six.so, six.rates, dropout=False)
    assert np.array_equal(out_d.endpoints, six.ends) and np.array_equal(out_d.valid.cpu().numpy(), valid)
    assert np.array_equal(out_d.feat.cpu().numpy()[valid != 0], feat[valid != 0])
