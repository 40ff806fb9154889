"""The cepstral pitch path on the device (pitch.pitch_detect, pitch.pitch_feature and their batched forms) against the
stored reference outputs (tests/golden/pitch_cepstrum_golden.npz) and, for random batches, against the NumPy
restatement that reproduces them (tests/pitch_cepstrum_ref.py).

Bounds: rows 1e-4 normwise per frame (the project's parity bar), over the whole row and over columns 1 .. L-1 alone
(column 0 is the row's maximum and would mask the quefrencies that matter); at most 1 % of the frames of a track may
differ from the reference (integer peak widths come from fp32 comparisons; the reference's own arithmetic in fp32
sits at 0 %, tests/golden/pitch_cepstrum_manifest.json) and at least 10 of 12 tracks are identical; where the track is
identical, features agree within 1e-9 max(1, |ref|) (the reference itself returns -6e-15 where a fit is exactly 0) with
p and the segments exact."""
import os

import numpy as np
import pytest

import pitch_cepstrum_ref as ref
from conftest import record
from pitch_cepstrum_cases import CASES, CHIRPS, L10, ROWS_CASES, S10, make_input, random_chirp_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 4096
SENT32 = np.int32(0x7fc0beef)            # a quiet-NaN pattern: never a result


@pytest.fixture(scope='module')
def pgold():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'pitch_cepstrum_golden.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def fp():
    from features import _native as nat
    from features import pitch
    nat.require_device()
    return pitch


def _case(name):
    return next(c for c in CASES if c['name'] == name)


def _gold(pgold, name):
    return {k.split('/', 1)[1]: v for k, v in pgold.items() if k.startswith(name + '/')}


def _so(clips):
    return np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)


def _feat_close(got, want):
    return bool(np.all(np.abs(np.asarray(got) - want) <= 1e-9 * np.maximum(1.0, np.abs(want))))


def _aux_matches(aux, seg, fo_b, g):
    """aux row / accepted values of one utterance against a reference dict with p, idx1, idx2, seg1, seg2."""
    p, p_bias, a1, b1, a2, b2, m1, m2, valid = (int(v) for v in aux)
    assert valid == 1
    assert p == int(g['p']) and p_bias == (5 if p > 15 else 0)
    assert (a1, b1) == tuple(int(v) for v in g['idx1']) and (a2, b2) == tuple(int(v) for v in g['idx2'])
    assert np.array_equal(seg[fo_b + p_bias:fo_b + p_bias + m1], g['seg1'])
    assert np.array_equal(seg[fo_b + p:fo_b + p + m2], g['seg2'])


@pytest.fixture(scope='module')
def tracks(fp, pgold):
    """name -> (pitch, scores) of the device for every case."""
    out = {}
    for c in CASES:
        sig, rate = make_input(c)
        s10 = ref.decimate(sig, rate)
        pitch, scores, fo = fp.pitch_cepstrum_tracks_batch(s10, [0, len(s10)], L10, S10)
        assert len(pitch) == int(pgold[f"{c['name']}/n_frames"]) == fo[-1]
        out[c['name']] = (pitch, scores)
    return out


# ---- 1 ----
@pytest.mark.parametrize('name', ROWS_CASES)
def test_rows_match_the_stored_fp64_rows(name, fp, pgold):
    sig, rate = make_input(_case(name))
    s10 = ref.decimate(sig, rate)
    want = pgold[f'{name}/rows']
    rows, amp, fo = fp.cepstrum_rows_batch(s10, [0, len(s10)], L10, S10)
    assert rows.shape == want.shape
    for t in range(len(want)):
        full = np.max(np.abs(rows[t] - want[t])) / np.max(np.abs(want[t]))
        tail = np.max(np.abs(rows[t, 1:] - want[t, 1:])) / np.max(np.abs(want[t, 1:]))
        print(f'{name} frame {t}: normwise {full:.3e}, columns 1.. {tail:.3e}')
        record('pitch_cepstrum_rows_normwise', full)
        record('pitch_cepstrum_rows_normwise_cols1', tail)
        assert full <= 1e-4 and tail <= 1e-4, (name, t, full, tail)
    # the amplitude stream: sums of |x| of the unclipped frames; the clip reaches the kernel as fp32 (2^-24 per sample)
    F = ref.frames_of(s10, L10, S10)
    want_amp = np.abs(F).sum(axis=1)
    tol = 1e-12 if s10.dtype == np.int16 else 1e-6
    assert np.all(np.abs(amp - want_amp) <= tol * np.maximum(1.0, want_amp))
    # one frame through the drop-in helper: clipping on the host, the rest a batch of one
    t = len(want) // 2
    one = fp.pitch_detect_frame(fp.center_clip(F[t], False), 10000, 'male')
    assert one.dtype == np.float64 and one.shape == (L10,)
    assert np.max(np.abs(one[1:] - want[t, 1:])) / np.max(np.abs(want[t, 1:])) <= 1e-4


# ---- 1b ----
@pytest.mark.parametrize('L', [128, 256, 1024])
def test_rows_scores_and_tracks_at_the_other_frame_lengths(L, fp):
    """The kernels at the served frame lengths no caller of the reference uses: L = 128, 256 and 1024 give 1, 2 and 8 FIR
    outputs per lane and half and 2, 4 and 16 registers per row.  Two 10 kHz chirps of 0.3 s, a clip of 100 samples
    and a silent clip, hop 100.  Rows of the voiced frames (the restatement's row is finite) against the restatement
    at the project's 1e-4, per frame as in test 1; scores and Hz values exactly against the restatement's tracker on
    the device's own rows."""
    from pitch_cepstrum_cases import chirp
    rng = np.random.default_rng(300 + L)
    clips = [chirp(rng, 10000, 0.3), chirp(rng, 10000, 0.3), chirp(rng, 10000, 0.3)[1400:1500], np.zeros(1500)]
    so = _so(clips)
    flat = np.concatenate(clips)
    rows, amp, fo = fp.cepstrum_rows_batch(flat, so, L, S10)
    pitch, scores, fo2 = fp.pitch_cepstrum_tracks_batch(flat, so, L, S10)
    assert rows.shape == (fo[-1], L) and np.array_equal(fo, fo2)
    voiced = 0
    for b, c in enumerate(clips):
        want = ref.cepstrum_rows(ref.frames_of(c, L, S10))
        got = rows[fo[b]:fo[b + 1]]
        assert got.shape == want.shape, b
        for t in range(len(want)):
            if not np.isfinite(want[t]).all():
                continue
            voiced += 1
            full = np.max(np.abs(got[t] - want[t])) / np.max(np.abs(want[t]))
            tail = np.max(np.abs(got[t, 1:] - want[t, 1:])) / np.max(np.abs(want[t, 1:]))
            print(f'L = {L} clip {b} frame {t}: normwise {full:.3e}, columns 1.. {tail:.3e}')
            record(f'pitch_cepstrum_rows_normwise_L{L}', full)
            record(f'pitch_cepstrum_rows_normwise_cols1_L{L}', tail)
            assert full <= 1e-4 and tail <= 1e-4, (L, b, t, full, tail)
        scores_b = ref.peak_scores(ref.smooth_rows(got))
        assert np.array_equal(scores[fo[b]:fo[b + 1]], scores_b), (L, b)
        assert np.array_equal(pitch[fo[b]:fo[b + 1]], ref.robust_track(scores_b)), (L, b)
    assert voiced >= 2 * (1 + (3000 - L) // S10)                             # every frame of the two chirps
    assert fo[4] - fo[3] > 1 and np.all(pitch[fo[3]:fo[4]] == 500.0)         # the silent clip


# ---- 2 ----
def test_scores_and_tracks_of_the_chirps(tracks, pgold):
    frames = bad = bad_rows = same = 0
    for c in CHIRPS:
        pitch, scores = tracks[c['name']]
        g = _gold(pgold, c['name'])
        n_bad = int(np.sum(pitch != g['pitch']))
        n_rows = int(np.sum(np.any(scores != g['scores'], axis=1)))
        print(f"{c['name']}: {len(pitch)} frames, {n_bad} Hz values differ, {n_rows} score rows differ")
        frames += len(pitch)
        bad += n_bad
        bad_rows += n_rows
        same += n_bad == 0
    record('pitch_cepstrum_track_mismatch_fraction', bad / frames)
    record('pitch_cepstrum_score_row_mismatch_fraction', bad_rows / frames)
    print(f'{frames} chirp frames: {bad} Hz values differ, {bad_rows} score rows differ, {same} of {len(CHIRPS)} tracks identical')
    assert frames >= 800
    assert bad / frames <= 0.01
    assert same >= 10
    # the voiced part of silent_tail, and short, fall under the same cap
    g, (pitch, _) = _gold(pgold, 'silent_tail'), tracks['silent_tail']
    first500 = len(g['pitch'])                                             # start of the trailing run of 500.0
    while first500 > 0 and g['pitch'][first500 - 1] == 500.0:
        first500 -= 1
    extra_frames = first500 + len(tracks['short'][0])
    extra_bad = int(np.sum(pitch[:first500] != g['pitch'][:first500])) + int(np.sum(tracks['short'][0] != pgold['short/pitch']))
    print(f'silent_tail (voiced part) and short: {extra_bad} of {extra_frames} Hz values differ')
    assert (bad + extra_bad) / (frames + extra_frames) <= 0.01


def test_pitch_detect_is_the_reference_signature(fp, tracks, pgold):
    c = CHIRPS[3]
    sig, rate = make_input(c)
    pitch, frames = fp.pitch_detect(sig, rate)
    assert isinstance(pitch, list) and len(pitch) == len(frames) == int(pgold[f"{c['name']}/n_frames"])
    assert np.array_equal(np.array(pitch), tracks[c['name']][0])
    assert np.asarray(frames).shape[1] == L10
    # peak_score: a batch of one through the tracker with both flags clear, on fp64 rows
    rows = ref.smooth_rows(ref.cepstrum_rows(np.asarray(frames, dtype=np.float64)))
    want = ref.peak_scores(rows)
    for t in (0, len(rows) // 2, len(rows) - 1):
        got = fp.peak_score(rows[t])
        assert isinstance(got, list) and len(got) == 80 and got == [int(v) for v in want[t]]
    assert fp.peak_score(rows[1][:300]) == [int(v) for v in ref.peak_scores(rows[1:2, :300])[0]]   # any length >= 100
    assert fp.peak_score(np.full(512, np.nan)) == [0] * 80


# ---- 3 ----
def test_pitch_feature_three_forms(fp, tracks, pgold):
    import torch
    dev = torch.device('cuda', 0)
    checked = 0
    for c in CHIRPS:
        name = c['name']
        g = _gold(pgold, name)
        sig, rate = make_input(c)
        one = fp.pitch_feature(sig, rate)
        assert isinstance(one, tuple) and len(one) == 5 and all(isinstance(v, np.float64) for v in one)
        feat, valid, d = fp.pitch_feature_batch(sig, [0, len(sig)], rate, details=True)
        x = torch.from_numpy(np.asarray(sig, dtype=np.float32)).to(dev)
        so = torch.tensor([0, len(sig)], dtype=torch.int64, device=dev)
        r = fp.pitch_features_device(x.data_ptr(), so.data_ptr(), 1, len(sig), rate, stream=torch.cuda.current_stream(dev))
        torch.cuda.synchronize(dev)
        dfeat = r.feat.download((1, 5), np.float64)
        assert valid[0]
        assert np.array(one).tobytes() == feat[0].tobytes() == dfeat[0].tobytes()          # the three forms agree bitwise
        assert np.array_equal(d['pitch'], tracks[name][0])
        if not np.array_equal(d['pitch'], g['pitch']):
            continue
        checked += 1
        _aux_matches(d['aux'][0], d['seg'], 0, g)
        print(name, 'feat', feat[0], 'reference', g['feat'])
        assert _feat_close(feat[0], g['feat']), (name, feat[0], g['feat'])
    assert checked >= 10


# ---- 4 ----
def _run_tail(nat, pitches, amps):
    """dsp_pitch_feature_batch and dsp_pitch_smooth_subseq_batch through the C ABI on a ragged batch."""
    lib = nat.load()
    fo = np.concatenate([[0], np.cumsum([len(p) for p in pitches])]).astype(np.int64)
    B, n = len(pitches), int(fo[-1])
    d_p = nat.DeviceBuffer(n * 8).upload(np.concatenate(pitches).astype(np.float64))
    d_a = nat.DeviceBuffer(n * 8).upload(np.concatenate(amps).astype(np.float64))
    d_fo = nat.DeviceBuffer(fo.nbytes).upload(fo)
    d_seg, d_feat, d_aux = nat.DeviceBuffer(n * 8), nat.DeviceBuffer(B * 40), nat.DeviceBuffer(B * 36)
    nat.check(lib.dsp_pitch_feature_batch(d_p.ptr, d_a.ptr, d_fo.ptr, B, d_seg.ptr, d_feat.ptr, d_aux.ptr, None))
    res = (d_feat.download((B, 5), np.float64), d_aux.download((B, 9), np.int32), d_seg.download((n,), np.float64), fo)
    d_only = nat.DeviceBuffer(B * 36)
    nat.check(lib.dsp_memset(d_only.ptr, 0xff, B * 36, None))
    nat.check(lib.dsp_pitch_feature_batch(None, d_a.ptr, d_fo.ptr, B, None, None, d_only.ptr, None))
    only = d_only.download((B, 9), np.int32)
    assert np.array_equal(only[:, 0], res[1][:, 0]) and np.all(only[:, 1:] == -1)           # d_pitch == NULL: p alone
    d_seg2, d_info = nat.DeviceBuffer(n * 8), nat.DeviceBuffer(B * 12)
    nat.check(lib.dsp_pitch_smooth_subseq_batch(d_p.ptr, d_fo.ptr, B, 3, 30.0, d_seg2.ptr, d_info.ptr, None))
    return res + (d_info.download((B, 3), np.int32), d_seg2.download((n,), np.float64))


def test_tail_alone_on_the_stored_tracks(fp, pgold):
    from features import _native as nat
    pitches, amps, golds = [], [], []
    for c in CASES:
        sig, rate = make_input(c)
        F = ref.frames_of(ref.decimate(sig, rate), L10, S10)
        pitches.append(pgold[f"{c['name']}/pitch"])
        amps.append(np.abs(F).sum(axis=1))
        golds.append(_gold(pgold, c['name']))
    feat, aux, seg, fo, info, seg2 = _run_tail(nat, pitches, amps)
    for b, (c, g) in enumerate(zip(CASES, golds)):
        if g['raises']:
            assert aux[b, 8] == 0 and np.isnan(feat[b]).all()
            continue
        _aux_matches(aux[b], seg, int(fo[b]), g)
        assert _feat_close(feat[b], g['feat']), (c['name'], feat[b], g['feat'])
        # the helpers: batches of one
        p, p_bias = int(g['p']), 5 if int(g['p']) > 15 else 0
        s1, i1 = fp.find_smooth_subsequence(list(pitches[b][p_bias:p]), bias=p_bias)
        assert isinstance(s1, list) and np.array_equal(s1, g['seg1']) and tuple(i1) == tuple(int(v) for v in g['idx1'])
        s2, i2 = fp.find_smooth_subsequence(pitches[b][p:], bias=p)
        assert np.array_equal(s2, g['seg2']) and tuple(i2) == tuple(int(v) for v in g['idx2'])
        frames = ref.frames_of(ref.decimate(make_input(c)[0], c['rate']), L10, S10)
        assert fp.sub_endpoint_detect(frames) == p
        assert abs(fp.slope(s1) - g['feat'][0]) <= 1e-9 and abs(fp.quad_params(s2) - g['feat'][3]) <= 1e-9
        assert fp.peakshift(s1, s2) == g['feat'][4]
    with pytest.raises(ValueError):
        fp.find_smooth_subsequence([])


def test_tail_alone_on_random_sequences(fp):
    """200 integer-valued pitch sequences (so segment lengths tie often) of 1 .. 140 frames, T <= 20 included, with random
    amplitudes, against the restatement."""
    from features import _native as nat
    rng = np.random.default_rng(2024)
    pitches, amps = [], []
    for k in range(200):
        T = int(rng.integers(1, 21)) if k % 4 == 0 else int(rng.integers(21, 141))
        level = rng.choice([100.0, 125.0, 160.0, 200.0, 250.0, 320.0, 500.0], size=T)
        hold = np.repeat(level[::4], 4)[:T] if k % 3 else level            # long smooth runs, or jumps everywhere
        pitches.append(hold + rng.integers(-12, 13, T))
        a = rng.integers(50, 5000, T).astype(np.float64)
        if k % 5 == 0:
            a[:] = a[0]                                                     # every frame a tie: the first candidate wins
        amps.append(a)
    feat, aux, seg, fo, info, seg2 = _run_tail(nat, pitches, amps)
    n_valid = n_tie = 0
    for b in range(200):
        w = ref.features_of(pitches[b], amps[b])
        assert int(aux[b, 0]) == w['p'], b
        assert int(aux[b, 8]) == int(w['valid']), b
        s, a0, b0 = ref.smooth_subsequence(pitches[b])
        assert tuple(int(v) for v in info[b]) == (a0, b0, len(s)), b
        assert np.array_equal(seg2[fo[b]:fo[b] + len(s)], s), b
        if not w['valid']:
            assert np.isnan(feat[b]).all(), b
            continue
        n_valid += 1
        _aux_matches(aux[b], seg, int(fo[b]), w)
        assert _feat_close(feat[b], w['feat']), (b, feat[b], w['feat'])
    print(f'{n_valid} of 200 random sequences valid')
    assert 50 <= n_valid < 200


# ---- 5 ----
def test_silent_tail_short_and_one_frame(fp, tracks, pgold):
    from features import _native as nat
    sig, rate = make_input(_case('silent_tail'))
    F = ref.frames_of(ref.decimate(sig, rate), L10, S10)
    first_silent = int(np.flatnonzero(~F.any(axis=1))[0])
    pitch, scores = tracks['silent_tail']
    assert np.all(pgold['silent_tail/pitch'][first_silent - 1:] == 500.0)
    assert np.all(pitch[first_silent - 1:] == 500.0)                       # exactly, as stored
    assert np.all(scores[first_silent - 1:] == 0)
    rows, _, _ = fp.cepstrum_rows_batch(ref.decimate(sig, rate), [0, len(ref.decimate(sig, rate))], L10, S10)
    assert np.isposinf(rows[first_silent, 0]) and np.isnan(rows[first_silent, 1:]).all()   # [inf, nan, nan, ...] as NumPy
    for name in ('silent_tail', 'short'):
        g = _gold(pgold, name)
        s, r = make_input(_case(name))
        feat = fp.pitch_feature(s, r)                                      # the reference returns numbers for both
        assert np.isfinite(feat).all()
        if np.array_equal(tracks[name][0], g['pitch']):
            assert _feat_close(feat, g['feat']), (name, feat, g['feat'])
    s, r = make_input(_case('short'))
    _, _, d = fp.pitch_feature_batch(s, [0, len(s)], r, details=True)
    assert tuple(d['aux'][0, :2]) == (8, 0) and tuple(d['aux'][0, 2:6]) == (0, 8, 8, 16)
    s, r = make_input(_case('one_frame'))
    feat, valid = fp.pitch_feature_batch(s, [0, len(s)], r)
    assert not valid[0] and np.isnan(feat[0]).all()
    assert tracks['one_frame'][0].tolist() == [500.0]
    with pytest.raises(ValueError):
        fp.pitch_feature(s, r)
    # a frame length of 500: DSP_EINVAL through the C ABI, ValueError from the Python side
    lib = nat.load()
    x = nat.DeviceBuffer(4 * 4000).upload(np.zeros(4000, dtype=np.float32))
    so = nat.DeviceBuffer(16).upload(np.array([0, 4000], dtype=np.int64))
    fo = nat.DeviceBuffer(16).upload(nat.frame_offsets([0, 4000], 500, 100))
    rows_buf, taps = nat.DeviceBuffer(36 * 500 * 4), nat.DeviceBuffer(500 * 8).upload(np.zeros(1000, dtype=np.float32))
    assert lib.dsp_pitch_cepstrum_batch(x.ptr, so.ptr, fo.ptr, 1, 36, 0, 500, 100, taps.ptr, 1, rows_buf.ptr, None, None) == nat.EINVAL
    assert b'500' in lib.dsp_last_error()
    with pytest.raises(ValueError):
        fp.pitch_detect(make_input(CHIRPS[0])[0], CHIRPS[0]['rate'], winlen=0.05)
    with pytest.raises(ValueError):
        fp.pitch_detect_frame(np.ones(500), 10000, 'male')


# ---- 6 ----
def test_ragged_batch_against_the_restatement(fp):
    clips, rate = random_chirp_batch(77, 64)
    clips.insert(17, clips[0][:300].copy())                               # shorter than one 10 kHz frame
    so = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    flat = np.concatenate(clips)
    feat, valid, d = fp.pitch_feature_batch(flat, so, rate, details=True)
    feat2, valid2, d2 = fp.pitch_feature_batch(flat, so, rate, details=True)
    assert feat.tobytes() == feat2.tobytes() and d['pitch'].tobytes() == d2['pitch'].tobytes()
    assert d['aux'].tobytes() == d2['aux'].tobytes()
    fo = d['frame_off']
    frames = bad = same = checked = 0
    for b, clip in enumerate(clips):
        w = ref.full(clip, rate)
        got = d['pitch'][fo[b]:fo[b + 1]]
        assert len(got) == len(w['pitch']), b
        if b == 17:
            assert len(got) == 1 and got[0] == 500.0 and not valid[b] and np.isnan(feat[b]).all()
            continue
        n_bad = int(np.sum(got != w['pitch']))
        frames += len(got)
        bad += n_bad
        same += n_bad == 0
        assert int(d['aux'][b, 0]) == w['p'], b                           # int16 clips: the amplitude sums are exact
        if n_bad:
            continue
        assert bool(valid[b]) == w['valid'], b
        if w['valid']:
            checked += 1
            _aux_matches(d['aux'][b], d['seg'], int(fo[b]), w)
            assert _feat_close(feat[b], w['feat']), (b, feat[b], w['feat'])
    record('pitch_cepstrum_ragged_track_mismatch_fraction', bad / frames)
    print(f'ragged batch: {frames} frames, {bad} Hz values differ, {same} of 64 tracks identical, {checked} feature rows checked')
    assert bad / frames <= 0.01
    assert same * 12 >= 64 * 10                                           # the share test 2 asks of the chirps: 10 of 12
    assert checked >= 32


# ---- 7 ----
def _guarded(nbytes, dev):
    import torch
    total = (PAD + nbytes + PAD + 3) // 4 * 4
    buf = torch.empty(total // 4, dtype=torch.int32, device=dev)
    buf.fill_(int(SENT32))
    raw = buf.view(torch.uint8)

    def check(what):
        torch.cuda.synchronize(dev)
        host = raw.cpu().numpy()
        sent = np.full(total // 4, SENT32, dtype=np.int32).view(np.uint8)
        assert np.array_equal(host[:PAD], sent[:PAD]), f'{what}: bytes BEFORE the buffer were written'
        assert np.array_equal(host[PAD + nbytes:], sent[PAD + nbytes:]), f'{what}: bytes AFTER the buffer were written'
        return host[PAD:PAD + nbytes]
    return buf, buf.data_ptr() + PAD, check


def test_outputs_stay_inside_their_buffers(fp):
    """Sentinel words around every buffer the three launches write, on a ragged batch with clips of 1, 99, 512, 513 and
    612 samples (one frame; one frame; exactly one; two with the second almost empty; two)."""
    import torch
    from features import _native as nat
    dev = torch.device('cuda', 0)
    lib = nat.load()
    rng = np.random.default_rng(9)
    lens = [1, 99, 512, 513, 612, 5000, 7777, 3001]
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = nat.frame_offsets(so, L10, S10)
    n, B = int(fo[-1]), len(lens)
    x = torch.from_numpy(np.round(3000 * rng.standard_normal(int(so[-1]))).astype(np.float32)).to(dev)
    d_so, d_fo = torch.from_numpy(so).to(dev), torch.from_numpy(fo).to(dev)
    taps = fp._device_taps(L10, 10000, 1000)
    g_rows, p_rows, c_rows = _guarded(n * L10 * 4, dev)
    g_amp, p_amp, c_amp = _guarded(n * 8, dev)
    g_pitch, p_pitch, c_pitch = _guarded(n * 8, dev)
    g_sc, p_sc, c_sc = _guarded(n * 80 * 4, dev)
    g_seg, p_seg, c_seg = _guarded(n * 8, dev)
    g_feat, p_feat, c_feat = _guarded(B * 40, dev)
    g_aux, p_aux, c_aux = _guarded(B * 36, dev)
    nat.check(lib.dsp_pitch_cepstrum_batch(x.data_ptr(), d_so.data_ptr(), d_fo.data_ptr(), B, n, 0, L10, S10, taps.ptr, 1, p_rows, p_amp, None))
    nat.check(lib.dsp_pitch_cepstrum_track_batch(p_rows, 0, d_fo.data_ptr(), B, L10, 3, p_pitch, p_sc, None))
    nat.check(lib.dsp_pitch_feature_batch(p_pitch, p_amp, d_fo.data_ptr(), B, p_seg, p_feat, p_aux, None))
    rows = c_rows('d_rows').view(np.float32)
    assert not np.any(rows.view(np.int32) == SENT32)                       # every element written
    amp = c_amp('d_amp').view(np.float64)
    assert np.isfinite(amp).all() and (amp >= 0).all()
    pitch = c_pitch('d_pitch').view(np.float64)
    assert np.all((pitch >= 50.0) & (pitch <= 500.0))
    sc = c_sc('d_scores').view(np.int32)
    assert np.all((sc >= 0) & (sc < 100))
    c_seg('d_seg')
    c_feat('d_feat')
    aux = c_aux('d_aux').view(np.int32).reshape(B, 9)
    assert np.all((aux[:, 8] == 0) | (aux[:, 8] == 1)) and np.all(aux[:5, 8] == 0)      # one or two frames: nothing to fit
    # the same batch with a launch grid sized by an upper bound of the frame count
    g_rows2, p_rows2, c_rows2 = _guarded(n * L10 * 4, dev)
    nat.check(lib.dsp_pitch_cepstrum_batch(x.data_ptr(), d_so.data_ptr(), d_fo.data_ptr(), B, n + 37, 0, L10, S10, taps.ptr, 1, p_rows2, None, None))
    assert c_rows2('d_rows, bounded grid').tobytes() == rows.tobytes()


# ---- 8 ----
def test_graph_capture_replays_to_the_same_bytes(fp):
    import torch
    dev = torch.device('cuda', 0)
    clips, rate = random_chirp_batch(5, 16, 0.4, 0.6)
    so = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    x = torch.from_numpy(np.concatenate(clips).astype(np.float32)).to(dev)
    d_so = torch.from_numpy(so).to(dev)
    B, n = len(clips), int(so[-1])

    def enqueue(stream):
        return fp.pitch_features_device(x.data_ptr(), d_so.data_ptr(), B, n, rate, stream=stream)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        r = enqueue(side)                                                  # every scratch buffer exists after this
    side.synchronize()
    first = r.feat.download((B, 5), np.float64)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rg = enqueue(torch.cuda.current_stream(dev))
    assert rg.feat.ptr == r.feat.ptr and rg.pitch.ptr == r.pitch.ptr       # nothing was reallocated
    # new data of the same lengths
    clips2, _ = random_chirp_batch(6, 16, 0.4, 0.6)
    flat2 = np.concatenate([np.resize(c2, len(c)) for c, c2 in zip(clips, clips2)]).astype(np.float32)
    x.copy_(torch.from_numpy(flat2).to(dev))
    torch.cuda.synchronize(dev)
    graph.replay()
    torch.cuda.synchronize(dev)
    fo = r.frame_off.download((B + 1,), np.int64)
    replayed = (r.feat.download((B, 5), np.float64).tobytes(), r.aux.download((B, 9), np.int32).tobytes(),
                r.pitch.download((int(fo[-1]),), np.float64).tobytes())
    r2 = enqueue(None)
    torch.cuda.synchronize(dev)
    eager = (r2.feat.download((B, 5), np.float64).tobytes(), r2.aux.download((B, 9), np.int32).tobytes(),
             r2.pitch.download((int(fo[-1]),), np.float64).tobytes())
    assert replayed == eager
    assert replayed[0] != first.tobytes()                                  # the replay did see the new clips
