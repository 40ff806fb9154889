"""Clips with frames whose narrow mel filters are cancelled on purpose.

Filter 0 of the 40-filter bank (NFFT 512, 16 kHz) is FFT bin 1 alone, filter 1 is bins {2, 3}; the 64-filter bank has
eight such filters.  When pre-emphasis and window nearly cancel such a bin in a frame, the filter's output falls many
orders of magnitude below the frame's energy, and an fp32 spectrum -- whose error is a few 1e-7 of the frame's RMS in
every bin -- loses c1..c12 of that frame.  In random data this happens about once in 1e5 frames; here it is built.

X_t[k], the bin after pre-emphasis, window and DFT, is a linear functional of the samples.  `engineer` takes the
minimum-norm change (numpy.linalg.lstsq) of the samples of the asked frames that puts X_t[k] at ratio x median_k |X_t|
for the asked bins, jointly for all of them; the contribution of the sample in front of a frame (through the
pre-emphasis) is part of the functional and stays what it is.  Rounding to the input type comes last:
  fp32   ten "knob" samples per frame are set to zero first; after rounding, the residue is taken up by those knobs alone,
         whose values stay so small (1e-7) that their own rounding is far below any ratio asked for (down to 1e-8);
  int16  greedy +-1 moves (single samples, then pairs) until every bin is at or below the asked ratio.

Inputs are seeded and generated, never stored; tests/golden/make_cancel_golden.py stores the engineered clips of CASES
and the reference's mfcc of them.
"""
import numpy as np

PLAN40 = dict(samplerate=16000, winlen=0.025, winstep=0.01, numcep=13, nfilt=40, nfft=512, lowfreq=0, highfreq=None,
              preemph=0.97, ceplifter=22, appendEnergy=True)
PLAN26 = dict(PLAN40, nfilt=26)
PLAN64 = dict(PLAN40, nfilt=64)          # more filters than the NFFT = 512 kernel takes (48): the generic kernel on every route
PLAN44 = dict(PLAN40, nfilt=44)          # the NFFT = 512 kernel's catch-all instantiation (six filter iterations)
L, S, NFFT = 400, 160, 512
N13, N13PAD = 2320, 2400          # 13 frames exactly; 14 frames, the last one zero padded
RATIOS = (1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 1e-6, 1e-8)


def n_frames(n, L=L, S=S):
    return 1 if n <= L else 1 + -(-(n - L) // S)


def bin_functional(n, L, S, nfft, preemph, win, t, k):
    """c [n] complex (longdouble) with X_t[k] = sum_p c[p] x[p] for a clip of n samples."""
    ld = np.longdouble
    lfft = min(L, nfft)
    m = np.arange(lfft)
    e = np.exp(-2j * np.pi * ld(k) * m.astype(ld) / ld(nfft)) * np.asarray(win, dtype=ld)[:lfft]
    c = np.zeros(n, dtype=np.clongdouble)
    p = t * S + m
    ok = p < n
    c[p[ok]] += e[ok]                                # y[p] = x[p] - a x[p - 1], y[0] = x[0]
    q = p - 1
    ok = (p < n) & (q >= 0)
    c[q[ok]] -= ld(preemph) * e[ok]
    return c


def spectrum(x, L, S, nfft, preemph, win, t):
    """|X_t[k]|, k <= nfft / 2, in fp64 (for the median only)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.append(x[0], x[1:] - preemph * x[:-1])
    fr = np.zeros(L)
    seg = y[t * S: t * S + L]
    fr[:len(seg)] = seg
    return np.abs(np.fft.rfft((fr * win)[:min(L, nfft)], nfft))


def achieved(x, L, S, nfft, preemph, win, frames, bins):
    """ratio |X_t[k]| / median_k |X_t| of every (frame, bin), the bin as a longdouble DFT sum."""
    xl = np.asarray(x, dtype=np.longdouble)
    out = np.zeros((len(frames), len(bins)))
    for i, t in enumerate(frames):
        med = np.median(spectrum(x, L, S, nfft, preemph, win, t))
        for j, k in enumerate(bins):
            out[i, j] = float(abs(np.sum(bin_functional(len(xl), L, S, nfft, preemph, win, t, k) * xl))) / med
    return out


def _knobs(n, L, S, t):
    p = t * S + 20 + 36 * np.arange(10)
    return p[p < min(n, t * S + L)]


def engineer(x, L, S, nfft, preemph, winfunc, frames, bins, ratio, dtype):
    """The clip x (any real array) with X_t[k] at ratio x median_k |X_t| for every t in frames, k in bins; dtype float32 or int16."""
    dtype = np.dtype(dtype)
    win = np.asarray(winfunc(L), dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).copy()
    n = len(x)
    frames, bins = list(frames), list(bins)
    knobs = np.unique(np.concatenate([_knobs(n, L, S, t) for t in frames]))
    if dtype == np.float32:
        x[knobs] = 0.0
    var = np.unique(np.concatenate([np.arange(t * S, min(n, t * S + L)) for t in frames]))
    C = np.array([bin_functional(n, L, S, nfft, preemph, win, t, k) for t in frames for k in bins])   # [rows, n]

    def target():
        tg = []
        for t in frames:
            med = np.median(spectrum(x, L, S, nfft, preemph, win, t))
            for k in bins:
                cur = complex(np.sum(bin_functional(n, L, S, nfft, preemph, win, t, k) * x))
                ph = cur / abs(cur) if abs(cur) > 0 else 1.0
                tg.append(ratio * med * ph)
        return np.array(tg, dtype=np.clongdouble)

    def solve(cols, goal):
        res = goal - C @ x.astype(np.longdouble)
        A = np.concatenate([C[:, cols].real, C[:, cols].imag]).astype(np.float64)
        b = np.concatenate([res.real, res.imag]).astype(np.float64)
        d = np.linalg.lstsq(A, b, rcond=None)[0]
        x[cols] += d

    goal = target()
    solve(var, goal)
    for it in range(8):           # the median moves with the change (a wide filter is a tenth of the bins): again against the
        new = target()            # new one, until it stands still
        if it > 0 and np.max(np.abs(np.abs(new) - np.abs(goal)) / np.abs(goal)) < 1e-3:
            break
        goal = new
        solve(var, goal)
    if dtype == np.float32:
        x = x.astype(np.float32).astype(np.float64)
        for _ in range(3):
            if len(C) > len(knobs):     # a wide filter: fewer knobs than bins cannot take the residue, and at the ratios
                break                   # asked of such a filter (1e-5) plain rounding is already within half a percent
            solve(knobs, goal)
            x = x.astype(np.float32).astype(np.float64)
        return x.astype(np.float32)
    # int16: round, then greedy +-1 moves on the frames' samples until every |residue| is at or below its goal
    x = np.round(x)
    Cv = C[:, var].astype(np.complex128)                       # [rows, nv]
    moves = np.concatenate([Cv, -Cv], axis=1)                  # +1 on sample v, -1 on sample v
    lim = np.abs(goal).astype(np.float64)
    for _ in range(200):
        res = (C @ x.astype(np.longdouble)).astype(np.complex128)
        if np.all(np.abs(res) <= lim):
            break
        cost = lambda r: np.sum(np.maximum(np.abs(r) - 0.7 * lim[:, None], 0.0) ** 2, axis=0)   # noqa: E731
        c1 = cost(res[:, None] + moves)
        best1 = int(np.argmin(c1))
        # pairs of moves: the best partner of each of the 32 best single moves
        cand = np.argsort(c1)[:32]
        best = (c1[best1], (best1,))
        for a in cand:
            c2 = cost(res[:, None] + moves[:, [a]] + moves)
            b = int(np.argmin(c2))
            if c2[b] < best[0]:
                best = (c2[b], (int(a), b))
        if best[0] >= cost(res[:, None])[0]:
            break
        for mv in best[1]:
            x[var[mv % len(var)]] += 1.0 if mv < len(var) else -1.0
    assert np.max(np.abs(x)) < 32767
    return x.astype(np.int16)


def base_clip(seed, n, dtype):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n)
    return 0.25 * g if np.dtype(dtype) == np.float32 else 3000.0 * g


def _case(name, seed, n, dtype, frames, bins, ratio, plan='40', winfunc='hamming', preemph=0.97, whole=None):
    """whole: a whole narrow filter of the plan is cancelled (the case must break an fp32 pipeline when ratio <= 1e-5)."""
    if whole is None:
        whole = {'40': set(bins) >= {1} or set(bins) >= {2, 3},
                 '64': any(set(bins) >= s for s in ({0}, {1}, {2}, {3}, {4}, {5}, {6, 7}, {7, 8})), '26': False, '44': False}[plan]
    return dict(name=name, seed=seed, n=n, dtype=dtype, frames=tuple(frames), bins=tuple(bins), ratio=ratio, plan=plan,
                winfunc=winfunc, preemph=preemph, whole=whole)


def plan_kwargs(case):
    kw = dict({'40': PLAN40, '26': PLAN26, '64': PLAN64, '44': PLAN44}[case['plan']], preemph=case['preemph'])
    return kw, {'hamming': np.hamming, 'hanning': np.hanning}[case['winfunc']]


LAST, LASTPAD = 12, 13            # last frame of a 2 320-sample clip (full) and of a 2 400-sample one (zero padded)
CASES = []
# the ratio sweep: one utterance per ratio, bin 1 (all of filter 0) in frame 5
CASES += [_case(f'sweep_b1_r{r:g}', 300 + i, N13, 'float32', (5,), (1,), r) for i, r in enumerate(RATIOS)]
CASES += [_case(f'sweep_b23_r{r:g}', 320 + i, N13, 'float32', (6,), (2, 3), r) for i, r in enumerate(RATIOS)]
# bins: filters 0 and 1 together; controls ({2} alone leaves filter 1 its other tap; the 26-filter bank has no narrow filter)
CASES += [
    _case('b123_r1e-5', 340, N13, 'float32', (4,), (1, 2, 3), 1e-5),
    _case('b123_r1e-6', 341, N13, 'float32', (9,), (1, 2, 3), 1e-6),
    _case('ctl_b2_r1e-6', 342, N13, 'float32', (4,), (2,), 1e-6),
    _case('ctl_p26_b123_r1e-6', 343, N13, 'float32', (4,), (1, 2, 3), 1e-6, plan='26'),
    _case('p64_b0_r1e-6', 344, N13, 'float32', (3,), (0,), 1e-6, plan='64'),
    _case('p64_b3_r1e-6', 345, N13, 'float32', (3,), (3,), 1e-6, plan='64'),
    _case('p64_b5_r1e-5', 346, N13, 'float32', (8,), (5,), 1e-5, plan='64'),
    _case('p64_b67_r1e-6', 347, N13, 'float32', (8,), (6, 7), 1e-6, plan='64'),
    _case('p64_b0to5_r1e-5', 348, N13, 'float32', (6,), (0, 1, 2, 3, 4, 5), 1e-5, plan='64'),
]
# Whole WIDE filters, and the 44-filter plan: where a filter sits in the NFFT = 512 kernel (lane and iteration) follows a
# dealing rule with mirrored slots and, for an odd number of iterations, a middle iteration; the repair must name the
# filter of a flagged slot.  40 filters: filter 16 and its mirror image 23 lie in the middle iteration; 44 filters run the catch-all
# instantiation, their last filter in a mirrored slot.  (whole = False where the filter is so wide that a single-precision
# pipeline averages its error away: those cases are about WHICH filter is recomputed.)
CASES += [
    _case('p40_f16_r1e-5', 350, N13, 'float32', (5,), range(38, 45), 1e-5, whole=True),
    _case('p40_f23_r1e-5', 351, N13, 'float32', (6,), range(70, 81), 1e-5, whole=False),
    _case('p44_b1_r1e-6', 353, N13, 'float32', (5,), (1,), 1e-6, plan='44', whole=True),
    _case('p44_f22_r1e-5', 354, N13, 'float32', (7,), range(55, 63), 1e-5, plan='44', whole=True),
    _case('p44_f43_r1e-5', 355, N13, 'float32', (8,), range(227, 256), 1e-5, plan='44', whole=False),
]
# frame positions
CASES += [
    _case('frame0_b1', 360, N13, 'float32', (0,), (1,), 1e-6),
    _case('frames7_8_b1', 361, N13, 'float32', (7, 8), (1,), 1e-5),            # across the kernel's 8-frame groups, adjacent
    _case('frames2_3_b23', 362, N13, 'float32', (2, 3), (2, 3), 1e-6),
    _case('group0_all8_b1', 363, N13, 'float32', range(8), (1,), 1e-5),
    _case('last_full_b1', 364, N13, 'float32', (LAST,), (1,), 1e-6),
    _case('last_padded_b1', 365, N13PAD, 'float32', (LASTPAD,), (1,), 1e-6),
    _case('last_padded_b123', 366, N13PAD, 'float32', (LASTPAD,), (1, 2, 3), 1e-6),
    _case('one_frame_b1', 367, 333, 'float32', (0,), (1,), 1e-6),
    _case('one_frame_b23', 368, 250, 'float32', (0,), (2, 3), 1e-5),
]
# window and pre-emphasis
CASES += [
    _case('hann_b1', 380, N13, 'float32', (5,), (1,), 1e-6, winfunc='hanning'),
    _case('hann_b23', 381, N13, 'float32', (10,), (2, 3), 1e-5, winfunc='hanning'),
    _case('nopre_b1', 382, N13, 'float32', (5,), (1,), 1e-6, preemph=0.0),
]
# int16
CASES += [
    _case('i16_b1_r1e-5', 411, N13, 'int16', (5,), (1,), 1e-5),
    _case('i16_b1_r1e-6', 401, N13, 'int16', (7,), (1,), 1e-6),
    _case('i16_b23_r1e-5', 402, N13, 'int16', (8,), (2, 3), 1e-5),
    _case('i16_frame0_b1', 403, N13, 'int16', (0,), (1,), 1e-5),
    _case('i16_last_padded_b1', 404, N13PAD, 'int16', (LASTPAD,), (1,), 1e-5),
    _case('i16_frames7_8_b1', 405, N13, 'int16', (7, 8), (1,), 1e-5),
    _case('i16_p64_b0', 406, N13, 'int16', (3,), (0,), 1e-5, plan='64'),
    _case('i16_ctl_b2', 407, N13, 'int16', (4,), (2,), 1e-5),
]
BY_NAME = {c['name']: c for c in CASES}
_made = {}


def make_input(case):
    """The engineered clip of a case (cached: engineering an int16 clip takes a moment)."""
    name = case['name']
    if name not in _made:
        kw, wf = plan_kwargs(case)
        x = base_clip(case['seed'], case['n'], case['dtype'])
        _made[name] = engineer(x, L, S, NFFT, kw['preemph'], wf, case['frames'], case['bins'], case['ratio'], case['dtype'])
    return _made[name]


# ---- the VAD -> trim -> MFCC pipeline: a burst in noise whose TRIMMED clip has cancelled frames --------------------------
VAD_FRAMES, VAD_BINS, VAD_RATIO = (0, 20), (1,), 1e-6     # frame 0 of the segment: its first sample is not pre-emphasised
VAD_SEEDS = range(10)


def burst_clip(seed):
    """fp32 clip of 1 - 2 s: noise of sigma 30 with a Hann-shaped tone burst of amplitude 8000 (the clips of
    tests/test_gpu_fullsize.py::test_config4_share_ragged, not rounded to integers)."""
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.uniform(1.0, 2.0) * 16000)
    x = rng.normal(0, 30, n)
    blen = int(rng.uniform(0.5, 0.9) * n)
    b0 = int(rng.integers(0, n - blen))
    t = np.arange(blen) / 16000.0
    x[b0:b0 + blen] += 8000 * np.sin(2 * np.pi * rng.uniform(100, 300) * t) * np.hanning(blen)
    return x.astype(np.float32)


def make_vad_case():
    """-> (seed, clip, left, right): the first seed whose clip, engineered RELATIVE TO the oracle's left endpoint (frames
    VAD_FRAMES of clip[left:right]), keeps both endpoints.  None if no seed of VAD_SEEDS does."""
    if 'vad' not in _made:
        from oracle import dsp_oracle
        _made['vad'] = None
        for seed in VAD_SEEDS:
            x = burst_clip(seed)
            l, r = dsp_oracle.basic_endpoint_detection(x, 16000)
            r = min(r, len(x))
            if r - l < (max(VAD_FRAMES) + 3) * S + L:
                continue
            y = x.copy()
            y[l:r] = engineer(x[l:r], L, S, NFFT, 0.97, np.hamming, VAD_FRAMES, VAD_BINS, VAD_RATIO, 'float32')
            l2, r2 = dsp_oracle.basic_endpoint_detection(y, 16000)
            if (l2, min(r2, len(y))) == (l, r):          # the endpoints did not move
                _made['vad'] = (seed, y, l, r)
                break
    return _made['vad']


def emulate_fp32(x, kw, winfunc):
    """base.mfcc with every array in single precision and numpy's single-precision FFT (more accurate than a GPU's)."""
    from oracle import dsp_oracle as o
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    y = np.append(x[0], x[1:] - f32(kw['preemph']) * x[:-1]).astype(f32)
    T = n_frames(len(y))
    pad = np.zeros((T - 1) * S + L, dtype=f32)
    pad[:len(y)] = y
    idx = np.arange(L)[None, :] + S * np.arange(T)[:, None]
    fr = pad[idx] * np.asarray(winfunc(L)).astype(f32)
    X = np.fft.rfft(fr, NFFT)
    assert X.dtype == np.complex64
    pw = (X.real * X.real + X.imag * X.imag) * f32(1.0 / NFFT)
    fb = o.get_filterbanks(kw['nfilt'], NFFT, kw['samplerate'], kw['lowfreq'], kw['highfreq']).astype(f32)
    energy = pw.sum(axis=1)
    energy = np.where(energy == 0, f32(np.finfo(float).eps), energy)
    feat = pw @ fb.T
    feat = np.where(feat == 0, f32(np.finfo(float).eps), feat)
    dct = (o.lifter_vector(kw['numcep'], kw['ceplifter'])[:, None] * o.dct2_ortho_matrix(kw['nfilt'], kw['numcep'])).astype(f32)
    c = np.log(feat) @ dct.T
    c[:, 0] = np.log(energy)
    return c


def normwise(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / np.max(np.abs(ref)))
