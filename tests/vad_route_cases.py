"""Shared by tests/test_vad_routes_host.py (CPU) and tests/test_gpu_vad_routes.py: the launch routes of dsp_vad_features_batch
(csrc/kernels_vad.h: vad_route), the batches that reach every one of them, and a NumPy reference of the operation
(endpoint.py:109-126, 182-198 on frames cut as sigproc.to_frames cuts them, sigproc.py:11-19).  The reference is written out
here and calls nothing from the package under test."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

# family codes of include/dsp_frontend.h (DSP_VAD_ROUTE_*), restated so that a renumbering there fails the host test
PER_FRAME, SCAN, SUM, TILE_ABS, TILE_SQ = 0, 1, 2, 3, 4
FAMILY_NAMES = {PER_FRAME: 'per-frame', SCAN: 'scan', SUM: 'sum', TILE_ABS: 'tile-abs', TILE_SQ: 'tile-sq'}
I16, F32 = 'int16', 'float32'
WAVE_CODE = {F32: 0, I16: 1}                 # DSP_WAVE_F32, DSP_WAVE_I16
COLUMNS = [(I16, 0), (I16, 1), (F32, 0), (F32, 1)]      # the order of a row below: int16 |x|, int16 x^2, fp32 |x|, fp32 x^2

_PF = ((PER_FRAME, 1),) * 4


def _row(scan_fr, family, fr):
    """scan<scan_fr> / <family-or-its-x^2-form><fr> x 3; family 'tile': tile-sq / tile-abs / tile-sq."""
    if family == 'sum':
        return ((SCAN, scan_fr), (SUM, fr), (SUM, fr), (SUM, fr))
    return ((SCAN, scan_fr), (TILE_SQ, fr), (TILE_ABS, fr), (TILE_SQ, fr))


# (L, S) -> the expected (family, frames per wave) of the four columns, and why the cell is there
CELLS = {
    (48, 16): _PF,                          # L < 64
    (64, 16): _row(16, 'sum', 16),          # smallest tiled shape
    (67, 5): _row(16, 'tile', 16),          # nothing vector-aligned
    (65, 99): _row(16, 'tile', 16),         # hop longer than the frame
    (68, 200): _row(16, 'sum', 16),         # 16 frames fill the staging exactly (15 S + L = 3068), S > L
    (72, 200): _row(8, 'sum', 4),           # one vector past that limit
    (69, 200): _row(8, 'tile', 4),          # same, unaligned
    (480, 480): _row(8, 'sum', 4),          # the hop == length form get_amplitude uses
    (661, 661): _row(4, 'tile', 4),         # eight frames do not fit 20 rounds
    (900, 700): _row(4, 'sum', 4),          # same, aligned
    (1323, 441): _row(8, 'tile', 4),        # 44.1 kHz framing
    (1529, 513): _row(8, 'tile', 4),        # both limits at once: 7 S + L = 5120, 3 S + L = 3068
    (1530, 513): _PF,                       # one sample past them
    (3065, 1): _row(8, 'tile', 4),          # hop of one sample, longest tiled frame
    (3066, 1): _PF,                         # one past
}

# every (family, frames per wave, sample type) the library instantiates
INSTANTIATED = ({(SCAN, fr, I16) for fr in (16, 8, 4)} | {(PER_FRAME, 1, t) for t in (I16, F32)} |
                {(SUM, fr, t) for fr in (16, 4) for t in (I16, F32)} | {(TILE_ABS, fr, F32) for fr in (16, 4)} |
                {(TILE_SQ, fr, t) for fr in (16, 4) for t in (I16, F32)})

# the routes whose waves are sent round their group loop at least twice (tests/test_gpu_vad_routes.py): (family, fr, type, use_sq)
MULTI_ROUND = [(SCAN, 16, I16, 0), (SCAN, 8, I16, 0), (SUM, 16, F32, 0), (SUM, 4, I16, 1), (TILE_ABS, 16, F32, 0),
               (TILE_SQ, 16, I16, 1), (TILE_SQ, 4, F32, 1)]
# the largest number of workgroups of a VAD kernel the launcher keeps resident per CU (per_cu in vad_tile_launch_k), and the
# waves of a workgroup (VAD_WAVES)
MAX_WORKGROUPS_PER_CU, WAVES_PER_WORKGROUP = 8, 4


def expected(L, S, dtype, use_sq):
    return CELLS[(L, S)][COLUMNS.index((dtype, int(use_sq)))]


def case_id(L, S, dtype, use_sq):
    fam, fr = expected(L, S, dtype, use_sq)
    return f'{L}x{S}-{dtype}-{"sq" if use_sq else "abs"}-{FAMILY_NAMES[fam]}{fr}'


def smallest_cell(family, fr, dtype, use_sq):
    """The first cell of the table that takes this route (the table goes from short frames to long ones)."""
    for (L, S) in CELLS:
        if expected(L, S, dtype, use_sq) == (family, fr):
            return L, S
    raise KeyError((family, fr, dtype, use_sq))


# ---- samples ----------------------------------------------------------------------------------------------------------------

def samples(dtype, n, rng, kind=0):
    """int16 -- kind 0: full range, 1: values in [-3, 3] with many zeros, 2: all -32768, 3: +32767 / -32768 alternating.
    fp32 -- normal draws times 10 ** uniform(-3, 4) per sample, a tenth exact 0.0, a twentieth -0.0 (a set sign bit that is no
    crossing); no denormals."""
    if dtype == I16:
        kind %= 4
        if kind == 0:
            return rng.integers(-32768, 32768, n).astype(np.int16)
        if kind == 1:
            return (rng.integers(-3, 4, n) * (rng.random(n) < 0.5)).astype(np.int16)
        if kind == 2:
            return np.full(n, -32768, dtype=np.int16)
        return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 4, n)).astype(np.float32)
    u = rng.random(n)
    x[u < 0.10] = 0.0
    x[(u >= 0.10) & (u < 0.15)] = -0.0
    assert not np.any((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny))
    return x


# ---- batches ----------------------------------------------------------------------------------------------------------------

def clip_lengths(L, S, fr):
    """The ragged clips of a cell whose route takes `fr` frames per wave: the edges of the framing rule, one exactly full group,
    one frame more, two random lengths up to three groups, empty clips first and last."""
    rng = np.random.default_rng(100000 * L + 100 * S + fr)
    lens = [0, 1, 3, L - 1, L, L + 1, L + S, L + S + 1, 5 * S + 7, (fr - 1) * S + L, (fr - 1) * S + L + 2]
    lens += [int(rng.integers(1, 3 * fr * S + L + 1)) for _ in range(2)]
    lens.append(0)
    if S == 1:
        lens = [min(n, L + 40) for n in lens]          # a hop of one sample: a frame per sample, keep the case small
    return lens


def ragged_batch(L, S, dtype, use_sq):
    """-> (flat, sample_offsets int64)."""
    fr = expected(L, S, dtype, use_sq)[1]
    lens = clip_lengths(L, S, fr)
    rng = np.random.default_rng(7 * L + S + (13 if dtype == I16 else 0) + use_sq)
    clips = [samples(dtype, n, rng, k) for k, n in enumerate(lens)]
    return np.concatenate(clips), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def dense_batch(L, S, dtype, use_sq, rem):
    """Five clips of N samples each, N % 4 == rem, a little over one group of frames."""
    fr = expected(L, S, dtype, use_sq)[1]
    n0 = (fr + 1) * S + L + 2
    N = n0 - n0 % 4 + rem
    rng = np.random.default_rng(11 * L + S + rem + (17 if dtype == I16 else 0) + use_sq)
    return np.stack([samples(dtype, N, rng, k) for k in range(5)])


def dense_offsets(x):
    B, N = x.shape
    return np.arange(B + 1, dtype=np.int64) * N


def multi_round_batch(L, S, dtype, fr, min_groups, ragged, seed=0):
    """A batch of at least `min_groups` groups of `fr` frames.  Dense: -> [B, N] with N % 4 == 0 and 5 fr + 3 frames a clip (six
    groups, the last one partly filled).  Ragged: -> (flat, sample_offsets), many short clips of fr + 1 .. 3 fr - 1 frames, none
    a multiple of fr, the last frame of each cut short by a random amount."""
    rng = np.random.default_rng(31 * L + S + fr + seed)
    if not ragged:
        T = 5 * fr + 3
        N = (T - 1) * S + L
        N -= N % 4                                       # less than a hop shorter (S >= 4 here): still T frames
        assert S >= 4 and frame_counts(np.array([N]), L, S)[0] == T
        B = -(-min_groups // 6)
        return samples(dtype, B * N, rng).reshape(B, N)
    Ts, groups = [], 0
    while groups < min_groups:
        T = int(rng.integers(fr + 1, 3 * fr))
        if T % fr == 0:
            continue
        Ts.append(T)
        groups += -(-T // fr)
    Ts = np.array(Ts, dtype=np.int64)
    lens = (Ts - 1) * S + L - rng.integers(0, min(S, L), len(Ts))
    assert np.array_equal(frame_counts(lens, L, S), Ts)
    return samples(dtype, int(lens.sum()), rng), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ---- the reference ----------------------------------------------------------------------------------------------------------

def frame_counts(lens, L, S):
    """T = 1 if n <= L else 1 + ceil((n - L) / S)  (sigproc.py:79-82)."""
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens <= L, 1, 1 + -(-(lens - L) // S)).astype(np.int64)


def frames_of(flat, so, L, S):
    """Every frame of every clip, zero padding of the last one (sigproc.py:84-87) -> ([F, L] int64 or float64, frame offsets).
    The rows are views into one padded copy of the batch (sliding_window_view), gathered by their first sample."""
    so = np.asarray(so, dtype=np.int64)
    lens = np.diff(so)
    T = frame_counts(lens, L, S)
    fo = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    padlen = (T - 1) * S + L
    po = np.concatenate([[0], np.cumsum(padlen)]).astype(np.int64)
    wide = np.int64 if flat.dtype == np.int16 else np.float64
    padded = np.zeros(int(po[-1]), dtype=wide)
    clip = np.repeat(np.arange(len(lens)), lens)                       # clip of every sample
    padded[np.arange(int(so[-1])) - so[clip] + po[clip]] = flat[:int(so[-1])]
    fclip = np.repeat(np.arange(len(T)), T)                             # clip of every frame
    starts = po[fclip] + (np.arange(int(fo[-1])) - fo[fclip]) * S
    return sliding_window_view(padded, L)[starts], fo


def reference(flat, so, L, S, use_sq):
    """-> (amp, zcr int64, frame offsets).  int16: amp = sum |x| or sum x^2 in int64 (below 2^53: the fp64 result must be
    EQUAL).  fp32: the samples in fp64 (squares of fp32 are exact there), every frame summed in np.longdouble.  zcr: the count
    of x[i] * x[i + 1] < 0, the product formed in int64 / fp64 (no fp32 product of the samples drawn here underflows there)."""
    fr, fo = frames_of(flat, so, L, S)
    zcr = np.empty(len(fr), dtype=np.int64)
    amp = np.empty(len(fr), dtype=np.int64 if flat.dtype == np.int16 else np.longdouble)
    step = max(1, (1 << 22) // L)                                       # rows per pass: bounds the temporaries
    for lo in range(0, len(fr), step):
        f = fr[lo:lo + step]
        zcr[lo:lo + step] = (f[:, :-1] * f[:, 1:] < 0).sum(1)
        v = f * f if use_sq else np.abs(f)
        amp[lo:lo + step] = v.sum(1) if flat.dtype == np.int16 else v.astype(np.longdouble).sum(1)
    return amp, zcr, fo


def compare(got_amp, got_zcr, amp, zcr, L, what=''):
    """The rules of the route tests.  zcr always exact; int16 amp exact; fp32 amp within L 2^-52 of the reference, relatively:
    any-order fp64 summation of L non-negative terms errs by at most (L - 1) 2^-53 of the sum to first order, the bar is twice
    that (an fp32 accumulator misses it by nine orders of magnitude).  Returns the worst relative error (0.0 for int16)."""
    got_amp, got_zcr = np.asarray(got_amp), np.asarray(got_zcr)
    assert got_amp.dtype == np.float64 and got_amp.shape == amp.shape and got_zcr.shape == zcr.shape, what
    bad = np.flatnonzero(got_zcr != zcr)
    assert bad.size == 0, (what, 'zcr', bad[:5], got_zcr[bad[:5]], zcr[bad[:5]])
    if amp.dtype == np.int64:
        assert amp.max(initial=0) < 2 ** 53
        bad = np.flatnonzero(got_amp != amp.astype(np.float64))
        assert bad.size == 0, (what, 'amp', bad[:5], got_amp[bad[:5]], amp[bad[:5]])
        return 0.0
    err = np.abs(got_amp.astype(np.longdouble) - amp)
    bad = np.flatnonzero(~(err <= L * np.longdouble(2.0) ** -52 * amp))                    # (a NaN fails too)
    assert bad.size == 0, (what, 'amp', bad[:5], got_amp[bad[:5]], amp[bad[:5]])
    nz = amp > 0
    return float(np.max(err[nz] / amp[nz])) if nz.any() else 0.0
