"""Plans and inputs for the generic feature kernel (csrc/kernels_generic.h) at every NFFT dsp_plan_create accepts.

The file describes cases and inputs and nothing else; tests/test_generic_cases_host.py (no GPU) shows that the inputs are
feasible -- a single-precision pipeline with numpy's FFT, its flagged filters taken from fp64, stays at half the 1e-4 bar --
and tests/test_gpu_generic_configs.py runs them on the device against oracle/dsp_oracle.py.  Nothing is stored: every clip
is generated from a seed.

  PLANS            51 plans: the 17 sizes x three frame lengths (L < NFFT, L = NFFT, L > NFFT: the transform truncates)
  clips / dense    seven ragged clips per plan and dtype (one frame, a padded last frame, exact fits), four dense ones
  random_plans     seeded random plans over all sizes, rates, band limits, windows; random_clips: their ragged batches
  fuzz_trials      the configurations and batches of tests/test_gpu_fuzz.py::test_random_configs_fast_vs_generic
  NATURAL          white-noise frames whose smallest filter lies just ABOVE the repair threshold (seed and frame index)
  ENGINEERED       one whole narrow filter cancelled on purpose (cancel_cases.engineer) at other sizes than 512
  emulate_fp32     the single-precision pipeline, with the kernels' repair rule mirrored in repair_threshold
"""
import numpy as np

import cancel_cases as cc

NFFTS = (16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096)   # 2^k and 3 2^k in [16, 4096]
LKINDS = ('lt', 'eq', 'gt')
RATE = 16000
WINFUNCS = {'hamming': np.hamming, 'hanning': np.hanning, 'ones': lambda n: np.ones((n,))}

# ---- the repair rule of csrc/kernels_repair.h, mirrored in this one place -------------------------------------------------
REPAIR_RATIO = 7e-10          # DSP_REPAIR_RATIO: derived at NFFT 512 (257 bins)
REPAIR_BINS = 257             # DSP_REPAIR_BINS: the bin count it was derived at


def repair_threshold(K):
    """dsp_repair_threshold(K): filter output / frame energy below which a filter is recomputed in fp64, for a plan of K
    bins; the same single-precision operations in the same order.  (257 / K)^3 below 257 bins, the constant from there on:
    profiles/generic_repair_sweep.txt has the measurements it follows from."""
    if K >= REPAIR_BINS:
        return np.float32(REPAIR_RATIO)
    s = np.float32(REPAIR_BINS) / np.float32(K)
    return np.float32(REPAIR_RATIO) * (s * s * s)


def frame_len(nfft, kind):
    return {'lt': 25 * nfft // 32, 'eq': nfft, 'gt': nfft + nfft // 4 + 1}[kind]


def _kw(rate, L, S, C, M, nfft, low=0, high=None, preemph=0.97, lifter=22, energy=True):
    return dict(samplerate=rate, winlen=L / rate, winstep=S / rate, numcep=C, nfilt=M, nfft=nfft, lowfreq=low,
                highfreq=high, preemph=preemph, ceplifter=lifter, appendEnergy=energy)


def make_plan(nfft, kind):
    L = frame_len(nfft, kind)
    S = max(1, L // 3)
    M = min(26, max(1, nfft // 4))
    C = min(13, M)
    return dict(name=f'{nfft}-{kind}', nfft=nfft, kind=kind, L=L, S=S, M=M, C=C, winfunc='hamming',
                kw=_kw(RATE, L, S, C, M, nfft))


PLANS = [make_plan(n, k) for n in NFFTS for k in LKINDS]
PLAN_BY_NAME = {p['name']: p for p in PLANS}


def winfunc_of(plan):
    return WINFUNCS[plan['winfunc']]


def noise(rng, n, dtype):
    """0.25 N(0,1) as fp32, 3000 N(0,1) rounded to int16."""
    g = rng.standard_normal(n)
    if np.dtype(dtype) == np.int16:
        return np.clip(np.round(3000.0 * g), -32768, 32767).astype(np.int16)
    return (0.25 * g).astype(np.float32)


def clip_lengths(L, S):
    return [1, L - 1, L, L + 1, L + S, 3 * L + 2 * S + 5, 6 * L]


def clips(plan, dtype):
    """The seven ragged clips of a plan."""
    rng = np.random.default_rng([plan['nfft'], LKINDS.index(plan['kind']), np.dtype(dtype).itemsize])
    return [noise(rng, n, dtype) for n in clip_lengths(plan['L'], plan['S'])]


def dense_clips(plan, dtype):
    """[4, 3 L + 2 S + 5]."""
    rng = np.random.default_rng([plan['nfft'], LKINDS.index(plan['kind']), np.dtype(dtype).itemsize, 4])
    n = 3 * plan['L'] + 2 * plan['S'] + 5
    return noise(rng, 4 * n, dtype).reshape(4, n)


# ---- random plans -----------------------------------------------------------------------------------------------------
def random_plans(seed, n):
    """n plans; every one is valid for the reference (highfreq <= rate / 2 by construction), none is to be skipped."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nfft = int(rng.choice(NFFTS))
        L = int(rng.integers(3, int(1.3 * nfft) + 1))
        S = int(rng.integers(1, L + 1))
        rate = int(rng.choice([8000, 16000, 22050, 44100, 48000]))
        M = int(rng.integers(1, min(64, nfft) + 1))
        C = int(rng.integers(1, min(M, 16) + 1))
        low = float(rng.choice([0, 50, 300]))
        nyq = rate / 2
        high = None
        if rng.random() < 0.5:
            u = float(rng.random())                                  # (low + 0.2 nyq, nyq]
            high = min(nyq, nyq - u * (nyq - (low + 0.2 * nyq)))
        out.append(dict(name=f'r{seed}_{i}', nfft=nfft, L=L, S=S, M=M, C=C,
                        winfunc=str(rng.choice(['hamming', 'hanning', 'ones'])),
                        kw=_kw(rate, L, S, C, M, nfft, low, high, float(rng.choice([0.0, 0.95, 0.97])),
                               int(rng.choice([0, 22])), bool(rng.integers(0, 2)))))
    return out


RANDOM_SEED, N_RANDOM = 2024, 60


def random_clips(plan, index):
    """Ten ragged clips of a random plan: lengths in [1, 6 L + 7 S] plus {L, L + 1, 1}; fp32 for even index, int16 for odd."""
    rng = np.random.default_rng([RANDOM_SEED, index])
    L, S = plan['L'], plan['S']
    lens = [int(v) for v in rng.integers(1, 6 * L + 7 * S + 1, 7)] + [L, L + 1, 1]
    dtype = np.int16 if index % 2 else np.float32
    return [noise(rng, n, dtype) for n in lens]


# ---- the batches of test_gpu_fuzz.py::test_random_configs_fast_vs_generic ----------------------------------------------
def _fuzz_cfg(rng, nfft):
    rate = int(rng.choice([8000, 16000, 22050, 44100, 48000]))
    if nfft == 512:
        L = int(rng.integers(16, 513))
        S = 2 * int(rng.integers(1, 115))          # even hop, 7 S + 512 fits the wave buffer
        M = int(rng.integers(1, 65))
    else:
        L = int(rng.integers(64, 1537))
        S = int(rng.integers(1, 600))
        M = int(rng.integers(1, 65))
    C = int(rng.integers(1, min(M, 16) + 1))
    low = float(rng.choice([0, 0, 50, 300]))
    high = None if rng.random() < 0.5 else float(rng.uniform(low + 1000, rate / 2))
    return dict(samplerate=rate, winlen=(L + 0.25) / rate, winstep=(S + 0.25) / rate, numcep=C, nfilt=M,
                nfft=nfft, lowfreq=low, highfreq=high, preemph=float(rng.choice([0.0, 0.95, 0.97])),
                ceplifter=int(rng.choice([0, 22])), appendEnergy=bool(rng.integers(0, 2))), L, S


def fuzz_trials(nfft, has_fast_path):
    """Yields (trial, cfg, winfunc, L, S, flat, sample_offsets, dense or None) for the 40 seeded trials whose plan
    `has_fast_path(cfg, winfunc)` accepts; the random stream is the one the fuzz test always drew from (a trial without
    a fast path draws no batch)."""
    rng = np.random.default_rng(1000 + nfft)
    for trial in range(40):
        cfg, L, S = _fuzz_cfg(rng, nfft)
        winfunc = np.hamming if trial % 2 else np.hanning
        if not has_fast_path(cfg, winfunc):
            continue
        dtype = np.int16 if trial % 3 == 0 else np.float32
        lens = [int(x) for x in rng.integers(1, 6 * L + 7 * S, 9)] + [L, L + 1, 1]
        so = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        if dtype == np.int16:
            flat = np.clip(np.round(3000 * rng.standard_normal(so[-1])), -32768, 32767).astype(np.int16)
        else:
            flat = (0.25 * rng.standard_normal(so[-1])).astype(np.float32)
        n_dense = (3 * L + 5 * S) // 4 * 4
        dense = flat[:5 * n_dense].reshape(5, n_dense) if len(flat) >= 5 * n_dense else None
        yield trial, cfg, winfunc, L, S, flat, so, dense


# ---- fp64 and fp32 pipelines ------------------------------------------------------------------------------------------
def sizes(kw):
    from oracle import dsp_oracle as o
    return o.round_half_up(kw['winlen'] * kw['samplerate']), o.round_half_up(kw['winstep'] * kw['samplerate'])


def filter_ratios64(x, kw, winfunc):
    """[T, M] filter output / frame energy in fp64, zeros where the filter (or the frame) is exactly zero."""
    from oracle import dsp_oracle as o
    sig = o.preemphasis(np.asarray(x, dtype=np.float64), kw['preemph'])
    frames = o.framesig(sig, kw['winlen'] * kw['samplerate'], kw['winstep'] * kw['samplerate'], winfunc)
    ps = o.powspec(frames, kw['nfft'])
    fb = o.get_filterbanks(kw['nfilt'], kw['nfft'], kw['samplerate'], kw['lowfreq'], kw['highfreq'])
    e = ps.sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = (ps @ fb.T) / e[:, None]
    return np.where(np.isfinite(r), r, 0.0)


def emulate_fp32(x, kw, winfunc, flagged_from_fp64=False):
    """base.mfcc with every array in single precision and numpy's single-precision FFT (more accurate than a GPU's), for
    any (L, S, NFFT).  -> (cepstra [T, C], filter / energy ratios [T, M] of the fp32 pipeline).
    flagged_from_fp64: every filter the kernels' rule flags (0 < output < repair_threshold(K) * energy) takes its value
    from the fp64 spectrum, as dsp_repair_mel_f64 gives it."""
    from oracle import dsp_oracle as o
    f32 = np.float32
    L, S = sizes(kw)
    nfft = kw['nfft']
    x = np.asarray(x, dtype=f32)
    y = np.append(x[0], x[1:] - f32(kw['preemph']) * x[:-1]).astype(f32) if kw['preemph'] != 0 else x
    T = cc.n_frames(len(y), L, S)
    pad = np.zeros((T - 1) * S + L, dtype=f32)
    pad[:len(y)] = y
    idx = np.arange(L)[None, :] + S * np.arange(T)[:, None]
    fr = pad[idx] * np.asarray(winfunc(L)).astype(f32)
    X = np.fft.rfft(fr[:, :min(L, nfft)], nfft)
    assert X.dtype == np.complex64
    pw = (X.real * X.real + X.imag * X.imag) * f32(1.0 / nfft)
    fb = o.get_filterbanks(kw['nfilt'], nfft, kw['samplerate'], kw['lowfreq'], kw['highfreq']).astype(f32)
    energy = pw.sum(axis=1)
    feat = pw @ fb.T
    with np.errstate(invalid='ignore', divide='ignore'):
        ratios = np.where(energy[:, None] > 0, feat / energy[:, None], f32(0))
    if flagged_from_fp64:
        flag = (feat > 0) & (feat < repair_threshold(nfft // 2 + 1) * energy[:, None])
        if flag.any():
            f64, _ = o.fbank(x.astype(np.float64), kw['samplerate'], kw['winlen'], kw['winstep'], kw['nfilt'], nfft,
                             kw['lowfreq'], kw['highfreq'], kw['preemph'], winfunc)
            feat = np.where(flag, f64.astype(f32), feat)
    energy = np.where(energy == 0, f32(np.finfo(float).eps), energy)
    feat = np.where(feat == 0, f32(np.finfo(float).eps), feat)
    C = min(kw['numcep'], kw['nfilt'])
    dct = (o.lifter_vector(C, kw['ceplifter'])[:, None] * o.dct2_ortho_matrix(kw['nfilt'], C)).astype(f32)
    c = np.log(feat) @ dct.T
    if kw['appendEnergy']:
        c[:, 0] = np.log(energy)
    return c, ratios


def normwise(got, ref):
    """max|got - ref| / max|ref|; the absolute value where the reference is zero up to fp64 round-off (the rule of
    tests/test_gpu_golden.py for such references)."""
    got = np.asarray(got, dtype=np.float64)
    den = float(np.max(np.abs(ref)))
    num = float(np.max(np.abs(got - ref)))
    return num / den if den >= 1e-9 else num


# ---- near-threshold frames, natural --------------------------------------------------------------------------------------
# Frames of seeded white noise (the 'eq' plan of the size) whose smallest positive filter / energy ratio, in fp64, lies in
# [REPAIR_RATIO, 100 REPAIR_RATIO): just above the constant derived at 257 bins, so the parent's rule leaves them to the fp32
# spectrum.  (seed, frame) names frame `frame` of a block of NATURAL_BLOCK frames of noise(default_rng([nfft, seed])); the
# clip is the 13 frames around it, the frame itself being frame 6 of the clip.  Found with natural_search below (at most two per block, 13 frames
# apart); only the indices are kept.
NATURAL_BLOCK = 4096
NATURAL = {
    16: {'float32': [(0, 188), (0, 699), (1, 476), (1, 833), (2, 50), (2, 558), (3, 415), (3, 433)], 'int16': [(0, 429), (0, 503)]},
    24: {'float32': [(0, 107), (0, 231), (1, 387), (1, 658), (2, 63), (2, 288), (3, 152), (3, 233)], 'int16': [(0, 32), (0, 179)]},
    64: {'float32': [(0, 7), (0, 43), (1, 6), (1, 25), (2, 24), (2, 211), (3, 67), (3, 117)], 'int16': [(0, 53), (0, 85)]},
    192: {'float32': [(0, 20), (0, 50), (1, 7), (1, 70), (2, 34), (2, 92), (3, 26), (3, 41)], 'int16': [(0, 16), (0, 30)]},
}


def natural_block(nfft, seed, dtype):
    p = PLAN_BY_NAME[f'{nfft}-eq']
    rng = np.random.default_rng([nfft, seed, np.dtype(dtype).itemsize])
    return noise(rng, (NATURAL_BLOCK - 1) * p['S'] + p['L'], dtype)


def natural_search(nfft, seed, dtype):
    """Frames 6 .. NATURAL_BLOCK - 7 of a block whose smallest positive ratio is in the window (fp64)."""
    p = PLAN_BY_NAME[f'{nfft}-eq']
    r = filter_ratios64(natural_block(nfft, seed, dtype), p['kw'], winfunc_of(p))
    r = np.where(r > 0, r, np.inf).min(axis=1)
    t = np.nonzero((r >= REPAIR_RATIO) & (r < 100 * REPAIR_RATIO))[0]
    return [int(v) for v in t if 6 <= v < NATURAL_BLOCK - 6]


_blocks = {}


def natural_clip(nfft, seed, frame, dtype):
    p = PLAN_BY_NAME[f'{nfft}-eq']
    key = (nfft, seed, np.dtype(dtype).name)
    if key not in _blocks:
        _blocks.clear()                     # one block at a time: the cases of a size come in seed order
        _blocks[key] = natural_block(nfft, seed, dtype)
    x = _blocks[key]
    return x[(frame - 6) * p['S']:(frame - 6) * p['S'] + 12 * p['S'] + p['L']].copy()


def natural_cases():
    """[(name, plan, dtype, nfft, seed, frame)]"""
    out = []
    for nfft, by in NATURAL.items():
        for dt, lst in by.items():
            for seed, frame in lst:
                out.append(dict(name=f'nat{nfft}_{dt}_{seed}_{frame}', plan=PLAN_BY_NAME[f'{nfft}-eq'], dtype=dt, nfft=nfft,
                                seed=seed, frame=frame))
    return out


# ---- near-threshold frames, engineered ---------------------------------------------------------------------------------
# One whole narrow filter (the plan's filter with the fewest taps, the first of them) of frame `frame` of a 13-frame clip at
# |X[k]| = ratio x median_k |X|, by cancel_cases.engineer.  `pad`: the clip is cut short so that the engineered frame is the
# zero-padded last one.  `force`: the plan has a specialised kernel; the generic one is reached by dsp_debug_force_generic.
# `breaks`: a single-precision pipeline without the fp64 values misses the 1e-4 bar on the clip (the seeds are such that it does).
ENG_RATIOS = (1e-3, 1e-4, 1e-5, 1e-6)
ENG_PLANS = {
    'e64': dict(nfft=64, L=50, S=16, M=16, C=13, rate=16000, frame=5, pad=False),
    'e256': dict(nfft=256, L=200, S=80, M=26, C=13, rate=16000, frame=12, pad=True),
    'e1024': dict(nfft=1024, L=800, S=320, M=64, C=13, rate=16000, frame=7, pad=False),
    'e2048gt': dict(nfft=2048, L=2561, S=853, M=64, C=13, rate=48000, frame=12, pad=True),
    'e1536': dict(nfft=1536, L=1440, S=480, M=40, C=13, rate=48000, frame=8, pad=False, force=True),
}


def eng_plan(key):
    e = ENG_PLANS[key]
    return dict(name=key, nfft=e['nfft'], L=e['L'], S=e['S'], M=e['M'], C=e['C'], winfunc='hamming',
                kw=_kw(e['rate'], e['L'], e['S'], e['C'], e['M'], e['nfft']))


def narrowest_filter(kw):
    """(filter index, its bins with a non-zero weight): the fewest taps, the first such filter."""
    from oracle import dsp_oracle as o
    fb = o.get_filterbanks(kw['nfilt'], kw['nfft'], kw['samplerate'], kw['lowfreq'], kw['highfreq'])
    cnt = np.count_nonzero(fb, axis=1)
    j = int(np.argmin(np.where(cnt > 0, cnt, 1 << 30)))
    return j, tuple(int(k) for k in np.nonzero(fb[j])[0])


def engineered_cases():
    out = []
    for key, e in ENG_PLANS.items():
        for i, ratio in enumerate(ENG_RATIOS):
            dtype = 'int16' if (ratio == 1e-5 and key in ('e64', 'e1024')) else 'float32'
            out.append(dict(name=f'{key}_r{ratio:g}_{dtype}', key=key, plan=eng_plan(key), ratio=ratio, dtype=dtype,
                            seed=7000 + 10 * list(ENG_PLANS).index(key) + i, frame=e['frame'], pad=e['pad'],
                            force=bool(e.get('force')),
                            # profiles/r5_cancel_sweep.txt, without the repair: at 1e-5 of the median bin a whole filter
                            # costs 7e-5 .. 2e-3 depending on its phase, at 1e-6 never less than 3e-4
                            breaks=ratio <= 1e-6))
    return out


_eng = {}


def engineered_clip(case):
    if case['name'] not in _eng:
        p = case['plan']
        L, S = p['L'], p['S']
        n = 12 * S + L - (S // 2 if case['pad'] else 0)     # 13 frames; pad: the last one lacks half a hop of samples
        _, bins = narrowest_filter(p['kw'])
        x = cc.base_clip(case['seed'], n, case['dtype'])
        _eng[case['name']] = cc.engineer(x, L, S, p['nfft'], p['kw']['preemph'], winfunc_of(p), (case['frame'],), bins,
                                         case['ratio'], case['dtype'])
    return _eng[case['name']]
