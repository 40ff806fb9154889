"""Plans and inputs for the NFFT sizes dsp_plan_create_ex(DSP_PLAN_ANY_NFFT) adds: every integer in [16, 4096] that is
neither 2^k nor 3 2^k.  Cases and nothing else; tests/test_anyfft_host.py (no GPU) shows the inputs feasible and the
near-threshold frames where they claim to be, tests/test_gpu_anyfft.py runs them on the device.

  SMOOTH   even sizes whose half is 2^a 3^b 5^c (route 1, mixed radix): two and three factors of 3, up to four of 5, an odd
           half (50, 3750, 4050), both ends of the range (20, 4050)
  CHIRP    everything else (route 2, chirp-z): odd sizes, a prime (17, 331, 401, 1103, 4093), 2 x prime (22, 4094), the first
           size above a power of two (17, 2049), both ends of the range (17, 4095)
  PLANS    each size with the three frame lengths of generic_cases.frame_len; clips and dense batches are generic_cases'
  NEAR     white-noise frames whose smallest filter / energy ratio lies just below ('below': the kernels' rule recomputes
           that filter in fp64) and just above ('above': it is left to the fp32 spectrum) the plan's repair threshold
"""
import numpy as np

import generic_cases as gc

SMOOTH = (20, 50, 160, 400, 576, 1000, 1200, 2000, 3456, 3750, 4000, 4050)
CHIRP = (17, 22, 25, 331, 401, 551, 1103, 1323, 2049, 4093, 4094, 4095)
SIZES = SMOOTH + CHIRP
OLD = gc.NFFTS                                   # route 0: what dsp_plan_create accepts

PLANS = [gc.make_plan(n, k) for n in SIZES for k in gc.LKINDS]
PLAN_BY_NAME = {p['name']: p for p in PLANS}
# generic_cases.natural_block / natural_clip look their plan up by name: the 'eq' plans of these sizes join the table
gc.PLAN_BY_NAME.update({p['name']: p for p in PLANS if p['name'] not in gc.PLAN_BY_NAME})

# the sizes of tests/golden/anyfft_golden.npz: (nfft, rate, winlen, winstep)
GOLDEN = ((400, 16000, 0.025, 0.01), (551, 22050, 0.025, 0.01), (1103, 44100, 0.025, 0.01), (1200, 48000, 0.025, 0.01),
          (1323, 44100, 0.03, 0.01), (25, 16000, 0.0015, 0.0005), (4093, 48000, 0.08, 0.03))


def golden_kw(nfft, rate, winlen, winstep):
    return dict(samplerate=rate, winlen=winlen, winstep=winstep, numcep=13, nfilt=min(26, max(1, nfft // 4)), nfft=nfft,
                lowfreq=0, highfreq=None, preemph=0.97, ceplifter=22, appendEnergy=True)


def golden_clip(nfft, rate, winlen, winstep):
    """A short clip: four to six frames, the last one padded."""
    L, S = gc.sizes(dict(winlen=winlen, winstep=winstep, samplerate=rate))
    rng = np.random.default_rng([77, nfft])
    return (0.25 * rng.standard_normal(L + 2 * S + 17)).astype(np.float32)


def golden_frames(x, nfft, rate, winlen, winstep):
    """The [T, L] fp64 frames the spectrum functions of the golden file were called on: Hamming-windowed frames of the
    clip, no pre-emphasis (plain NumPy: an input of the test, not a result)."""
    L, S = gc.sizes(dict(winlen=winlen, winstep=winstep, samplerate=rate))
    T = gc.cc.n_frames(len(x), L, S)
    pad = np.zeros((T - 1) * S + L)
    pad[:len(x)] = x
    return pad[np.arange(L)[None, :] + S * np.arange(T)[:, None]] * np.hamming(L)


def expected_route(nfft):
    """0: 2^k / 3 2^k; 1: even with a half of 2^a 3^b 5^c; 2: the rest."""
    if nfft in OLD:
        return 0
    if nfft % 2:
        return 2
    h = nfft // 2
    for f in (2, 3, 5):
        while h % f == 0:
            h //= f
    return 1 if h == 1 else 2


def expected_conv_len(nfft, L):
    """The smallest 2^k or 3 2^k that holds min(L, nfft) + nfft // 2 points."""
    need = min(L, nfft) + nfft // 2
    return min(m for m in [1 << k for k in range(14)] + [3 << k for k in range(13)] if m >= need)


# ---- near-threshold frames ------------------------------------------------------------------------------------------------
# Natural: (seed, frame) names frame `frame` of generic_cases.natural_block(nfft, seed, dtype); the clip is the 13 frames
# around it (generic_cases.natural_clip).  'below': smallest positive ratio in [thr / 100, thr); 'above': in [thr, 100 thr),
# thr = generic_cases.repair_threshold(K).  Found with near_search below (generic_cases.natural_search with the window placed
# at the plan's own threshold); only the indices are kept.  White noise through the 26 wide filters of the 1103 and 4093
# plans never comes near 7e-10 of the frame's energy (six blocks of 4096 frames, either dtype: no frame in either window), nor
# below the threshold at 400: those sides are engineered (ENG below).
NEAR_SIZES = (400, 1103, 25, 4093)
NEAR = {
    400: {'above': {'float32': [(0, 1364), (0, 1380), (1, 706)], 'int16': [(0, 736)]}},
    25: {'below': {'float32': [(0, 22), (0, 58), (1, 16)], 'int16': [(0, 20)]},
         'above': {'float32': [(0, 6), (0, 19), (1, 7)], 'int16': [(0, 6)]}},
}


def near_window(nfft, side):
    thr = float(gc.repair_threshold(nfft // 2 + 1))
    return (thr / 100, thr) if side == 'below' else (thr, 100 * thr)


def near_search(nfft, seed, dtype, side):
    """generic_cases.natural_search with the window placed at the plan's own threshold, on either side of it."""
    p = gc.PLAN_BY_NAME[f'{nfft}-eq']
    r = gc.filter_ratios64(gc.natural_block(nfft, seed, dtype), p['kw'], gc.winfunc_of(p))
    r = np.where(r > 0, r, np.inf).min(axis=1)
    lo, hi = near_window(nfft, side)
    t = np.nonzero((r >= lo) & (r < hi))[0]
    return [int(v) for v in t if 6 <= v < gc.NATURAL_BLOCK - 6]


def near_cases():
    out = []
    for nfft, sides in NEAR.items():
        for side, by in sides.items():
            for dt, lst in by.items():
                for seed, frame in lst:
                    out.append(dict(name=f'near{nfft}_{side}_{dt}_{seed}_{frame}', plan=gc.PLAN_BY_NAME[f'{nfft}-eq'], nfft=nfft,
                                    side=side, dtype=dt, seed=seed, frame=frame))
    return out


# Engineered (generic_cases.engineered_clip's recipe): the plan's narrowest filter of frame `frame` of a 13-frame clip at
# |X[k]| = ratio x median_k |X|.  `above`: the ratios that leave the filter above the plan's threshold (fp64), the others
# put it below -- tests/test_anyfft_host.py checks both claims.
ENG_PLANS = {
    'e400': dict(nfft=400, L=400, S=160, M=40, C=13, rate=16000, frame=5, pad=False, ratios=(1e-2, 1e-3, 1e-4, 1e-5, 1e-6), above=(1e-2, 1e-3)),
    'e1103': dict(nfft=1103, L=1103, S=441, M=64, C=13, rate=44100, frame=7, pad=False, ratios=(1e-2, 1e-3, 1e-4, 1e-5, 1e-6), above=(1e-2, 1e-3)),
    'e4093': dict(nfft=4093, L=3840, S=1440, M=64, C=13, rate=16000, frame=12, pad=True, ratios=(1e-2, 1e-3, 1e-4, 1e-5, 1e-6), above=(1e-2, 1e-3)),
}


def eng_plan(key):
    e = ENG_PLANS[key]
    return dict(name=key, nfft=e['nfft'], L=e['L'], S=e['S'], M=e['M'], C=e['C'], winfunc='hamming',
                kw=gc._kw(e['rate'], e['L'], e['S'], e['C'], e['M'], e['nfft']))


def engineered_cases():
    out = []
    for key, e in ENG_PLANS.items():
        for i, ratio in enumerate(e['ratios']):
            for dtype in (('float32', 'int16') if i == 3 else ('float32',)):
                out.append(dict(name=f'{key}_r{ratio:g}_{dtype}', key=key, plan=eng_plan(key), ratio=ratio, dtype=dtype,
                                seed=7100 + 10 * list(ENG_PLANS).index(key) + i, frame=e['frame'], pad=e['pad'],
                                side='above' if ratio in e['above'] else 'below'))
    return out


_eng = {}


def engineered_clip(case):
    if case['name'] not in _eng:
        p = case['plan']
        L, S = p['L'], p['S']
        n = 12 * S + L - (S // 2 if case['pad'] else 0)     # 13 frames; pad: the last one lacks half a hop of samples
        _, bins = gc.narrowest_filter(p['kw'])
        x = gc.cc.base_clip(case['seed'], n, case['dtype'])
        _eng[case['name']] = gc.cc.engineer(x, L, S, p['nfft'], p['kw']['preemph'], gc.winfunc_of(p), (case['frame'],), bins,
                                            case['ratio'], case['dtype'])
    return _eng[case['name']]
