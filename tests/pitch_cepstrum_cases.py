"""Cases of the cepstral pitch path (pitch.pitch_detect / pitch.pitch_feature).  Inputs are seeded and generated, never
stored; tests/golden/make_pitch_golden.py runs the reference on them and stores only the numbers.

Twelve voiced chirps (six harmonics with amplitudes 1 / h and random phases under a Hann envelope, f0 rising by 20 %
per second, plus a little noise), rates cycling through 16 / 44.1 / 48 kHz, half of them int16 and half float64 after
preemphasis(., 0.97) -- what pitch_model.py passes -- and three edge cases: a chirp with a silent tail, a clip too short
for the sub-endpoint search, and a one-frame clip the reference raises on.
"""
import numpy as np

RATES = (16000, 44100, 48000)
WINLEN, STEP = 0.0512, 0.01
L10, S10 = 512, 100                       # int(10000 * WINLEN), int(STEP * 10000)


def preemph(sig, coeff=0.97):
    sig = np.asarray(sig, dtype=np.float64)
    return np.append(sig[0], sig[1:] - coeff * sig[:-1])


def chirp(rng, rate, seconds, f0=None):
    """round(6000 x hanning + 40 N(0, 1)) as float64 (integer valued, inside the int16 range)."""
    n = int(round(seconds * rate))
    t = np.arange(n) / rate
    f0 = rng.uniform(90, 300) if f0 is None else f0
    phase = 2 * np.pi * f0 * (t + 0.1 * t * t)              # instantaneous frequency f0 (1 + 0.2 t)
    x = np.zeros(n)
    for h in range(1, 7):
        x += np.sin(h * phase + rng.uniform(0, 2 * np.pi)) / h
    return np.round(6000 * x * np.hanning(n) + 40 * rng.standard_normal(n))


# seeds were kept or replaced by make_pitch_golden.py's rule: a chirp stays only if the reference's arithmetic in
# single precision gives the same track as in double precision (the manifest records the count per case)
CHIRP_SEEDS = [101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112]
ROWS_CASES = ('chirp00', 'chirp07')       # cases whose fp64 cepstrum rows are stored as well


def _chirp_case(k, seed):
    rate = RATES[k % 3]
    return dict(name=f'chirp{k:02d}', kind='chirp', seed=seed, rate=rate, preemph=bool(k % 2))


CASES = [_chirp_case(k, s) for k, s in enumerate(CHIRP_SEEDS)] + [
    dict(name='silent_tail', kind='silent_tail', seed=201, rate=16000, preemph=False),
    dict(name='short', kind='short', seed=202, rate=16000, preemph=False),
    dict(name='one_frame', kind='one_frame', seed=203, rate=16000, preemph=False),
]
CHIRPS = [c for c in CASES if c['kind'] == 'chirp']


def make_input(case):
    """-> (signal, rate): int16, or float64 after preemphasis."""
    rng = np.random.default_rng(case['seed'])
    rate = case['rate']
    if case['kind'] == 'chirp':
        x = chirp(rng, rate, rng.uniform(0.5, 1.0))
    elif case['kind'] == 'silent_tail':
        x = np.concatenate([chirp(rng, rate, 0.7), np.zeros(int(0.2 * rate))])
    elif case['kind'] == 'short':
        x = chirp(rng, rate, 0.2)
    else:
        x = chirp(rng, rate, 0.04)
    if case['preemph']:
        return preemph(x), rate
    return x.astype(np.int16), rate


def random_chirp_batch(seed, n, lo=0.3, hi=1.0):
    """n chirps at mixed rates-independent lengths, all at one rate (a batch shares its rate) -> (list of int16 clips, rate)."""
    rng = np.random.default_rng(seed)
    rate = 44100
    return [chirp(rng, rate, rng.uniform(lo, hi)).astype(np.int16) for _ in range(n)], rate
