"""Cepstral pitch path, the part that needs no GPU: the names pitch_model.py star-imports, the C ABI's declarations, the
band-pass taps, the argument checks (they return before any launch), and the NumPy restatement
(tests/pitch_cepstrum_ref.py, the checker of the random GPU batches) against the stored reference outputs."""
import os
import re

import numpy as np
import pytest

import pitch_cepstrum_ref as ref
from pitch_cepstrum_cases import CASES, CHIRPS, ROWS_CASES, make_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ('dsp_pitch_cepstrum_batch', 'dsp_pitch_cepstrum_track_batch', 'dsp_pitch_feature_batch',
                    'dsp_pitch_smooth_subseq_batch')


@pytest.fixture(scope='module')
def pgold():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'pitch_cepstrum_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def test_star_import_yields_what_pitch_model_needs():
    """pitch_model.py does `from features.pitch import *` and then uses these names (pitch_model.py:38-73)."""
    ns = {}
    exec('from features.pitch import *', ns)
    for name in ('pitch_feature', 'pitch_detect', 'pitch_detect_frame', 'peak_score', 'sub_endpoint_detect',
                 'find_smooth_subsequence', 'slope', 'quad_params', 'peakshift', 'basic_endpoint_detection',
                 'robust_endpoint_detection', 'get_amplitude', 'preemphasis', 'to_frames', 'window', 'acr', 'downsampling',
                 'pickle', 'np', 'pitch_detect_sr', 'smooth', 'robust_max_pitch', 'center_clip'):
        assert name in ns, name
    import features.pitch as fp
    src = open(fp.__file__).read()
    assert not re.search(r'^\s*(import|from)\s+(sklearn|matplotlib)', src, re.M)
    import features
    for name in ('pitch_feature', 'pitch_detect', 'pitch_feature_batch', 'pitch_features_device'):
        assert hasattr(features, name), name


def test_new_entry_points_are_declared_exported_and_bound():
    from features import _native as nat
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    lib = nat.load()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', hdr), f'{name} is not declared in the header'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in nat.SIGNATURES, f'{name} has no ctypes signature'
    assert re.search(r'pitch\.py:\d+', hdr[hdr.index('dsp_pitch_cepstrum_batch') - 1500:])   # cites the lines it serves
    mk = open(os.path.join(ROOT, 'dsp-speech-recognition_amd', 'csrc', 'Makefile')).read()
    # the library is rebuilt when the header changes: the compiler writes the dependencies (-MMD) and the Makefile reads them
    assert re.search(r'-MMD -MP -c\b', mk) and re.search(r'^-include \$\(OBJS:\.o=\.d\)', mk, re.M)
    dep = os.path.join(ROOT, 'dsp-speech-recognition_amd', 'lib', 'obj', 'libdsp_frontend', 'dsp_frontend.d')
    if os.path.exists(dep):
        assert 'kernels_cepstrum.h' in open(dep).read()


def test_argument_checks_return_before_any_launch():
    """NULL buffers, empty batches and frame lengths the kernels do not serve are DSP_EINVAL with a message."""
    from features import _native as nat
    lib = nat.load()
    one = 0x1000                                         # never dereferenced: every call below is rejected first
    assert lib.dsp_pitch_cepstrum_batch(one, one, one, 1, 1, 0, 500, 100, one, 1, one, None, None) == nat.EINVAL
    assert b'500' in lib.dsp_last_error() and b'power of two' in lib.dsp_last_error()
    for L in (64, 2048, 0, -512, 384):
        assert lib.dsp_pitch_cepstrum_batch(one, one, one, 1, 1, 0, L, 100, one, 1, one, None, None) == nat.EINVAL
        assert lib.dsp_pitch_cepstrum_track_batch(one, 0, one, 1, L, 3, one, None, None) == nat.EINVAL
    assert lib.dsp_pitch_cepstrum_batch(one, one, one, 1, 1, 0, 512, 100, None, 1, one, None, None) == nat.EINVAL
    assert lib.dsp_pitch_cepstrum_batch(one, one, one, 1, 1, 0, 512, 100, one, 1, None, None, None) == nat.EINVAL
    assert lib.dsp_pitch_cepstrum_batch(None, one, one, 1, 1, 0, 512, 100, one, 1, one, None, None) == nat.EINVAL
    assert lib.dsp_pitch_cepstrum_batch(one, one, one, 0, 1, 0, 512, 100, one, 1, one, None, None) == nat.EINVAL
    assert lib.dsp_pitch_cepstrum_batch(one, one, one, 1, 1, 0, 512, 0, one, 1, one, None, None) == nat.EINVAL
    assert lib.dsp_pitch_cepstrum_batch(one, None, None, 1, 1, 0, 512, 100, one, 1, one, None, None) == nat.EINVAL
    assert lib.dsp_pitch_cepstrum_track_batch(None, 0, one, 1, 512, 3, one, None, None) == nat.EINVAL
    assert lib.dsp_pitch_cepstrum_track_batch(one, 0, one, 0, 512, 3, one, None, None) == nat.EINVAL
    assert lib.dsp_pitch_cepstrum_track_batch(one, 0, one, 1, 512, 3, None, one, None) == nat.EINVAL     # arg-max needs d_pitch
    assert lib.dsp_pitch_cepstrum_track_batch(one, 0, one, 1, 512, 0, None, None, None) == nat.EINVAL    # nothing to write
    assert lib.dsp_pitch_cepstrum_track_batch(one, 0, one, 1, 512, 4, one, one, None) == nat.EINVAL      # unknown flag
    assert lib.dsp_pitch_feature_batch(one, None, one, 1, one, one, one, None) == nat.EINVAL
    assert lib.dsp_pitch_feature_batch(one, one, one, 0, one, one, one, None) == nat.EINVAL
    assert lib.dsp_pitch_feature_batch(one, one, one, 1, None, one, one, None) == nat.EINVAL             # a track needs d_seg
    assert lib.dsp_pitch_feature_batch(one, one, one, 1, one, one, None, None) == nat.EINVAL
    assert lib.dsp_pitch_smooth_subseq_batch(None, one, 1, 3, 30.0, one, one, None) == nat.EINVAL
    assert lib.dsp_pitch_smooth_subseq_batch(one, one, 0, 3, 30.0, one, one, None) == nat.EINVAL
    assert lib.dsp_pitch_smooth_subseq_batch(one, one, 1, 0, 30.0, one, one, None) == nat.EINVAL
    assert lib.dsp_last_error()


def test_bandpass_taps_of_the_cepstral_band():
    from features.pitch import bandpass_taps
    h = bandpass_taps(512, 10000, 50, 1000, 'hamming')
    assert h.shape == (512,) and np.iscomplexobj(h)
    Hd = np.fft.fft(h / (2 * np.pi * np.hamming(512))).real
    on = np.flatnonzero(Hd > 0.5)
    assert on[0] == 2 and on[-1] == 50 and len(on) == 49          # support [2, 51)
    assert np.allclose(h, ref.taps(512), rtol=0, atol=1e-15)
    assert np.max(np.abs(h - bandpass_taps(512, 10000, 50, 900, 'hamming'))) > 1e-3   # not the score path's band


def test_golden_file_covers_the_cases(pgold):
    import json
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'pitch_cepstrum_manifest.json')))
    assert len(CHIRPS) == 12
    assert sum(len(pgold[f"{c['name']}/pitch"]) for c in CHIRPS) >= 800
    for c in CASES:
        m = man['cases'][c['name']]
        assert m['seed'] == c['seed']
        if c['kind'] == 'chirp':
            assert m['fp32_track_frames_differing'] == 0       # the reference's arithmetic in fp32 keeps these tracks
        assert bool(pgold[f"{c['name']}/raises"]) == (c['name'] == 'one_frame')
    for name in ROWS_CASES:
        assert pgold[f'{name}/rows'].dtype == np.float64 and pgold[f'{name}/rows'].shape[1] == 512
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'pitch_cepstrum_golden.npz')) < (1 << 20)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_restatement_reproduces_the_reference(case, pgold):
    """rows <= 1e-12 normwise, scores, pitch, p and segments exact, feat within 1e-9 max(1, |ref|)."""
    name = case['name']
    sig, rate = make_input(case)
    r = ref.full(sig, rate)
    g = {k.split('/', 1)[1]: v for k, v in pgold.items() if k.startswith(name + '/')}
    assert len(r['pitch']) == int(g['n_frames'])
    if 'rows' in g:
        for t in range(len(g['rows'])):
            a, b = r['rows'][t], g['rows'][t]
            assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), (name, t)
            assert np.max(np.abs(a[1:] - b[1:])) <= 1e-12 * np.max(np.abs(b)), (name, t)
    assert np.array_equal(r['scores'], g['scores']), name
    assert np.array_equal(r['pitch'], g['pitch']), name
    if g['raises']:
        assert not r['valid'] and np.isnan(r['feat']).all()
        return
    assert r['valid']
    assert r['p'] == int(g['p'])
    assert np.array_equal(r['seg1'], g['seg1']) and tuple(r['idx1']) == tuple(g['idx1'])
    assert np.array_equal(r['seg2'], g['seg2']) and tuple(r['idx2']) == tuple(g['idx2'])
    assert np.all(np.abs(r['feat'] - g['feat']) <= 1e-9 * np.maximum(1.0, np.abs(g['feat']))), (r['feat'], g['feat'])


def test_edge_cases_are_what_the_issue_describes(pgold):
    """silent_tail: 500.0 from the frame before the first silent one to the end; short: p = T // 2 with p_bias = 0 and the
    segments (0, 8), (8, 16)."""
    sig, rate = make_input(next(c for c in CASES if c['name'] == 'silent_tail'))
    F = ref.frames_of(ref.decimate(sig, rate))
    silent = np.flatnonzero(~F.any(axis=1))
    assert len(silent) >= 10
    pitch = pgold['silent_tail/pitch']
    assert np.all(pitch[silent[0] - 1:] == 500.0) and not np.all(pitch[:silent[0] - 1] == 500.0)
    assert int(pgold['short/n_frames']) == 16 and int(pgold['short/p']) == 8
    assert tuple(pgold['short/idx1']) == (0, 8) and tuple(pgold['short/idx2']) == (8, 16)
    assert int(pgold['one_frame/n_frames']) == 1


def test_orthogonal_fit_equals_polyfit():
    """The kernel's closed form of the leading least-squares coefficients (centred, orthogonal basis) against
    numpy.polyfit, which the reference calls."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(300):
        m = int(rng.integers(3, 90))
        y = np.round(rng.uniform(80, 400, m), 2)
        x = np.arange(m) - (m - 1) / 2
        q = x * x - (m * m - 1) / 12
        got = np.array([np.sum(x * y) / np.sum(x * x), np.sum(q * y) / np.sum(q * q)])
        want = np.array([np.polyfit(np.arange(m), y, 1)[0], np.polyfit(np.arange(m), y, 2)[0]])
        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))))
    assert worst <= 1e-11, worst
