"""Every launch route of dsp_vad_features_batch (csrc/kernels_vad.h: per-frame, scan 16 / 8 / 4, sum 16 / 4, tile-abs 16 / 4,
tile-sq 16 / 4, both sample types, sums of |x| and of x^2) against the NumPy reference of tests/vad_route_cases.py: every
frame of every clip, int16 exact, fp32 within L 2^-52, zero-crossing counts exact.  The route is asserted from
dsp_debug_vad_route -- the function the launcher switches on -- before each launch."""
import ctypes as C

import numpy as np
import pytest

import vad_route_cases as vc
from conftest import record

pytestmark = pytest.mark.gpu

FRONT, BACK, CANARY = 16, 64, 8          # elements in front of / behind the samples (FRONT: a whole vector of either type); rows behind the results


class _Wave:
    """The samples `off` elements past a 16-byte boundary inside a larger device buffer."""

    def __init__(self, nat, flat, off):
        host = np.zeros(FRONT + off + flat.size + BACK, dtype=flat.dtype)
        host[FRONT + off:FRONT + off + flat.size] = flat.reshape(-1)
        self.buf = nat.DeviceBuffer(host.nbytes).upload(host)
        self.ptr = self.buf.ptr + (FRONT + off) * flat.dtype.itemsize


def _upload(nat, a):
    a = np.ascontiguousarray(a)
    return nat.DeviceBuffer(a.nbytes).upload(a)


def _launch(nat, lib, wave, dtype, so, fo, uniform, L, S, use_sq, layout=None):
    """-> (amp fp64 [F], zcr int32 [F]); the result buffers start as NaN / -1 and every row must have been written, none behind."""
    F = int(fo[-1])
    d_amp = _upload(nat, np.full(F + CANARY, np.nan))
    d_zcr = _upload(nat, np.full(F + CANARY, -1, dtype=np.int32))
    d_so, d_fo = (None, None) if uniform else (_upload(nat, so), _upload(nat, fo))
    code = vc.WAVE_CODE[dtype]
    if layout is not None:
        nat.check(lib.dsp_vad_features_layout_batch(layout, wave.ptr, code, d_so.ptr, d_fo.ptr, use_sq, d_amp.ptr, d_zcr.ptr, None))
    else:
        nat.check(lib.dsp_vad_features_batch(wave.ptr, code, d_so.ptr if d_so else None, d_fo.ptr if d_fo else None, len(so) - 1, F,
                                             uniform, L, S, use_sq, d_amp.ptr, d_zcr.ptr, None))
    amp = d_amp.download((F + CANARY,), np.float64)
    zcr = d_zcr.download((F + CANARY,), np.int32)
    assert np.isnan(amp[F:]).all() and (zcr[F:] == -1).all(), 'rows behind the batch were written'
    assert not np.isnan(amp[:F]).any() and (zcr[:F] >= 0).all(), ('rows not written', np.flatnonzero(np.isnan(amp[:F]))[:5])
    return amp[:F], zcr[:F]


def _assert_route(lib, L, S, dtype, use_sq, want):
    fr = C.c_int32(-1)
    fam = lib.dsp_debug_vad_route(L, S, vc.WAVE_CODE[dtype], use_sq, C.byref(fr))
    assert (fam, fr.value) == want, (L, S, dtype, use_sq)


def _record(dtype, use_sq, rel):
    if dtype == vc.F32:
        record('vad_route_sq_f32_rel' if use_sq else 'vad_route_abs_f32_rel', rel)


MATRIX = [(L, S, dtype, use_sq) for (L, S) in sorted(vc.CELLS) for dtype, use_sq in vc.COLUMNS]


@pytest.mark.parametrize('L,S,dtype,use_sq', MATRIX, ids=[vc.case_id(*c) for c in MATRIX])
def test_vad_route_matrix(L, S, dtype, use_sq):
    """One cell x sample type x use_sq: the ragged batch with its base pointer 0, 1 and 3 elements past a vector boundary (the
    last two are launched as ragged batches of the aligned buffer: fused_kernel_view), and two dense batches of five clips,
    N % 4 == 0 and N % 4 == 1 (the second takes the view as well)."""
    from features import _native as nat
    lib = nat.load()
    _assert_route(lib, L, S, dtype, use_sq, vc.expected(L, S, dtype, use_sq))
    flat, so = vc.ragged_batch(L, S, dtype, use_sq)
    amp, zcr, fo = vc.reference(flat, so, L, S, use_sq)
    assert np.array_equal(fo, nat.frame_offsets(so, L, S))
    for off in (0, 1, 3):
        got = _launch(nat, lib, _Wave(nat, flat, off), dtype, so, fo, 0, L, S, use_sq)
        _record(dtype, use_sq, vc.compare(*got, amp, zcr, L, f'ragged, base + {off}'))
    for rem in (0, 1):
        x = vc.dense_batch(L, S, dtype, use_sq, rem)
        dso = vc.dense_offsets(x)
        amp, zcr, fo = vc.reference(x.reshape(-1), dso, L, S, use_sq)
        got = _launch(nat, lib, _Wave(nat, x, 0), dtype, dso, fo, x.shape[1], L, S, use_sq)
        _record(dtype, use_sq, vc.compare(*got, amp, zcr, L, f'dense, N = {x.shape[1]}'))


@pytest.mark.parametrize('dtype', [vc.I16, vc.F32])
@pytest.mark.parametrize('cell', [(64, 16), (661, 661), (1323, 441)], ids=lambda c: f'{c[0]}x{c[1]}')
def test_vad_layout_handle_with_and_without_squares(cell, dtype):
    """dsp_vad_features_layout_batch reads the handle's prebuilt group tables: byte-identical to the table-building call and
    equal to the reference, use_sq 0 and 1.  At (1323, 441) int16 sums of |x| read the eight-frame tables of the handle and sums
    of x^2 the four-frame ones."""
    from features import _native as nat
    lib = nat.load()
    L, S = cell
    if cell == (1323, 441) and dtype == vc.I16:
        _assert_route(lib, L, S, dtype, 0, (vc.SCAN, 8))
        _assert_route(lib, L, S, dtype, 1, (vc.TILE_SQ, 4))
    for use_sq in (0, 1):
        _assert_route(lib, L, S, dtype, use_sq, vc.expected(L, S, dtype, use_sq))
        flat, so = vc.ragged_batch(L, S, dtype, use_sq)
        amp, zcr, fo = vc.reference(flat, so, L, S, use_sq)
        wave = _Wave(nat, flat, 0)
        d_fo = _upload(nat, fo)
        handle = C.c_void_p(0)
        nat.check(lib.dsp_layout_create(d_fo.ptr, len(so) - 1, int(fo[-1]), L, S, None, C.byref(handle)))
        try:
            for q in (use_sq, 1 - use_sq, use_sq):                  # one handle serves both, in any order
                a, z, _ = vc.reference(flat, so, L, S, q)
                with_tables = _launch(nat, lib, wave, dtype, so, fo, 0, L, S, q, layout=handle)
                building = _launch(nat, lib, wave, dtype, so, fo, 0, L, S, q)
                assert with_tables[0].tobytes() == building[0].tobytes() and with_tables[1].tobytes() == building[1].tobytes()
                _record(dtype, q, vc.compare(*with_tables, a, z, L, f'layout handle, use_sq = {q}'))
        finally:
            nat.check(lib.dsp_layout_destroy(handle))


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'ragged'])
@pytest.mark.parametrize('route', vc.MULTI_ROUND, ids=[f'{vc.FAMILY_NAMES[r[0]]}{r[1]}-{r[2]}-{"sq" if r[3] else "abs"}' for r in vc.MULTI_ROUND])
def test_vad_second_trip_round_the_group_loop(route, ragged):
    """More groups than waves can be resident: 1.25 x (8 workgroups per CU, the largest cap in kernels_vad.h, x 4 waves x CUs),
    so every wave of every route stages a second group into the LDS it has just read (F512_FENCE; the scan kernel's
    `locate` of the next group).  Every frame is checked."""
    import torch
    from features import _native as nat
    lib = nat.load()
    fam, fr, dtype, use_sq = route
    L, S = vc.smallest_cell(fam, fr, dtype, use_sq)
    _assert_route(lib, L, S, dtype, use_sq, (fam, fr))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    min_groups = -(-5 * vc.MAX_WORKGROUPS_PER_CU * vc.WAVES_PER_WORKGROUP * cus // 4)
    if ragged:
        flat, so = vc.multi_round_batch(L, S, dtype, fr, min_groups, True)
        uniform = 0
    else:
        x = vc.multi_round_batch(L, S, dtype, fr, min_groups, False)
        flat, so, uniform = x.reshape(-1), vc.dense_offsets(x), x.shape[1]
    amp, zcr, fo = vc.reference(flat, so, L, S, use_sq)
    assert int(np.sum(-(-np.diff(fo) // fr))) >= min_groups
    got = _launch(nat, lib, _Wave(nat, flat, 0), dtype, so, fo, uniform, L, S, use_sq)
    _record(dtype, use_sq, vc.compare(*got, amp, zcr, L, 'multi-round'))


@pytest.mark.parametrize('dtype', [np.int16, np.float64])
@pytest.mark.parametrize('shape', [(7, 661), (7, 480), (3, 48), (2, 3070)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_public_get_amplitude_and_get_zcr_on_frame_matrices(shape, dtype):
    """features.get_amplitude(frames, use_sq=...) and features.get_zcr(frames) on explicit frame matrices (hop == length)
    against the oracle on fp64 copies.  float64 input is rounded to fp32 first, as the package does.  int16: EQUAL (either
    side divides the same exact integer by L).  float: within L 2^-52 of the oracle, relatively -- two fp64 sums of L
    non-negative terms in different orders, (L - 1) 2^-53 each, and one rounding of each division; the same bar against
    the case module's long-double sums."""
    import features
    from oracle import dsp_oracle
    T, L = shape
    rng = np.random.default_rng(T * 10000 + L)
    if dtype == np.int16:
        frames = np.stack([vc.samples(vc.I16, L, rng, k) for k in range(T)])
        f64 = frames.astype(np.float64)
    else:
        frames = vc.samples(vc.F32, T * L, rng).reshape(T, L).astype(np.float64) * (1 + 2.0 ** -30)     # not representable in fp32
        f64 = frames.astype(np.float32).astype(np.float64)
    assert np.array_equal(np.array(features.get_zcr(frames), dtype=np.int64), np.array(dsp_oracle.get_zcr(f64), dtype=np.int64))
    for use_sq in (False, True):
        got = np.array(features.get_amplitude(frames, use_sq=use_sq), dtype=np.float64)
        flat = frames.reshape(-1) if dtype == np.int16 else f64.astype(np.float32).reshape(-1)
        want_sum, _, _ = vc.reference(flat, np.arange(T + 1, dtype=np.int64) * L, L, L, int(use_sq))
        oracle = np.array(dsp_oracle.get_amplitude(f64, use_sq=use_sq), dtype=np.float64)
        if dtype == np.int16:
            assert np.array_equal(got, oracle)
            assert np.array_equal(got, want_sum.astype(np.float64) / L)
        else:
            bound = L * 2.0 ** -52
            assert np.all(np.abs(got - oracle) <= bound * oracle)
            assert np.all(np.abs(got.astype(np.longdouble) * L - want_sum) <= bound * want_sum)
