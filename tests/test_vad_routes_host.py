"""The launch routes of dsp_vad_features_batch without a device: dsp_debug_vad_route (the function the launcher itself switches
on, csrc/kernels_vad.h: vad_route) against the table of tests/vad_route_cases.py, the table against the list of kernels the
library instantiates, and the case module's reference against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import vad_route_cases as vc
from conftest import ROOT


@pytest.fixture(scope='module')
def lib():
    from features import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return nat.load()


def _route(lib, L, S, dtype, use_sq):
    fr = C.c_int32(-1)
    fam = lib.dsp_debug_vad_route(L, S, vc.WAVE_CODE[dtype], use_sq, C.byref(fr))
    return fam, fr.value


def test_route_codes_match_the_header():
    import re
    from features import _native as nat
    hdr = open(os.path.join(ROOT, 'include', 'dsp_frontend.h')).read()
    codes = {k: int(v) for k, v in re.findall(r'#define\s+DSP_VAD_ROUTE_([A-Z_]+)\s+(\d+)', hdr)}
    assert codes == {'PER_FRAME': vc.PER_FRAME, 'SCAN': vc.SCAN, 'SUM': vc.SUM, 'TILE_ABS': vc.TILE_ABS, 'TILE_SQ': vc.TILE_SQ}
    assert (nat.VAD_PER_FRAME, nat.VAD_SCAN, nat.VAD_SUM, nat.VAD_TILE_ABS, nat.VAD_TILE_SQ) == \
           (vc.PER_FRAME, vc.SCAN, vc.SUM, vc.TILE_ABS, vc.TILE_SQ)
    assert (nat.WAVE_F32, nat.WAVE_I16) == (vc.WAVE_CODE[vc.F32], vc.WAVE_CODE[vc.I16])


@pytest.mark.parametrize('cell', sorted(vc.CELLS), ids=lambda c: f'{c[0]}x{c[1]}')
def test_route_query_returns_the_table(lib, cell):
    L, S = cell
    for dtype, use_sq in vc.COLUMNS:
        assert _route(lib, L, S, dtype, use_sq) == vc.expected(L, S, dtype, use_sq), vc.case_id(L, S, dtype, use_sq)
    assert lib.dsp_debug_vad_route(L, S, vc.WAVE_CODE[vc.I16], 0, None) == vc.expected(L, S, vc.I16, 0)[0]   # NULL: code alone


def test_route_query_follows_force_generic(lib):
    from features import _native as nat
    nat.check(lib.dsp_debug_force_generic(1))
    try:
        for (L, S) in vc.CELLS:
            for dtype, use_sq in vc.COLUMNS:
                assert _route(lib, L, S, dtype, use_sq) == (vc.PER_FRAME, 1)
    finally:
        nat.check(lib.dsp_debug_force_generic(0))
    assert _route(lib, 64, 16, vc.I16, 0) == (vc.SCAN, 16)


def test_route_query_refuses_what_the_entry_point_refuses(lib):
    from features import _native as nat
    fr = C.c_int32(-7)
    for args in ((0, 16, 1, 0), (64, 0, 1, 0), (-5, 16, 0, 0), (64, 16, 2, 0), (64, 16, -1, 1)):
        assert lib.dsp_debug_vad_route(*args, C.byref(fr)) == nat.EINVAL and fr.value == -7, args


def test_table_covers_every_instantiated_kernel():
    """A cell cannot be dropped silently: every (family, frames per wave, sample type) the library instantiates is the expected
    route of at least one cell, with use_sq 0 and 1 where the family takes both."""
    seen, seen_sq = set(), set()
    for (L, S) in vc.CELLS:
        for dtype, use_sq in vc.COLUMNS:
            fam, fr = vc.expected(L, S, dtype, use_sq)
            seen.add((fam, fr, dtype))
            seen_sq.add((fam, fr, dtype, use_sq))
    assert seen == vc.INSTANTIATED, seen ^ vc.INSTANTIATED
    for fam, fr, dtype in vc.INSTANTIATED:
        if fam in (vc.SCAN, vc.TILE_ABS):
            want = {0}
        elif fam == vc.TILE_SQ or (fam == vc.SUM and dtype == vc.I16):      # int16 sums of |x| all go to the scan kernel
            want = {1}
        else:
            want = {0, 1}
        assert {q for q in (0, 1) if (fam, fr, dtype, q) in seen_sq} == want, (fam, fr, dtype)
    for fam, fr, dtype, use_sq in vc.MULTI_ROUND:
        assert vc.expected(*vc.smallest_cell(fam, fr, dtype, use_sq), dtype, use_sq) == (fam, fr)
    assert len(vc.CELLS) == 15


@pytest.mark.parametrize('cell', [(64, 16), (661, 661), (1323, 441)], ids=lambda c: f'{c[0]}x{c[1]}')
def test_reference_equals_the_oracle(cell):
    """The case module's sums against dsp_oracle.get_amplitude(...) * L and dsp_oracle.get_zcr on fp64 copies of the frames.
    int16: mean * L is within 2^-52 of a sum below 2^42 relatively, so rounding it recovers the integer.  fp32: the oracle's fp64
    sum of L terms (at most (L - 1) 2^-53 relatively) and its two roundings (divide, multiply back): (L + 2) 2^-52 is ample."""
    from oracle import dsp_oracle
    L, S = cell
    for dtype in (vc.I16, vc.F32):
        for use_sq in (0, 1):
            flat, so = vc.ragged_batch(L, S, dtype, use_sq)
            amp, zcr, fo = vc.reference(flat, so, L, S, use_sq)
            for b in range(len(so) - 1):
                clip = flat[so[b]:so[b + 1]].astype(np.float64)
                frames = dsp_oracle.framesig(clip, L, S)
                assert frames.shape == (fo[b + 1] - fo[b], L)
                want = np.array(dsp_oracle.get_amplitude(frames, use_sq=bool(use_sq)), dtype=np.float64) * L
                got = amp[fo[b]:fo[b + 1]]
                if dtype == vc.I16:
                    assert np.array_equal(np.rint(want).astype(np.int64), got)
                else:
                    assert np.all(np.abs(want.astype(np.longdouble) - got) <= (L + 2) * 2.0 ** -52 * got)
                assert np.array_equal(np.array(dsp_oracle.get_zcr(frames), dtype=np.int64), zcr[fo[b]:fo[b + 1]])


def test_ragged_clip_lists_have_the_librarys_frame_counts(lib):
    from features import _native as nat
    for (L, S) in vc.CELLS:
        for dtype, use_sq in vc.COLUMNS:
            fr = vc.expected(L, S, dtype, use_sq)[1]
            lens = vc.clip_lengths(L, S, fr)
            assert lens[0] == 0 and lens[-1] == 0 and {1, 3, L - 1, L, L + 1, (fr - 1) * S + L} <= set(lens)
            flat, so = vc.ragged_batch(L, S, dtype, use_sq)
            assert np.array_equal(np.diff(so), lens) and flat.dtype == np.dtype(dtype) and len(flat) == so[-1]
            fo = nat.frame_offsets(so, L, S)
            assert np.array_equal(vc.frames_of(flat, so, L, S)[1], fo)
            assert np.array_equal(np.diff(fo), vc.frame_counts(lens, L, S))
        for rem in (0, 1):
            x = vc.dense_batch(L, S, vc.F32, 0, rem)
            assert x.shape[0] == 5 and x.shape[1] % 4 == rem
