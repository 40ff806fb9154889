"""tools/pipe_cycles.py on a hand-written listing: what lies in a marked cold block is left out, the c0 block is reported
on its own, a bracket is widened to its basic block, and the prices are the two tables'."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

LISTING = """\
_Z14mfcc512_kernelTESTv:
	s_load_dword s0, s[4:5], 0x0
.LBB0_1:
	v_add_f32_e32 v0, v1, v2
	s_cbranch_scc1 .LBB0_3
	v_add_u32_e32 v9, v9, v9
	; F512_PATH slow_stage begin
	ds_write_b128 v3, v[4:7]
	; F512_PATH slow_stage end
	v_mul_f32_e32 v9, v9, v9
.LBB0_3:
	; F512_FAST_STAGE
	global_load_dwordx4 v[4:7], v[8:9], off
	s_waitcnt vmcnt(0)
	ds_write_b128 v3, v[4:7]
	v_pk_mul_f32 v[0:1], v[2:3], v[4:5]
	s_and_saveexec_b64 s[0:1], vcc
	s_cbranch_execz .LBB0_5
	v_fma_f32 v1, v1, v1, v1
	; F512_PATH c0 begin
	; F512_PATH c0 end
	v_mov_b32_e32 v2, v1
.LBB0_5:
	ds_write2_b32 v3, v1, v2 offset0:1 offset1:9
	ds_read_b128 v[4:7], v3
	s_cbranch_scc1 .LBB0_7
	; F512_PATH repair begin
	v_log_f32_e32 v1, v1
	; F512_PATH repair end
.LBB0_7:
	s_cbranch_scc1 .LBB0_9
	; F512_PATH clamp begin
	ds_read_b64 v[4:5], v3
	; F512_PATH clamp end
.LBB0_9:
	ds_write_b32 v3, v1
	s_branch .LBB0_1
	s_endpgm
"""


def test_hot_path_of_a_small_listing(tmp_path, capsys):
    import pipe_cycles as pc
    src = tmp_path / 'k.s'
    src.write_text(LISTING)
    valu, lds = pc.report('mfcc512_kernelTEST', str(src))
    out = capsys.readouterr().out
    # hot: v_add_f32, v_pk_mul; c0 (widened to its block): v_fma, v_mov; the slow block's three vector ops are left out
    assert valu == pytest.approx(2.26 + 3.9 + 2.26 + 2.0)
    assert 'c == 0 branch      4 cycles: f32=1 mov=1' in out
    # ds_write_b128 13, ds_write2_b32 6, ds_read_b128 4, ds_write_b32 4; the clamp block's read and the slow store are out
    assert lds == 13 + 6 + 4 + 4
    assert 'left out: 1 clamp, 1 repair, 3 slow_stage instructions' in out
    assert 'vector memory 1' in out


def test_a_block_laid_out_in_pieces_is_an_error(tmp_path):
    import pipe_cycles as pc
    src = tmp_path / 'k.s'
    src.write_text(LISTING.replace('\t; F512_PATH repair begin\n', ''))
    with pytest.raises(SystemExit):
        pc.report('mfcc512_kernelTEST', str(src))
