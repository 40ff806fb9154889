"""Mixed-rate batches through one recorded launch sequence (features.model_glue.MixedRateCapacityBatch,
features.train.MixedRateTrainBatch; include/dsp_frontend.h: dsp_rate_groups_batch, dsp_gather_groups_batch,
dsp_scatter_segments_batch, dsp_model_finalize_placed_batch with negative columns).

  A  the partition kernel alone (tables only, no audio) against the restatement of tests/mixed_capacity_cases.py under ``==``,
     canary words behind every table;
  B  the gather: ``array_equal`` against NumPy, pad slots, canaries behind offsets_g[B];
  C  the placed finalize kernel with negative columns on the placement test's shapes: skipped clips leave the sentinel, the
     others equal the unskipped call in every bit;
  D  ``MixedRateCapacityBatch``: one capture, five replays, against the eager exact-shape ``MixedRateFeatureBatch.run`` on the same
     device clips (len0 and endpoints exact, rows per clip within 5e-5 normwise: the project's bar between two device routes --
     the gather can change a clip's alignment and the fp64 sums depend on order); ``run(capacity=)`` equals the replay in every
     byte; the two golden clips of the real reference within 1e-4;
  E  ``MixedRateTrainBatch``: three replays equal three eager ``run(capacity=)`` steps in every bit of every loss, parameter and
     moment; the first step against parent code (``MixedRateFeatureBatch.run``, the head, cross-entropy, backward): logits within
     2e-5 max(1, max |ref|), every gradient tensor within 2e-5 normwise (max |a - b| / max |ref|);
  F  the refusals.

Measured on the MI355X: D is bit-equal (normwise 0 on every clip of every vector, with and without jitter), the golden clips are
within 5.7e-6, and E's first step equals the parent route in every bit of the logits and of every gradient tensor."""
import copy
import ctypes
import random

import numpy as np
import pytest

import capacity_cases as cc
import mixed_capacity_cases as mc
from conftest import normwise, record
from golden_cases import case_by_name, make_signal

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = np.float32(-7.5e33)               # never a result (tests/test_gpu_mixed_rate.py)
SENT32 = np.int32(0x7fc0beef)
SENT_TAB = -7777                         # never a table word: picks are >= -1, offsets and counts >= 0
POOL = (44100, 48000, 16000, 8000)
C = 13


@pytest.fixture(scope='module')
def env():
    import types

    import torch
    from features import _native as nat
    nat.require_device()
    return types.SimpleNamespace(nat=nat, lib=nat.load(), torch=torch, dev=torch.device('cuda', 0))


def _np(t):
    return t.detach().cpu().numpy()


def _dev(env, a):
    return env.torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)


def _guarded(env, n, dtype, sent=SENT_TAB):
    return env.torch.full((n + GUARD,), sent, dtype=dtype, device=env.dev)


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# ---- A: the partition kernel alone ----------------------------------------------------------------------------------------------

def _partition_on_device(env, rates, so_in, table, pad, cap, jitter=None):
    """-> the structure of ``mc.partition`` read back from the device; asserts the canaries behind every table."""
    torch, nat = env.torch, env.nat
    B, G = len(rates), len(table)
    d_r, d_in = _dev(env, np.asarray(rates, dtype=np.int32)), _dev(env, np.asarray(so_in, dtype=np.int64))
    d_j = None if jitter is None else _dev(env, np.asarray(jitter, dtype=np.int64).reshape(B, 2))
    san = _guarded(env, B + 1, torch.int64)
    pick = [_guarded(env, B, torch.int32) for _ in range(G)]
    col = [_guarded(env, B, torch.int32) for _ in range(G)]
    off = [_guarded(env, B + 1, torch.int64) for _ in range(G)]
    jit = [_guarded(env, 2 * B, torch.int64) for _ in range(G)]
    count, status = _guarded(env, G, torch.int32), _guarded(env, 1, torch.int32)
    h_rates = (ctypes.c_int32 * G)(*table)
    nat.check(env.lib.dsp_rate_groups_batch(d_r.data_ptr(), d_in.data_ptr(), None if d_j is None else d_j.data_ptr(), B, cap, G, h_rates,
                                            pad, san.data_ptr(), _ptrs(pick), _ptrs(col), _ptrs(off), None if d_j is None else _ptrs(jit),
                                            count.data_ptr(), status.data_ptr(), torch.cuda.current_stream(env.dev).cuda_stream))
    torch.cuda.synchronize(env.dev)
    for name, tabs, n in (('sanitised', [san], B + 1), ('pick', pick, B), ('dst_col', col, B), ('offsets', off, B + 1),
                          ('jitter', jit, 2 * B if d_j is not None else 0), ('count', [count], G), ('status', [status], 1)):
        for g, t in enumerate(tabs):
            assert np.all(_np(t)[n:] == SENT_TAB), f'{name}[{g}]: a word behind the table was written'
    groups = [dict(pick=_np(pick[g])[:B], dst_col=_np(col[g])[:B], offsets=_np(off[g])[:B + 1],
                   jitter=None if d_j is None else _np(jit[g])[:2 * B].reshape(B, 2)) for g in range(G)]
    return dict(sanitised=_np(san)[:B + 1], status=int(_np(status)[0]), count=_np(count)[:G], groups=groups)


def _same_partition(got, want, what):
    assert got['status'] == want['status'], (what, got['status'], want['status'])
    assert np.array_equal(got['sanitised'], want['sanitised']), what
    assert np.array_equal(got['count'], want['count']), (what, got['count'], want['count'])
    for g, (a, b) in enumerate(zip(got['groups'], want['groups'])):
        for key in ('pick', 'dst_col', 'offsets'):
            assert np.array_equal(a[key], b[key]), (what, g, key)          # == on every word: none kept the fill value
        if b['jitter'] is not None:
            assert np.array_equal(a['jitter'], b['jitter']), (what, g, 'jitter')


@pytest.mark.parametrize('B', [1, 5, 64, 1500])
def test_a_partition_kernel(env, B):
    rng = np.random.default_rng(B)
    lens = rng.integers(3, 2000, B)
    so = cc.offsets_of(lens)
    cap = int(so[-1]) + 2
    jitter = rng.integers(-4800, 4800, (B, 2))
    for G in (1, 2, 4):
        table = POOL[:G]
        vectors = {'seeded': mc.rate_vector(B, table, 10 * B + G), 'one group': np.full(B, table[-1], dtype=np.int32)}
        if G >= 2:
            vectors['first rate absent'] = mc.rate_vector(B, table, B + G, absent=table[0])
            vectors['last rate absent'] = mc.rate_vector(B, table, 1000 + B - G, absent=table[-1])
        unknown = vectors['seeded'].copy()
        unknown[B // 2] = 12345
        vectors['unknown rate'] = unknown
        for what, rates in vectors.items():
            for pad, jit in ((1, jitter), (3, None)):
                want = mc.partition(rates, so, table, pad, cap, jit)
                got = _partition_on_device(env, rates, so, table, pad, cap, jit)
                _same_partition(got, want, (G, what, pad))
                assert want['status'] == (mc.BIT_UNKNOWN_RATE if what == 'unknown rate' else 0)
        assert B // 2 in mc.partition(unknown, so, table, 1, cap)['groups'][0]['pick']          # the unknown clip sits in group 0
        if G == 2:
            for bit, bad in cc.invalid_tables(so, cap).items():
                want = mc.partition(vectors['seeded'], bad, table, 2, cap, jitter)
                got = _partition_on_device(env, vectors['seeded'], bad, table, 2, cap, jitter)
                assert want['status'] == bit
                _same_partition(got, want, (G, 'status bit', bit))
                for grp in got['groups']:          # whatever the caller wrote: monotone and inside the group's capacity
                    assert grp['offsets'][0] == 0 and np.all(np.diff(grp['offsets']) >= 0) and grp['offsets'][-1] <= cap + 2 * B
            wild = rng.integers(-50, 3 * cap, B + 1)
            wild[0] = 9
            got = _partition_on_device(env, unknown, wild, table, 1, cap, jitter)
            _same_partition(got, mc.partition(unknown, wild, table, 1, cap, jitter), 'wild')
            again = _partition_on_device(env, unknown, wild, table, 1, cap, jitter)          # the same bits on every run
            _same_partition(again, got, 'second run')


# ---- B: the gather --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.int16, np.float32])
def test_b_gather_groups(env, dtype):
    torch, nat = env.torch, env.nat
    lens = [1, 7, 8, 9, 4097, 5, 4097, 8]
    rates = np.array([44100, 48000, 48000, 44100, 48000, 16000, 44100, 16000], dtype=np.int32)
    table = (44100, 48000, 16000, 8000)                      # the last group: pads only
    B, G = len(lens), len(table)
    so = cc.offsets_of(lens)
    cap = int(so[-1]) + 11
    rng = np.random.default_rng(3)
    src = rng.integers(-30000, 30000, cap).astype(dtype)
    src[src == mc.PAD_VALUE] = 2
    code = nat.WAVE_I16 if dtype == np.int16 else nat.WAVE_F32
    tdtype = torch.int16 if dtype == np.int16 else torch.float32
    sent = dtype(-12321)
    for pad in (1, 5):
        part = mc.partition(rates, so, table, pad, cap)
        d_san = _dev(env, part['sanitised'])
        d_pick = [_dev(env, g['pick']) for g in part['groups']]
        d_off = [_dev(env, g['offsets']) for g in part['groups']]
        for s_shift in (0, 1, 3, 8):                         # the source need not start on a vector; the group buffers must
            d_src = torch.zeros(cap + s_shift, dtype=tdtype, device=env.dev)
            d_src[s_shift:].copy_(_dev(env, src))
            outs = [torch.full((cap + B * pad + GUARD,), sent.item(), dtype=tdtype, device=env.dev) for _ in range(G)]
            assert all(o.data_ptr() % 16 == 0 for o in outs)
            nat.check(env.lib.dsp_gather_groups_batch(d_src[s_shift:].data_ptr(), code, d_san.data_ptr(), B, G, _ptrs(d_pick), _ptrs(d_off),
                                                      pad, _ptrs(outs), None))
            torch.cuda.synchronize(env.dev)
            for g in range(G):
                want = mc.gathered(src, part, g, pad)
                got = _np(outs[g])
                assert len(want) == part['groups'][g]['offsets'][-1] <= cap + B * pad
                assert np.array_equal(got[:len(want)], want), (pad, s_shift, g)
                assert np.all(got[len(want):] == sent), (pad, s_shift, g, 'a sample behind offsets_g[B] was written')
            n3 = int(part['count'][3])
            assert n3 == 0 and np.all(_np(outs[3])[:B * pad] == dtype(mc.PAD_VALUE))          # a group of pad slots alone
    # a misaligned group buffer is refused, not served element by element
    rc = env.lib.dsp_gather_groups_batch(d_src.data_ptr(), code, d_san.data_ptr(), B, 1, _ptrs(d_pick[:1]), _ptrs(d_off[:1]), pad,
                                         (ctypes.c_void_p * 1)(outs[0].data_ptr() + 2), None)
    assert rc == nat.EINVAL and b'alignment' in env.lib.dsp_last_error()


# ---- C: the placed finalize kernel with negative columns ------------------------------------------------------------------------

T_LIST = [0, 1, 7, 199, 200, 201, 260]         # tests/test_gpu_mixed_rate.py: empty, shorter than the delta halo, either side of max_len
DST_COL = [3, 1, 7, 5, 2, 6, 4]
SKIPS = ([1, 4], [0], [6, 5, 3], list(range(7)))


def test_c_finalize_skips_negative_columns(env):
    torch, nat, lib = env.torch, env.nat, env.lib
    n = len(T_LIST)
    fo = cc.offsets_of(T_LIST)
    rng = np.random.default_rng(11)
    d_cep, d_fo = _dev(env, rng.standard_normal((int(fo[-1]), C)).astype(np.float32)), _dev(env, fo)
    seg = np.stack([np.zeros(n, dtype=np.int64), 1000 + 100 * np.arange(n, dtype=np.int64)], axis=1)
    nsamp = (seg[:, 1] - seg[:, 0]).astype(np.float64)
    d_seg, d_stats = _dev(env, seg), _dev(env, np.stack([0.25 * nsamp, (2.0 + np.arange(n)) * nsamp], axis=1))

    def placed(cols, source):
        out = torch.full((200, 9, 44), float(SENT), dtype=torch.float32, device=env.dev)
        len0 = torch.full((9,), int(SENT32), dtype=torch.int32, device=env.dev)
        p_seg, p_work = (d_seg.data_ptr(), d_stats.data_ptr()) if source == 'in_place' else (None, None)
        d_col = _dev(env, np.array(cols, dtype=np.int32))
        nat.check(lib.dsp_model_finalize_placed_batch(d_cep.data_ptr(), C, d_fo.data_ptr(), p_seg, p_work, n, C, 3, 200, out.data_ptr(),
                                                      len0.data_ptr(), d_col.data_ptr(), 9, 44, 2, None))
        torch.cuda.synchronize(env.dev)
        return _np(out), _np(len0)
    for source in ('copy', 'in_place'):
        full, full_len = placed(DST_COL, source)
        assert full_len[DST_COL].tolist() == [min(t, 200) for t in T_LIST]
        for skip in SKIPS:
            cols = [-1 - 3 * b if b in skip else c for b, c in enumerate(DST_COL)]           # -1, -4, -7, ...: any negative column
            got, got_len = placed(cols, source)
            want, want_len = full.copy(), full_len.copy()
            for b in skip:
                want[:, DST_COL[b]] = SENT
                want_len[DST_COL[b]] = SENT32
            assert got.tobytes() == want.tobytes(), (source, skip)          # skipped: the sentinel; the others: every bit
            assert np.array_equal(got_len, want_len), (source, skip)


# ---- D: MixedRateCapacityBatch --------------------------------------------------------------------------------------------------

SEVEN_RATES = [44100, 48000, 44100, 48000, 48000, 44100, 44100]


def _seven(extra=0, seed=700):
    """Six clips of 0.9 - 1.4 s interleaved 44.1 / 48 kHz, built as tests/test_gpu_mixed_rate.py's ``six`` builds them, and one
    clip of 0.3 s (30 VAD frames: under the 50 of endpoint.py:44-62).  ``extra`` samples are spread over the six long clips."""
    secs = [0.9, 1.0, 1.1, 1.2, 1.3, 1.4]
    add = [extra // 6 + (extra % 6 if i == 5 else 0) for i in range(6)]
    clips = [make_signal(('vad', seed + i, int(s * r) + 37 * i + 1 + add[i], r, 0.6)) for i, (s, r) in enumerate(zip(secs, SEVEN_RATES))]
    clips.append(make_signal(('vad', seed + 6, int(0.3 * 44100) + 5, 44100, 0.6)))
    return clips


def _load(env, buf, clips, tail=12345):
    flat = np.concatenate(clips)
    host = np.full(buf.numel(), tail, dtype=flat.dtype)
    host[:len(flat)] = flat
    buf.copy_(env.torch.from_numpy(host))
    return flat, cc.offsets_of([len(c) for c in clips])


def _snap(res):
    return tuple(_np(t).tobytes() for t in res)


def test_d_mixed_capacity_batch_replays_any_lengths_and_rates(env, monkeypatch):
    torch, nat = env.torch, env.nat
    from features.model_glue import MixedRateCapacityBatch, MixedRateFeatureBatch, _MixedPlan
    B = 7
    first = _seven()
    cap = sum(len(c) for c in first) + 30001
    order = [3, 0, 6, 2, 5, 1, 4]                        # positions 0, 1, 2, 4, 5 change their rate
    filling = _seven(extra=30001, seed=720)
    vectors = [('first', first, SEVEN_RATES),
               ('permuted', [first[i] for i in order], [SEVEN_RATES[i] for i in order]),
               ('one_rate', _seven(extra=900, seed=740), [48000] * B),          # the 44.1 kHz group: pads alone
               ('filling', filling, SEVEN_RATES[::-1]),
               ('first', first, SEVEN_RATES)]
    assert [a != b for a, b in zip(vectors[0][2], vectors[1][2])].count(True) >= 4
    assert sum(len(c) for c in filling) == cap
    ref = MixedRateFeatureBatch()
    mcb = MixedRateCapacityBatch((44100, 48000))
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    flat, so = _load(env, buf, first)

    def boom(*a, **k):
        raise AssertionError('library scratch was asked for while the graph was being built')
    with monkeypatch.context() as m:                       # no library scratch pointer can be recorded
        m.setattr(nat.SCRATCH, 'get', boom)
        g = mcb.capture(buf, so, SEVEN_RATES, capacity=cap)
    assert g.sample_offsets.dtype == torch.int64 and tuple(g.sample_offsets.shape) == (B + 1,) and g.sample_offsets.is_cuda
    assert g.rates.dtype == torch.int32 and tuple(g.rates.shape) == (B,) and g.jitter is None
    replays, worst, bit_equal = [], 0.0, True
    for k, (tag, clips, rates) in enumerate(vectors):
        flat, so = _load(env, buf, clips, tail=12345 + k)
        assert so[-1] <= cap
        g.sample_offsets.copy_(torch.from_numpy(so))
        g.rates.copy_(torch.from_numpy(np.asarray(rates, dtype=np.int32)))
        inp, len0, ends = g.replay()
        torch.cuda.synchronize(env.dev)
        assert int(g.status.cpu()[0]) == 0, tag
        replays.append(_snap((inp, len0, ends)))
        if k == 4:
            break
        assert len0.dtype == torch.int32 and ends.dtype == torch.int64 and tuple(ends.shape) == (B, 2)
        eager, elen, eends = ref.run(torch.from_numpy(flat).to(env.dev), so, rates)
        assert np.array_equal(_np(len0), elen) and np.array_equal(_np(ends), eends), tag
        got, want = _np(inp), _np(eager)
        assert got.shape == (200, B, 39) and np.isfinite(got).all()
        for b in range(B):
            e = record('mixed_capacity_inp_vs_exact_shape', normwise(got[:, b], want[:, b]))
            worst = max(worst, e)
            assert e <= 5e-5, (tag, b, e)
        bit_equal = bit_equal and got.tobytes() == want.tobytes()
        short = order.index(6) if tag == 'permuted' else B - 1
        assert int(len0[short]) < 50                          # the short clip: under 50 frames, the fallback of endpoint.py:44-62
        # the eager form: the same launch sequence, the same bytes
        r = mcb.run(buf, so, rates, capacity=cap)
        torch.cuda.synchronize(env.dev)
        assert int(r[3].cpu()[0]) == 0 and _snap(r[:3]) == replays[k], tag
    print(f'mixed capacity replays against the exact-shape eager run: worst normwise {worst:.3g}, bit-equal: {bit_equal}')
    assert replays[4] == replays[0]                          # back on the first vector: the first replay's bytes
    # the graph's tables after the last replay: the restatement's, and _MixedPlan's rebased offsets
    arena = g.hold[0]
    part = mc.partition(SEVEN_RATES, so, (44100, 48000), 1, cap)
    plan = _MixedPlan(ref, so, np.asarray(SEVEN_RATES, dtype=np.int64), env.dev, True)
    for gi, grp in enumerate(plan.groups):
        n = len(grp.index)
        assert grp.rate == mcb.rates[gi] and int(_np(arena.count)[gi]) == n
        assert np.array_equal(_np(arena.lays[gi].sample_offsets_in), part['groups'][gi]['offsets'])
        assert np.array_equal(_np(arena.lays[gi].sample_offsets_in)[:n + 1], grp.so)
        assert np.array_equal(_np(arena.dst_col[gi]), part['groups'][gi]['dst_col'])
        assert int(arena.lays[gi].status.cpu()[0]) == 0


def test_d_jitter_and_float_clips(env):
    """The augmented front end (model.py:54-60) and fp32 clips through ``run(capacity=)`` against the exact-shape eager run."""
    torch = env.torch
    from features.model_glue import MixedRateCapacityBatch, MixedRateFeatureBatch
    clips = [c.astype(np.float32) for c in _seven(seed=760)]
    cap = sum(len(c) for c in clips) + 17
    rates = SEVEN_RATES
    jitter = MixedRateFeatureBatch.draw_jitter(rates, random.Random(5))
    buf = torch.zeros(cap, dtype=torch.float32, device=env.dev)
    flat, so = _load(env, buf, clips, tail=-3.5)
    inp, len0, ends, status = MixedRateCapacityBatch().run(buf, so, rates, jitter=jitter, capacity=cap)
    eager, elen, eends = MixedRateFeatureBatch().run(torch.from_numpy(flat).to(env.dev), so, rates, jitter=jitter)
    torch.cuda.synchronize(env.dev)
    assert int(status.cpu()[0]) == 0 and np.array_equal(_np(len0), elen) and np.array_equal(_np(ends), eends)
    for b in range(len(clips)):
        assert record('mixed_capacity_inp_jitter_fp32', normwise(_np(inp)[:, b], _np(eager)[:, b])) <= 5e-5, b


def test_d_two_rates_against_the_reference(env, golden):
    """The two golden clips of the real reference in one mixed capacity call: the project's bar, 1e-4."""
    torch = env.torch
    from features.model_glue import MixedRateCapacityBatch
    clips = [make_signal(case_by_name('model_feat_48k')['sig']), make_signal(case_by_name('model_feat_44k')['sig'])]
    rates, names = [48000, 44100], ['model_feat_48k', 'model_feat_44k']
    cap = sum(len(c) for c in clips) + 1000
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    _, so = _load(env, buf, clips)
    inp, len0, ends, status = MixedRateCapacityBatch().run(buf, so, rates, capacity=cap)
    torch.cuda.synchronize(env.dev)
    got, len0 = _np(inp), _np(len0)
    assert int(status.cpu()[0]) == 0 and got.shape == (200, 2, 39)
    for b, name in enumerate(names):
        n = int(golden[f'{name}/len'][0])
        assert len0[b] == n
        for key, col in (('m0', 0), ('m1', 13), ('m2', 26)):
            err = record(f'mixed_capacity_{name}_{key}', normwise(got[:n, b, col:col + 13], golden[f'{name}/{key}'][:n]))
            assert err <= 1e-4, (name, key, err)
        assert not got[n:, b].any()


# ---- E: MixedRateTrainBatch -----------------------------------------------------------------------------------------------------

LRS = [1e-3, 1e-3, 0.8e-3]
BAR = 2e-5


def _head(kind, dev):
    import torch
    from features import classifier as Cl
    torch.manual_seed(0)
    head = getattr(Cl, kind)().train()
    Cl.fill_parameters(head, 3)
    for m in head.modules():
        if isinstance(m, Cl._DynEnc):
            m.gru.dropout = 0.0
    return head.to(dev)


def _train_content(tb, B, n):
    """n batches, each with its own clips (0.5 - 0.8 s at the clip's own rate), lengths, rate assignments, labels and jitter; and
    the capacity: 1.1 x the longest batch."""
    out = []
    for k in range(n):
        rng = np.random.default_rng(100 * B + k)
        rates = mc.rate_vector(B, (44100, 48000), 7 * B + k)
        clips = [make_signal(('vad', 900 + 40 * k + i, int(rng.uniform(0.5, 0.8) * r) + i, int(r), 0.6)) for i, r in enumerate(rates)]
        labels = rng.integers(0, 20, B).astype(np.int64)
        out.append((clips, rates, labels, tb.draw_jitter(rates, random.Random(B + k))))
    cap = (11 * max(sum(len(c) for c in b[0]) for b in out)) // 10
    return cap, out


def _bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _err(got, ref):
    ref = _np(ref).astype(np.float64)
    return float(np.max(np.abs(_np(got).astype(np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


@pytest.mark.parametrize('kind,B', [('HMRNNHead', 5), ('TransformerHead', 32)])
def test_e_three_replays_equal_three_eager_steps(env, kind, B):
    torch, dev = env.torch, env.dev
    from features.model_glue import MixedRateFeatureBatch
    from features.optim import DeviceAdam
    from features.train import CAPTURE_VERIFIED, MixedRateTrainBatch
    assert B in CAPTURE_VERIFIED[kind]
    head = _head(kind, dev)
    twin, parent = copy.deepcopy(head), copy.deepcopy(head)         # the same start for the eager steps and for the parent's step
    kw = {'dropout': False}
    tb, tb_twin = MixedRateTrainBatch((44100, 48000), head), MixedRateTrainBatch((44100, 48000), twin)
    cap, content = _train_content(tb, B, 3)
    assert len({tuple(c[1].tolist()) for c in content}) == 3        # three rate assignments
    params = list(head.parameters())
    opt = DeviceAdam(params, lr=LRS[0])
    buf = torch.zeros(cap, dtype=torch.int16, device=dev)
    _, so0 = _load(env, buf, content[0][0])
    lab, jit = torch.from_numpy(content[0][2]).to(dev), torch.from_numpy(content[0][3]).to(dev)
    start = [p.detach().clone() for p in params]
    g = tb.capture(buf, so0, content[0][1], lab, jit, optimizer=opt, capacity=cap, **kw)
    torch.cuda.synchronize(dev)
    assert all(_bits(p, q) for p, q in zip(params, start)) and opt.device_state() == (0, LRS[0], 0.9, 0.999, 1e-8)
    losses, eager_in = [], []
    for k, (clips, rates, l, j) in enumerate(content):
        flat, so = _load(env, buf, clips, tail=77 + k)
        eager_in.append((flat, so))
        g.sample_offsets.copy_(torch.from_numpy(so))
        g.rates.copy_(torch.from_numpy(rates))
        lab.copy_(torch.from_numpy(l))
        g.jitter.copy_(torch.from_numpy(j))
        if LRS[k] != opt.lr:
            opt.set_lr(LRS[k])
        res = g.replay()
        losses.append(res.loss.clone())
    torch.cuda.synchronize(dev)
    assert int(res.n_clamped.cpu()[0]) == 0 and int(g.status.cpu()[0]) == 0
    opt_twin = DeviceAdam(list(twin.parameters()), lr=LRS[0])
    want, first = [], None
    for k, (clips, rates, l, j) in enumerate(content):
        if LRS[k] != opt_twin.lr:
            opt_twin.set_lr(LRS[k])
        _load(env, buf, clips, tail=77 + k)
        for p in opt_twin.params:
            p.grad = None
        out = tb_twin.run(buf, eager_in[k][1], rates, torch.from_numpy(l).to(dev), torch.from_numpy(j).to(dev), capacity=cap, **kw)
        out.loss.backward()
        if k == 0:
            first = (out.logits.detach().clone(), out.loss.detach().clone(), [p.grad.clone() for p in opt_twin.params])
        opt_twin.step()
        want.append(out.loss.detach().clone())
        torch.cuda.synchronize(dev)
        assert int(out.status.cpu()[0]) == 0
    differing = [k for k in range(3) if not _bits(losses[k], want[k])]
    print(f'{kind} B={B} capacity {cap}: losses {[float(x) for x in losses]}, differing from the eager steps in bits: {differing}')
    assert not differing
    names = [n for n, _ in head.named_parameters()]
    bad = [n for n, p, q in zip(names, head.parameters(), twin.parameters()) if not _bits(p, q)]
    bad += [n + '.exp_avg' for n, p, q in zip(names, opt.exp_avg, opt_twin.exp_avg) if not _bits(p, q)]
    bad += [n + '.exp_avg_sq' for n, p, q in zip(names, opt.exp_avg_sq, opt_twin.exp_avg_sq) if not _bits(p, q)]
    assert not bad, bad
    assert opt.device_state() == opt_twin.device_state() == (3, LRS[2], 0.9, 0.999, 1e-8)
    assert not any(_bits(p, q) for p, q in zip(params, start))     # ... and every parameter moved

    # the first step against parent code: the eager exact-shape mixed-rate front end, the head, cross-entropy, backward
    clips, rates, l, j = content[0]
    flat, so = eager_in[0]
    inp, len0, _ = MixedRateFeatureBatch().run(torch.from_numpy(flat).to(dev), so, rates, jitter=j)
    out = parent(inp, torch.from_numpy(np.asarray(len0, dtype=np.int32)).to(dev), device_len=True, device_grad=True, **kw)
    logits = out[0] if isinstance(out, (tuple, list)) else out
    torch.nn.functional.cross_entropy(logits, torch.from_numpy(l).to(dev)).backward()
    torch.cuda.synchronize(dev)
    e_logits = record(f'mixed_capacity_train_{kind}_logits_vs_parent', _err(first[0], logits))
    worst, worst_name = 0.0, ''
    for name, a, p in zip(names, first[2], parent.parameters()):
        e = normwise(_np(a), _np(p.grad))
        if e > worst:
            worst, worst_name = e, name
    record(f'mixed_capacity_train_{kind}_grads_vs_parent', worst)
    print(f'{kind} B={B}: first step against the parent route: logits {e_logits:.3g}, worst gradient {worst:.3g} normwise ({worst_name})')
    assert e_logits <= BAR
    assert worst <= BAR, (worst_name, worst)


# ---- F: refusals ----------------------------------------------------------------------------------------------------------------

def test_f_refusals(env):
    torch, dev = env.torch, env.dev
    from features.model_glue import MixedRateCapacityBatch
    from features.train import CAPTURE_VERIFIED, MixedRateTrainBatch
    clips = _seven()[:3]
    so = cc.offsets_of([len(c) for c in clips])
    cap = int(so[-1]) + 100
    buf = torch.zeros(cap, dtype=torch.int16, device=dev)
    wrong = torch.zeros(cap - 1, dtype=torch.int16, device=dev)
    rates = SEVEN_RATES[:3]
    lab = torch.zeros(3, dtype=torch.int64, device=dev)
    mcb = MixedRateCapacityBatch()
    tb = MixedRateTrainBatch((44100, 48000), _head('HMRNNHead', dev))
    assert all(3 not in sizes for sizes in CAPTURE_VERIFIED.values())
    with pytest.raises(NotImplementedError, match='CAPTURE_VERIFIED'):
        tb.capture(buf, so, rates, lab, None, capacity=cap, dropout=False)
    so5 = cc.offsets_of([len(c) for c in _seven()[:5]])
    lab5 = torch.zeros(5, dtype=torch.int64, device=dev)
    for call in (lambda: mcb.run(wrong, so, rates, capacity=cap), lambda: mcb.capture(wrong, so, rates, capacity=cap),
                 lambda: mcb.capture(buf.unsqueeze(0), so, rates, capacity=cap),
                 lambda: tb.run(wrong, so, rates, lab, capacity=cap, dropout=False),
                 lambda: tb.capture(wrong, so5, SEVEN_RATES[:5], lab5, None, capacity=cap, dropout=False)):
        with pytest.raises(ValueError, match='exactly that many samples'):
            call()
    with pytest.raises(TypeError, match='device tensor'):
        mcb.run(np.zeros(cap, dtype=np.int16), so, rates, capacity=cap)
    for call in (lambda: mcb.run(buf, so, rates), lambda: mcb.capture(buf, so, rates), lambda: tb.run(buf, so, rates, lab, dropout=False)):
        with pytest.raises(ValueError, match='capacity routes only'):
            call()
    with pytest.raises(ValueError, match='rates must be'):
        mcb.run(buf, so, rates[:2], capacity=cap)
    for table in ((44100, 48000, 16000, 8000, 22050), (44100, 44100), (48000, 0)):
        with pytest.raises(ValueError):
            MixedRateCapacityBatch(table)
        with pytest.raises(ValueError):
            MixedRateTrainBatch(table, _head('HMRNNHead', dev))
