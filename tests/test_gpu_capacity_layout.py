"""Graph replays for clips of any length (features/pipeline.py: ``CapacityLayout``; include/dsp_frontend.h:
dsp_batch_offsets_batch, dsp_layout_create_capacity, dsp_layout_refresh).

  A  the offsets kernel alone: integers against dsp_frame_offsets on the host and the restatement of tests/capacity_cases.py;
  B  the VAD kernels on a capacity handle against the exact handle: ``==`` on the true frames, canaries behind them;
  C  ``ModelFeatureBatch.capture(..., capacity=)``: three replays on three length vectors against the eager exact-layout run;
  D  ``EnsembleBatch.capture(..., capacity=)``: the same with the assertions of tests/test_gpu_ensemble_graph.py, and a fourth
     replay back on the first vector (stale tables would show);
  E  ``TrainBatch.capture(..., capacity=)`` with and without ``DeviceAdam``, with the assertions of tests/test_gpu_train_optim.py
     and tests/test_gpu_train_capture.py;
  F  the refusals.

Clips are ``ensemble_cases.make_clips()`` cut to prefixes; the whole-chain tests feed valid offsets only."""
import copy
import ctypes
import random

import numpy as np
import pytest

import capacity_cases as cc
from conftest import normwise, record
from ensemble_cases import PAIRS, THRESHOLDS, make_clips

pytestmark = pytest.mark.gpu

BAR = 2e-5                      # tests/test_gpu_ensemble_graph.py: logits of a replay against the eager run
PAD = 4096
SENT32 = np.int32(0x7fc0beef)   # a quiet-NaN pattern: never a result (tests/test_gpu_canaries.py)


def _np(t):
    return t.detach().cpu().numpy()


def _dev():
    import torch
    from features import _native as nat
    nat.require_device()
    return torch.device('cuda', 0)


# ---- length vectors: prefixes of the stored clips -------------------------------------------------------------------------------

def _cut(stored, B, k):
    """Batch k of B clips: stored clips in an order and at prefix lengths that change with k (batch 0 is the shortest: the
    capacity is 1.25 x its total)."""
    out = []
    for i in range(B):
        c = stored[(i + 3 * k) % len(stored)]
        frac = (0.60 + 0.05 * ((3 * i) % 5)) if k == 0 else (0.60 + 0.10 * ((7 * i + 3 * k) % 5))
        out.append(c[:int(frac * len(c)) + 7 * i + k])
    return out


def _fit(clips, cap, exact=False):
    """Cut the longest clips until the batch fits ``cap`` samples; ``exact``: lengthening is not possible, so the caller has
    chosen clips that overshoot, and the batch comes back summing to exactly ``cap``."""
    clips = list(clips)
    excess = sum(len(c) for c in clips) - cap
    while excess > 0:
        j = int(np.argmax([len(c) for c in clips]))
        take = min(excess, len(clips[j]) - 6000)
        assert take > 0, 'the clips cannot be cut to the capacity'
        clips[j] = clips[j][:len(clips[j]) - take]
        excess -= take
    assert not exact or sum(len(c) for c in clips) == cap, 'the chosen clips do not reach the capacity'
    return clips


def _variant(flat, k):
    x = flat.astype(np.int32)
    return [x, -x // 2, (3 * x) // 4, -(x // 3)][k % 4].astype(np.int16)


def _fill(buf, clips, k=0, tail=12345):
    """Write the batch into the capacity buffer; the samples behind it are set to ``tail`` (they must be ignored)."""
    import torch
    flat = _variant(np.concatenate(clips), k)
    host = np.full(buf.numel(), tail, dtype=np.int16)
    host[:len(flat)] = flat
    buf.copy_(torch.from_numpy(host))
    return flat, cc.offsets_of([len(c) for c in clips])


# ---- A: the offsets kernel alone ------------------------------------------------------------------------------------------------

FRAMINGS_A = [(480, 160), (64, 200)]          # the 16 kHz VAD framing; a hop longer than the frame


def _offsets_kernel(nat, torch, dev, table, n_utt, cap):
    d_in = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)).to(dev)
    d_out = torch.full((n_utt + 1,), -7, dtype=torch.int64, device=dev)
    d_fo = [torch.full((n_utt + 1,), -7, dtype=torch.int64, device=dev) for _ in FRAMINGS_A]
    d_st = torch.full((1,), -7, dtype=torch.int32, device=dev)
    Ls = (ctypes.c_int32 * 2)(*[f[0] for f in FRAMINGS_A])
    Ss = (ctypes.c_int32 * 2)(*[f[1] for f in FRAMINGS_A])
    tabs = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in d_fo])
    st = torch.cuda.current_stream(dev).cuda_stream
    nat.check(nat.load().dsp_batch_offsets_batch(d_in.data_ptr(), n_utt, cap, 2, Ls, Ss, d_out.data_ptr(), tabs, d_st.data_ptr(), st))
    torch.cuda.synchronize(dev)
    return _np(d_out), [_np(t) for t in d_fo], int(_np(d_st)[0])


@pytest.mark.parametrize('n_utt', [1, 5, 64, 1500])
def test_a_offsets_kernel(n_utt):
    import torch
    from features import _native as nat
    dev = _dev()
    rng = np.random.default_rng(n_utt)
    lens = rng.integers(3, 2000, n_utt)
    lens[:min(n_utt, 4)] = [3, 480, 481, 64][:min(n_utt, 4)]
    so = cc.offsets_of(lens)
    for cap in (int(so[-1]), int(so[-1]) + 1, 2 * int(so[-1])):
        out, fos, status = _offsets_kernel(nat, torch, dev, so, n_utt, cap)
        assert status == 0 and np.array_equal(out, so), cap
        for (L, S), fo in zip(FRAMINGS_A, fos):
            assert np.array_equal(fo, nat.frame_offsets(so, L, S)) and np.array_equal(fo, cc.frame_offsets(so, L, S)), (cap, L, S)
            assert fo[-1] <= nat.frames_bound(cap, n_utt, L, S)
    cap = int(so[-1]) + 2
    for bit, table in cc.invalid_tables(so, cap).items():
        out, fos, status = _offsets_kernel(nat, torch, dev, table, n_utt, cap)
        want = cc.sanitise(table, cap)
        assert status == bit, (bit, status)
        assert np.array_equal(out, want), bit
        assert out[0] == 0 and np.all(np.diff(out) >= 0) and out[-1] <= cap
        for (L, S), fo in zip(FRAMINGS_A, fos):
            assert np.array_equal(fo, nat.frame_offsets(want, L, S)), (bit, L, S)
    # a table with everything wrong at once: every bit, and still a table no kernel can leave the buffer with
    wild = rng.integers(-50, 3 * cap, n_utt + 1)
    wild[0] = 9
    if n_utt >= 3:
        wild[2] = wild[1]
        wild[3] = wild[2] - 1
    out, fos, status = _offsets_kernel(nat, torch, dev, wild, n_utt, cap)
    assert status == cc.status(wild, cap) and np.array_equal(out, cc.sanitise(wild, cap))
    for (L, S), fo in zip(FRAMINGS_A, fos):
        assert np.array_equal(fo, nat.frame_offsets(out, L, S))


# ---- B: the VAD kernels on a capacity handle ------------------------------------------------------------------------------------

def _guarded(n_words, dev):
    """An int32 tensor of PAD + n_words * 4 + PAD bytes, all sentinel; (tensor, payload pointer, host copy of everything)."""
    import torch
    buf = torch.full((2 * PAD // 4 + n_words,), int(SENT32), dtype=torch.int32, device=dev)

    def read():
        torch.cuda.synchronize(dev)
        return buf.cpu().numpy()
    return buf, buf.data_ptr() + PAD, read


VAD_CELLS = [(480, 160, 16, 16), (1323, 441, 8, 4), (661, 661, 4, 4), (48, 16, 1, 1)]     # (L, S, frames per wave: int16 |x|, every other)


@pytest.mark.parametrize('use_sq', [0, 1])
@pytest.mark.parametrize('dtype', ['int16', 'float32'])
@pytest.mark.parametrize('L,S,fr_scan,fr_other', VAD_CELLS)
def test_b_vad_on_a_capacity_handle_equals_the_exact_handle(L, S, fr_scan, fr_other, dtype, use_sq):
    import torch
    from features import _native as nat
    dev = _dev()
    lib = nat.load()
    wd = nat.WAVE_I16 if dtype == 'int16' else nat.WAVE_F32
    fr = ctypes.c_int32(0)
    family = lib.dsp_debug_vad_route(L, S, wd, use_sq, ctypes.byref(fr))
    assert fr.value == (fr_scan if dtype == 'int16' and not use_sq else fr_other)
    assert (family == nat.VAD_PER_FRAME) == (fr.value == 1)
    stored, _ = make_clips()
    lens = [1, L, L + 1, 5 * S + L + 3, 7001]                     # one sample, exactly a frame, one more, and two longer clips
    clips = [stored[i][:n] for i, n in enumerate(lens)]
    flat = np.concatenate(clips)
    flat = flat if dtype == 'int16' else (flat.astype(np.float32) / 3.0)
    so = cc.offsets_of(lens)
    fo = nat.frame_offsets(so, L, S)
    n_true, total, B = int(fo[-1]), int(so[-1]), len(lens)
    st = torch.cuda.current_stream(dev).cuda_stream
    d_so, d_fo = torch.from_numpy(so).to(dev), torch.from_numpy(fo).to(dev)
    # the exact handle
    wave = torch.from_numpy(flat).to(dev)
    h = ctypes.c_void_p(0)
    nat.check(lib.dsp_layout_create(d_fo.data_ptr(), B, n_true, L, S, st, ctypes.byref(h)))
    amp0 = torch.zeros(n_true, dtype=torch.float64, device=dev)
    zcr0 = torch.zeros(n_true, dtype=torch.int32, device=dev)
    nat.check(lib.dsp_vad_features_layout_batch(h, wave.data_ptr(), wd, d_so.data_ptr(), d_fo.data_ptr(), use_sq, amp0.data_ptr(),
                                                zcr0.data_ptr(), st))
    torch.cuda.synchronize(dev)
    nat.check(lib.dsp_layout_destroy(h))
    amp0, zcr0 = _np(amp0), _np(zcr0)
    for cap in (total, total + 1, 2 * total):
        bound = nat.frames_bound(cap, B, L, S)
        assert bound >= n_true
        wbuf = torch.full((cap,), 9999, dtype=wave.dtype, device=dev)          # what lies behind the clips must not matter
        wbuf[:total] = wave
        d_in = torch.from_numpy(so).to(dev)
        d_san = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        d_fr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        Ls, Ss, tabs = (ctypes.c_int32 * 1)(L), (ctypes.c_int32 * 1)(S), (ctypes.c_void_p * 1)(d_fr.data_ptr())
        hc = ctypes.c_void_p(0)
        nat.check(lib.dsp_layout_create_capacity(B, bound, L, S, ctypes.byref(hc)))
        abuf, aptr, aread = _guarded(2 * bound, dev)
        zbuf, zptr, zread = _guarded(bound, dev)
        nat.check(lib.dsp_batch_offsets_batch(d_in.data_ptr(), B, cap, 1, Ls, Ss, d_san.data_ptr(), tabs, d_st.data_ptr(), st))
        nat.check(lib.dsp_layout_refresh(hc, d_fr.data_ptr(), st))
        nat.check(lib.dsp_vad_features_layout_batch(hc, wbuf.data_ptr(), wd, d_san.data_ptr(), d_fr.data_ptr(), use_sq, aptr, zptr, st))
        a, z = aread(), zread()
        nat.check(lib.dsp_layout_destroy(hc))
        assert int(_np(d_st)[0]) == 0 and np.array_equal(_np(d_fr), fo)
        lo = PAD // 4
        amp = a[lo:lo + 2 * n_true].view(np.float64)
        assert np.all(amp == amp0) and np.all(z[lo:lo + n_true] == zcr0), (cap, 'true frames')
        assert np.all(a[:lo] == SENT32) and np.all(a[lo + 2 * n_true:] == SENT32), (cap, 'amp_sum written outside the true frames')
        assert np.all(z[:lo] == SENT32) and np.all(z[lo + n_true:] == SENT32), (cap, 'zcr written outside the true frames')


def test_b_capacity_handle_refuses_what_needs_the_pool():
    """A wave buffer that does not start on a vector would need the shifted view in a pooled workspace: DSP_EINVAL, no reroute;
    and only a capacity handle can be refreshed."""
    import torch
    from features import _native as nat
    dev = _dev()
    lib = nat.load()
    L, S, B = 480, 160, 2
    so = cc.offsets_of([700, 900])
    fo = nat.frame_offsets(so, L, S)
    d_so, d_fo = torch.from_numpy(so).to(dev), torch.from_numpy(fo).to(dev)
    wave = torch.zeros(1608, dtype=torch.int16, device=dev)
    amp = torch.zeros(64, dtype=torch.float64, device=dev)
    zcr = torch.zeros(64, dtype=torch.int32, device=dev)
    hc, h = ctypes.c_void_p(0), ctypes.c_void_p(0)
    nat.check(lib.dsp_layout_create_capacity(B, nat.frames_bound(1600, B, L, S), L, S, ctypes.byref(hc)))
    nat.check(lib.dsp_layout_refresh(hc, d_fo.data_ptr(), None))
    rc = lib.dsp_vad_features_layout_batch(hc, wave.data_ptr() + 2, nat.WAVE_I16, d_so.data_ptr(), d_fo.data_ptr(), 0, amp.data_ptr(),
                                           zcr.data_ptr(), None)
    assert rc == nat.EINVAL and b'capacity layout' in lib.dsp_last_error()
    nat.check(lib.dsp_layout_create(d_fo.data_ptr(), B, int(fo[-1]), L, S, None, ctypes.byref(h)))
    assert lib.dsp_layout_refresh(h, d_fo.data_ptr(), None) == nat.EINVAL and b'dsp_layout_create_capacity' in lib.dsp_last_error()
    torch.cuda.synchronize(dev)
    nat.check(lib.dsp_layout_destroy(h))
    nat.check(lib.dsp_layout_destroy(hc))


# ---- C: ModelFeatureBatch -------------------------------------------------------------------------------------------------------

def test_c_model_feature_batch_replays_any_lengths():
    import torch
    from features.model_glue import ModelFeatureBatch
    dev = _dev()
    stored, rate = make_clips()
    B = 5
    first = _cut(stored, B, 0)
    cap = (5 * sum(len(c) for c in first)) // 4
    permuted = [first[i] for i in (3, 0, 4, 2, 1)]
    longest = sorted(stored, key=len)[-B:]
    full = _fit(longest, cap, exact=True)                                   # sums exactly to the capacity
    short = _fit([stored[6][:5000], stored[7], stored[8][:9001], stored[9], stored[10][:8500]], cap)
    n_short = 1 + -(-(5000 - int(rate * 0.03)) // int(rate * 0.01))
    assert n_short < 50                                                     # the reference's fallback, endpoint.py:42-62
    mfb, ref = ModelFeatureBatch(rate=rate), ModelFeatureBatch(rate=rate)
    buf = torch.zeros(cap, dtype=torch.int16, device=dev)
    flat, so = _fill(buf, first)
    g = mfb.capture(buf, so, capacity=cap)
    assert tuple(g.sample_offsets.shape) == (B + 1,) and g.sample_offsets.dtype == torch.int64 and g.sample_offsets.is_cuda
    for k, (tag, clips) in enumerate((('first', first), ('permuted', permuted), ('full', full), ('short', short))):
        flat, so = _fill(buf, clips, k)
        assert so[-1] <= cap and (tag != 'full' or so[-1] == cap)
        g.sample_offsets.copy_(torch.from_numpy(so))
        inp, len0, ends = g.replay()
        torch.cuda.synchronize(dev)
        assert int(g.status.cpu()[0]) == 0
        snap = (inp.clone(), len0.clone(), ends.clone())
        eager, elen, eends = ref.run(torch.from_numpy(flat).to(dev), so)
        assert np.array_equal(_np(len0), elen) and np.array_equal(_np(ends), eends), tag
        e = record(f'capacity_mfb_inp_{tag}', max(normwise(_np(inp)[:, b], _np(eager)[:, b]) for b in range(B)))
        print(f'{tag}: lengths {np.diff(so).tolist()}, inp normwise {e:.3g} against the exact-layout run')
        assert torch.equal(inp, eager), tag
        r_inp, r_len, r_ends = mfb.run(buf, so, capacity=cap)
        torch.cuda.synchronize(dev)
        assert int(mfb.capacity_status.cpu()[0]) == 0
        assert _np(r_inp).tobytes() == _np(snap[0]).tobytes() and torch.equal(r_len, snap[1]) and torch.equal(r_ends, snap[2]), tag


# ---- D: EnsembleBatch -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def env():
    """The fixture rules of tests/test_gpu_ensemble_graph.py's ``env``, with all stored clips."""
    import os
    import types
    import torch
    from conftest import ROOT
    from features import _native as nat
    from features import ensemble
    from features.classifier import HMRNNHead, fill_parameters
    dev = _dev()
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ensemble_golden.npz')) as z:
        models = [{k: z[f'svm{p[0]}{p[1]}/{k}'] for k in ('scale', 'support_vectors', 'dual_coef', 'intercept', 'gamma', 'classes')}
                  for p in PAIRS]
    rules = [(p, t, ensemble.PitchSVM.from_arrays(m['support_vectors'], m['dual_coef'], m['intercept'], m['gamma'], m['classes'],
                                                  scale=m['scale']))
             for p, t, m in zip(PAIRS, THRESHOLDS, models)]
    rng = np.random.default_rng(7)
    for pair in ((2, 3), (12, 13)):
        rules.append((pair, 0.9, ensemble.PitchSVM.from_arrays(rng.standard_normal((40, 5)), rng.uniform(-1, 1, 40), rng.uniform(-0.2, 0.2),
                                                               0.1, pair, scale=rng.uniform(0.5, 2.0, 5), center=rng.standard_normal(5))))
    head = HMRNNHead().to(dev).eval()
    fill_parameters(head, 3)
    clips, rate = make_clips()
    return types.SimpleNamespace(nat=nat, ens=ensemble, torch=torch, dev=dev, rules=rules, head=head, clips=clips, rate=rate)


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


def _compare(tag, got, want, n):
    """tests/test_gpu_ensemble_graph.py's ``_compare``: ``got`` a replayed (or sync-free) namespace, ``want`` the eager run()'s."""
    assert str(got.len0.dtype) == 'torch.int32' and got.len0.is_cuda
    assert str(got.endpoints.dtype) == 'torch.int64' and tuple(got.endpoints.shape) == (n, 2) and got.endpoints.is_cuda
    for name in ('pred', 'used', 'valid'):
        assert np.array_equal(_np(getattr(got, name)), _np(getattr(want, name))), (tag, name)
    assert np.array_equal(_np(got.len0), np.asarray(want.len0)) and np.array_equal(_np(got.endpoints), np.asarray(want.endpoints)), tag
    assert _np(got.feat).tobytes() == _np(want.feat).tobytes(), (tag, 'feat')
    assert _np(got.decision).tobytes() == _np(want.decision).tobytes(), (tag, 'decision')
    e = record(f'capacity_ensemble_logits_{tag}', _err(_np(got.logits), _np(want.logits)))
    print(f'{tag}: logits err {e:.3g}')
    assert e <= BAR
    assert int(_np(got.n_clamped)[0]) == 0
    print(f'{tag}: rules fired on {int((_np(want.used) != 0).sum())} of {n} clips')


def _snapshot(ns):
    return {k: _np(getattr(ns, k)).tobytes() for k in ('pred', 'used', 'valid', 'len0', 'endpoints', 'feat', 'decision', 'logits', 'prob')}


def test_d_ensemble_batch_replays_any_lengths(env, monkeypatch):
    torch, nat = env.torch, env.nat
    B = len(env.clips)
    assert B == 14
    batches = [_cut(env.clips, B, k) for k in range(3)]
    cap = (5 * sum(len(c) for c in batches[0])) // 4
    batches = [_fit(b, cap) for b in batches]
    buf = torch.zeros(cap, dtype=torch.int16, device=env.dev)
    flat, so = _fill(buf, batches[0])
    eb = env.ens.EnsembleBatch(env.rate, env.head, env.rules)

    def boom(*a, **k):
        raise AssertionError('library scratch was asked for while the graph was being built')
    with monkeypatch.context() as m:                       # no library scratch pointer can be recorded
        m.setattr(nat.SCRATCH, 'get', boom)
        g = eb.capture(buf, so, capacity=cap, dropout=False)
    with torch.no_grad():
        first = None
        for k, clips in enumerate(batches + [batches[0]]):
            flat, so = _fill(buf, clips, k % 3)
            g.sample_offsets.copy_(torch.from_numpy(so))
            out = g.replay()
            torch.cuda.synchronize(env.dev)
            assert int(g.status.cpu()[0]) == 0
            if k < 3:
                _compare(f'lengths_{k}', out, eb.run(flat, so, dropout=False), B)
            if k == 0:
                first = _snapshot(out)
            if k == 3:                                     # back on the first vector: the first replay's bytes
                again = _snapshot(out)
                for name in ('pred', 'used', 'valid', 'len0', 'endpoints', 'feat', 'decision'):
                    assert again[name] == first[name], name
                assert _err(np.frombuffer(again['logits'], np.float32), np.frombuffer(first['logits'], np.float32)) <= BAR
        # the eager form on the capacity layout gives the same namespace
        flat, so = _fill(buf, batches[1], 1)
        free = eb.run(buf, so, capacity=cap, dropout=False)
        torch.cuda.synchronize(env.dev)
        assert int(free.status.cpu()[0]) == 0
        _compare('run_capacity', free, eb.run(flat, so, dropout=False), B)


# ---- E: TrainBatch --------------------------------------------------------------------------------------------------------------

LRS = [1e-3, 1e-3, 0.8e-3]


def _head(kind, dev):
    import torch
    from features import classifier as C
    torch.manual_seed(0)
    head = getattr(C, kind)().train()
    C.fill_parameters(head, 3)
    for m in head.modules():
        if isinstance(m, C._DynEnc):
            m.gru.dropout = 0.0
    return head.to(dev)


def _train_content(tb, B, stored, n):
    """n batches, each with its own clips, lengths, labels and jitter; and the capacity: 1.25 x the first batch's total."""
    batches = [_cut(stored, B, k) for k in range(n)]
    cap = (5 * sum(len(c) for c in batches[0])) // 4
    labels = np.random.default_rng(B).integers(0, 20, B).astype(np.int64)
    return cap, [(_fit(b, cap), (labels + 7 * k) % 20, tb.draw_jitter(B, random.Random(B + k))) for k, b in enumerate(batches)]


def _bits(a, b):
    import torch
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _assert_same_state(head_a, opt_a, head_b, opt_b, step, lr):
    names = [n for n, _ in head_a.named_parameters()]
    bad = [n for n, p, q in zip(names, head_a.parameters(), head_b.parameters()) if not _bits(p, q)]
    bad += [n + '.exp_avg' for n, p, q in zip(names, opt_a.exp_avg, opt_b.exp_avg) if not _bits(p, q)]
    bad += [n + '.exp_avg_sq' for n, p, q in zip(names, opt_a.exp_avg_sq, opt_b.exp_avg_sq) if not _bits(p, q)]
    assert not bad, bad
    assert opt_a.device_state() == opt_b.device_state() == (step, lr, 0.9, 0.999, 1e-8)


@pytest.mark.parametrize('kind,B', [('HMRNNHead', 5), ('TransformerHead', 32)])
def test_e_three_replays_equal_three_eager_steps(kind, B):
    import torch
    from features.optim import DeviceAdam
    from features.train import CAPTURE_VERIFIED, TrainBatch
    assert B in CAPTURE_VERIFIED[kind]
    dev = _dev()
    stored, rate = make_clips()
    head = _head(kind, dev)
    twin = copy.deepcopy(head)                                     # the same start for the eager steps
    kw = {'dropout': False}
    tb, tb_twin = TrainBatch(rate, head), TrainBatch(rate, twin)
    cap, content = _train_content(tb, B, stored, 3)
    params = list(head.parameters())
    opt = DeviceAdam(params, lr=LRS[0])
    buf = torch.zeros(cap, dtype=torch.int16, device=dev)
    _, so0 = _fill(buf, content[0][0])
    lab, jit = (torch.from_numpy(a).to(dev) for a in content[0][1:])
    start = [p.detach().clone() for p in params]
    g = tb.capture(buf, so0, lab, jit, optimizer=opt, capacity=cap, **kw)
    torch.cuda.synchronize(dev)
    assert all(_bits(p, q) for p, q in zip(params, start)) and opt.device_state() == (0, LRS[0], 0.9, 0.999, 1e-8)
    losses, eager_in = [], []
    for k, (clips, l, j) in enumerate(content):
        flat, so = _fill(buf, clips, k)
        eager_in.append((flat, so))
        assert len(set(np.diff(so).tolist()) ^ set(np.diff(so0).tolist())) > 0 or k == 0      # new lengths
        g.sample_offsets.copy_(torch.from_numpy(so))
        lab.copy_(torch.from_numpy(l))
        jit.copy_(torch.from_numpy(j))
        if LRS[k] != opt.lr:
            opt.set_lr(LRS[k])
        res = g.replay()
        losses.append(res.loss.clone())
    torch.cuda.synchronize(dev)
    assert int(res.n_clamped.cpu()[0]) == 0 and int(g.status.cpu()[0]) == 0
    opt_twin = DeviceAdam(list(twin.parameters()), lr=LRS[0])
    want = []
    for k, (clips, l, j) in enumerate(content):
        if LRS[k] != opt_twin.lr:
            opt_twin.set_lr(LRS[k])
        flat, so = eager_in[k]
        for p in opt_twin.params:
            p.grad = None
        out = tb_twin.run(torch.from_numpy(flat).to(dev), so, torch.from_numpy(l).to(dev), torch.from_numpy(j).to(dev), **kw)
        out.loss.backward()
        opt_twin.step()
        want.append(out.loss.detach().clone())
    torch.cuda.synchronize(dev)
    differing = [k for k in range(3) if not _bits(losses[k], want[k])]
    print(f'{kind} B={B} capacity {cap}: losses {[float(x) for x in losses]}, differing from the eager steps in bits: {differing}')
    assert not differing
    _assert_same_state(head, opt, twin, opt_twin, 3, LRS[2])
    assert not any(_bits(p, q) for p, q in zip(params, start))     # ... and every parameter moved


@pytest.mark.parametrize('kind,B', [('HMRNNHead', 5), ('TransformerHead', 32)])
def test_e_second_replay_without_optimizer_equals_the_eager_step(kind, B):
    import torch
    from features.train import TrainBatch
    dev = _dev()
    stored, rate = make_clips()
    head = _head(kind, dev)
    kw = {'dropout': False}
    tb = TrainBatch(rate, head)
    cap, content = _train_content(tb, B, stored, 2)
    buf = torch.zeros(cap, dtype=torch.int16, device=dev)
    _, so = _fill(buf, content[0][0])
    lab, jit = (torch.from_numpy(a).to(dev) for a in content[0][1:])
    params = list(head.parameters())
    g = tb.capture(buf, so, lab, jit, capacity=cap, **kw)
    g.replay()
    torch.optim.Adam(params, lr=1e-3).step()
    flat, so = _fill(buf, content[1][0], 1)
    g.sample_offsets.copy_(torch.from_numpy(so))
    lab.copy_(torch.from_numpy(content[1][1]))
    jit.copy_(torch.from_numpy(content[1][2]))
    res = g.replay()
    torch.cuda.synchronize(dev)
    second, loss2 = [None if gr is None else gr.clone() for gr in g.grads], res.loss.clone()
    assert int(res.n_clamped.cpu()[0]) == 0 and int(g.status.cpu()[0]) == 0 and all(gr is not None for gr in second)
    for p in params:
        p.grad = None
    eager = tb.run(torch.from_numpy(flat).to(dev), so, lab, jit, **kw)
    eager.loss.backward()
    torch.cuda.synchronize(dev)
    bad = [n for (n, p), a in zip(head.named_parameters(), second) if not torch.equal(a.view(torch.int32), p.grad.view(torch.int32))]
    worst = max(float((a - p.grad).abs().max()) / max(1.0, float(p.grad.abs().max())) for a, p in zip(second, params))
    print(f'{kind} B={B}: second replay against eager: worst {worst:.3g}, differing in bits: {bad}')
    assert torch.equal(loss2.view(torch.int32), eager.loss.detach().view(torch.int32))
    assert not bad
    # the eager form on the capacity layout: the same loss
    for p in params:
        p.grad = None
    again = tb.run(buf, so, lab, jit, capacity=cap, **kw)
    torch.cuda.synchronize(dev)
    assert int(again.status.cpu()[0]) == 0 and torch.equal(again.loss.detach().view(torch.int32), loss2.view(torch.int32))


# ---- F: refusals ----------------------------------------------------------------------------------------------------------------

def test_f_refusals(env):
    import torch
    from features.model_glue import MixedRateFeatureBatch, ModelFeatureBatch
    from features.train import CAPTURE_VERIFIED, TrainBatch
    dev = env.dev
    clips = env.clips[:3]
    so = cc.offsets_of([len(c) for c in clips])
    cap = int(so[-1]) + 100
    buf = torch.zeros(cap, dtype=torch.int16, device=dev)
    rates = [env.rate] * 3
    for obj, args in ((MixedRateFeatureBatch(), (buf, so, rates)), (env.ens.MixedRateEnsembleBatch(env.head, env.rules), (buf, so, rates))):
        with pytest.raises(NotImplementedError, match='mixed-rate'):
            obj.capture(*args, capacity=cap)
        with pytest.raises(NotImplementedError, match='mixed-rate'):
            obj.run(*args, capacity=cap)
    wrong = torch.zeros(cap - 1, dtype=torch.int16, device=dev)
    mfb = ModelFeatureBatch(rate=env.rate)
    eb = env.ens.EnsembleBatch(env.rate, env.head, env.rules)
    lab = torch.zeros(5, dtype=torch.int64, device=dev)
    so5 = cc.offsets_of([len(c) for c in env.clips[:5]])
    tb = TrainBatch(env.rate, _head('HMRNNHead', dev))
    for call in (lambda: mfb.capture(wrong, so, capacity=cap), lambda: mfb.run(wrong, so, capacity=cap),
                 lambda: eb.capture(wrong, so, capacity=cap, dropout=False), lambda: eb.run(wrong, so, capacity=cap, dropout=False),
                 lambda: tb.capture(wrong, so5, lab, None, capacity=cap, dropout=False),
                 lambda: tb.run(wrong, so5, lab, None, capacity=cap, dropout=False),
                 lambda: mfb.capture(buf.unsqueeze(0), so, capacity=cap)):
        with pytest.raises(ValueError, match='exactly that many samples'):
            call()
    with pytest.raises(TypeError, match='device tensor'):
        mfb.run(np.zeros(cap, dtype=np.int16), so, capacity=cap)
    assert all(3 not in sizes for sizes in CAPTURE_VERIFIED.values())
    with pytest.raises(NotImplementedError, match='CAPTURE_VERIFIED'):
        TrainBatch(env.rate, _head('HMRNNHead', dev)).capture(buf, so, torch.zeros(3, dtype=torch.int64, device=dev), None, capacity=cap,
                                                              dropout=False)
