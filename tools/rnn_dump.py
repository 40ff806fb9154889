#!/usr/bin/env python3
"""Every output array of the recurrent entry points (dsp_bigru_*, dsp_hmlstm_*) on seeded inputs, for bitwise comparison of
two builds of the library: the build named by DSP_FRONTEND_LIB (default: this tree's) is run in this process and the arrays
are written to one .npz; --compare then holds two such files against each other.

    DSP_FRONTEND_LIB=<parent build> python tools/rnn_dump.py --out parent.npz
    python tools/rnn_dump.py --out branch.npz
    python tools/rnn_dump.py --compare parent.npz branch.npz      # CPU only; exit status 1 unless every pair is bitwise equal

Shapes: the smallest that reach every instantiation -- hidden sizes 4 / 100 / 132 / 200 / 256 (2 / 4 / 7 / max tiles per wave,
one backward chunk up to 128 and two from 132 on), B = 19 (two slices, the last one partial), T = 5, lengths that include 1
and T and once a NULL length pointer; GRU input sizes 1 / 39 / 512, 1 and 3 layers, with inter-layer multipliers and without;
HM-LSTM input sizes 4 / 200, with an initial state and without.  Every output buffer starts as zeros (the GRU tape keeps what
no step visits).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dsp-speech-recognition_amd'))
import numpy as np

SIZES = (4, 100, 132, 200, 256)
B, T = 19, 5
LENS = np.array([T, 1, 3, 2, T, 4, 1, 2, 3, T, 4, 4, 1, T, 2, 3, 1, T, 2], dtype=np.int32)


def gru_cases():
    """(name, I, H, L, drop, lens): every H x I with one layer; three layers at I = 39 with and without multipliers."""
    for H in SIZES:
        for I in (1, 39, 512):
            yield f'gru_I{I}_H{H}_L1', I, H, 1, False, True
        yield f'gru_I39_H{H}_L3', 39, H, 3, False, True
        yield f'gru_I39_H{H}_L3_drop', 39, H, 3, True, True
    yield 'gru_I39_H132_L3_nolen', 39, 132, 3, False, False


def hm_cases():
    """(name, I, H1, H2, state, lens)"""
    for H in SIZES:
        yield f'hm_I4_H{H}', 4, H, H, False, True
        yield f'hm_I200_H{H}_state', 200, H, H, True, True
    yield 'hm_I4_H132_state', 4, 132, 132, True, True
    yield 'hm_I200_H100_256', 200, 100, 256, False, True
    yield 'hm_I200_H256_4_state_nolen', 200, 256, 4, True, False


def dump(path):
    import torch
    from features import _native as nat
    lib, dev = nat.load(), torch.device('cuda', 0)
    C = nat.C
    out = {}
    st = lambda: torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()
    zeros = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
    d_lens = torch.from_numpy(LENS).to(dev)

    def keep(name, **arrays):
        torch.cuda.synchronize()
        for k, v in arrays.items():
            out[f'{name}.{k}'] = v.cpu().numpy()

    for seed, (name, I, H, L, drop, lens) in enumerate(gru_cases()):
        rng = np.random.default_rng(20261000 + seed)
        new = lambda *s, scale=1.0: torch.from_numpy((scale * rng.standard_normal(s)).astype(np.float32)).to(dev)
        params = []
        for l in range(L):
            for _ in range(2):
                params += [new(3 * H, I if l == 0 else 2 * H, scale=0.3), new(3 * H, H, scale=0.3), new(3 * H, scale=0.3), new(3 * H, scale=0.3)]
        d = nat.BigruDesc(I, H, L, 0)
        d.d_params[:8 * L] = [p.data_ptr() for p in params]
        h = nat.c_vp(0)
        nat.check(lib.dsp_bigru_create(C.byref(d), C.byref(h)))
        x, d_len = new(T, B, I), (d_lens if lens else None)
        mult = (torch.from_numpy((rng.random((L - 1, T, B, 2 * H)) < 0.8).astype(np.float32) / 0.8).to(dev)) if drop else None
        n = nat.c_i64(0)
        nat.check(lib.dsp_bigru_workspace_bytes(h, T, B, C.byref(n)))
        work, y, hn = zeros(n.value // 4), zeros(T, B, H), zeros(2 * L, B, H)
        nat.check(lib.dsp_bigru_forward(h, x.data_ptr(), T, B, ptr(d_len), y.data_ptr(), hn.data_ptr(), work.data_ptr(), n.value, st()))
        keep(name, y=y, h_n=hn)
        nat.check(lib.dsp_bigru_tape_bytes(h, T, B, C.byref(n)))
        tape, y, hn = zeros(n.value // 4), zeros(T, B, H), zeros(2 * L, B, H)
        nat.check(lib.dsp_bigru_forward_train(h, x.data_ptr(), T, B, ptr(d_len), ptr(mult), y.data_ptr(), hn.data_ptr(), tape.data_ptr(), n.value, st()))
        keep(name, train_y=y, train_h_n=hn, tape=tape)
        g_hn = new(2 * L, B, H)
        for l in range(L - 1, -1, -1):
            g, da = new(T, B, H if l == L - 1 else 2 * H), zeros(T, B, 2, 4 * H)
            nat.check(lib.dsp_bigru_backward(h, l, T, B, ptr(d_len), tape.data_ptr(), n.value, g.data_ptr(), g_hn[2 * l:].data_ptr(), da.data_ptr(), st()))
            keep(name, **{f'da_layer{l}': da})
        nat.check(lib.dsp_bigru_destroy(h))

    for seed, (name, I, H1, H2, state, lens) in enumerate(hm_cases()):
        rng = np.random.default_rng(20262000 + seed)
        new = lambda *s, scale=1.0: torch.from_numpy((scale * rng.standard_normal(s)).astype(np.float32)).to(dev)
        r1, r2 = 4 * H1 + 1, 4 * H2 + 1
        params = [new(r1, H1, scale=0.3), new(r1, H2, scale=0.3), new(r1, I, scale=0.3), new(r1, scale=0.3),
                  new(r2, H2, scale=0.3), new(r2, H1, scale=0.3), new(r2, scale=0.3)]
        d = nat.HmlstmDesc(I, H1, H2, 0, *[p.data_ptr() for p in params])
        h = nat.c_vp(0)
        nat.check(lib.dsp_hmlstm_create(C.byref(d), C.byref(h)))
        x, d_len = new(T, B, I), (d_lens if lens else None)
        state_in = None
        if state:
            parts = [new(H1, B), new(H1, B), torch.from_numpy((rng.random((1, B)) < 0.5).astype(np.float32)).to(dev),
                     new(H2, B), new(H2, B), torch.from_numpy((rng.random((1, B)) < 0.5).astype(np.float32)).to(dev)]
            state_in = torch.cat([p.reshape(-1) for p in parts])
        n = nat.c_i64(0)
        nat.check(lib.dsp_hmlstm_tape_bytes(h, T, B, C.byref(n)))
        for mode in ('', 'train_'):
            so, h1, h2 = zeros((2 * H1 + 2 * H2 + 2) * B), zeros(B, T, H1), zeros(B, T, H2)
            z1, z2 = zeros(B, T, dtype=torch.uint8), zeros(B, T, dtype=torch.uint8)
            zhat, last, tape = zeros(T, 2, B), zeros(B, H2), zeros(n.value // 4)
            args = [h, x.data_ptr(), T, B, 1.0, ptr(d_len), ptr(state_in), so.data_ptr(), h1.data_ptr(), h2.data_ptr(), z1.data_ptr(),
                    z2.data_ptr(), zhat.data_ptr(), last.data_ptr()]
            if mode:
                nat.check(lib.dsp_hmlstm_forward_train(*args, tape.data_ptr(), n.value, st()))
                keep(name, train_tape=tape)
            else:
                nat.check(lib.dsp_hmlstm_forward(*args, st()))
            keep(name, **{mode + 'h_1': h1, mode + 'h_2': h2, mode + 'z_1': z1, mode + 'z_2': z2, mode + 'z_hat': zhat,
                          mode + 'last_h2': last, mode + 'state_out': so})
        g1, g2, gl = new(B, T, H1), new(B, T, H2), new(B, H2)
        d1, d2 = zeros(T, B, r1), zeros(T, B, r2)
        nat.check(lib.dsp_hmlstm_backward(h, T, B, 1.0, ptr(d_len), ptr(state_in), tape.data_ptr(), n.value, h1.data_ptr(), h2.data_ptr(),
                                          z1.data_ptr(), z2.data_ptr(), g1.data_ptr(), g2.data_ptr(), gl.data_ptr(), d1.data_ptr(), d2.data_ptr(), st()))
        keep(name, dfs1=d1, dfs2=d2)
        nat.check(lib.dsp_hmlstm_destroy(h))

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(f'{len(out)} arrays from {nat.LIB_PATH} -> {path}')


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    names = sorted(set(a.files) | set(b.files))
    bad = 0
    for k in names:
        if k not in a.files or k not in b.files:
            print(f'   {k:44s} only in {pa if k in a.files else pb}')
            bad += 1
            continue
        u, v = a[k], b[k]
        eq = u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes()
        bad += not eq
        print(f'   {k:44s} {str(u.shape):18s} {str(u.dtype):8s} finite {bool(np.isfinite(u).all())!s:5s} nonzero {int(np.count_nonzero(u)):8d} bitwise_equal {eq}')
    print(f'   {len(names)} arrays, {"ALL BITWISE EQUAL" if not bad else f"{bad} DIFFER"}')
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--compare', nargs=2, default=None, metavar='NPZ')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    dump(args.out or 'rnn_dump.npz')


if __name__ == '__main__':
    main()
