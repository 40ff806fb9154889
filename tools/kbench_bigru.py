#!/usr/bin/env python3
"""Timing of the bidirectional GRU encoder (features/classifier.py::_DynEnc): the native call (dsp_bigru_forward, one HIP
launch per layer plus the direction sum) against the nn.GRU path (sort, pack, MIOpen, unpack, sum, unsort) on the same device
in the same process, alternating, at 39 -> 200 with 1, 2 and 3 layers, T = 200, B in {8, 64, 512}, with all lengths 200 and
with ragged lengths (the voiced burst of configs[4]: 0.5 .. 0.9 of a 1 .. 2 s clip at 100 frames per second, capped at 200);
and RNNHead and HMRNNHead at B = 512 with the native encoder and without it.

    python tools/kbench_bigru.py [--out profiles/bigru_kbench.json] [--rounds 5]
    python tools/kbench_bigru.py --kernel-only B [--layers L]   # one warm-up and ten native calls, for a rocprofv3 --kernel-trace run
    python tools/kbench_bigru.py --train [--out profiles/bigru_train_kbench.json] [--parent-lib PATH]
        # the training step: forward_train, the backward recurrence per layer, the GEMMs and the whole autograd step, native
        # against the nn.GRU path (39 -> 200, 2 and 3 layers, B 8 / 64 / 512, full and ragged); HMRNNHead and RNNHead training
        # steps at B 512, everything native against everything default; and dsp_bigru_forward against a build of the parent commit
    python tools/kbench_bigru.py --ab PARENT_LIB [--out FILE.json]
        # same-speed check against a build of the parent commit: dsp_bigru_forward, dsp_bigru_forward_train and dsp_bigru_backward
        # per layer (2 and 3 layers, B 512), each library in fresh processes, order parent, this tree, parent, this tree, ...;
        # the parent's processes form two series, whose difference is the bar

Times are device-event times around calls on one stream, median over the rounds (min and max are kept beside it); every
shape is warmed up first.  A direction of a layer multiplies 3 H (in + H) weights per column and step (in = 39, then 2 H).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np
import torch


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _stats(v):
    v = sorted(v)
    return {'median_ms': v[len(v) // 2], 'min_ms': v[0], 'max_ms': v[-1]}


def ragged_lengths(rng, B, T):
    n = (rng.uniform(0.5, 0.9, B) * rng.uniform(1.0, 2.0, B) * 100).astype(np.int64)
    return np.clip(n, 1, T)


def forward_rounds(rounds):
    """Child process of --train's guard and of --ab: the timed calls of the library DSP_FRONTEND_LIB names at 39 -> 200, B 512,
    T 200, full lengths -> {call: the rounds' times}; 'forward' is dsp_bigru_forward with 2 layers."""
    import ctypes
    from features import _native as nat
    from features.classifier import _DynEnc, fill_parameters
    probe = ctypes.CDLL(nat.LIB_PATH)
    for name in [n for n in nat.SIGNATURES if not hasattr(probe, n)]:     # a build of an older commit: these calls need none of them
        del nat.SIGNATURES[name]
    lib, dev = nat.load(), torch.device('cuda', 0)
    I, H, T, B = 39, 200, 200, 512
    rng = np.random.default_rng(2)
    new = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)
    x, lens = new(T, B, I), np.full(B, T)
    d_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    st = lambda: torch.cuda.current_stream(dev).cuda_stream
    out = {}
    for L in (2, 3):
        torch.manual_seed(0)
        enc = _DynEnc(I, H, L).eval()
        fill_parameters(enc, 1)
        enc = enc.to(dev)
        handle, n = enc._native_handle(dev), nat.c_i64(0)
        nat.check(lib.dsp_bigru_tape_bytes(handle, T, B, nat.C.byref(n)))
        tape, y, hn, da = torch.empty(n.value // 4, device=dev), torch.empty(T, B, H, device=dev), torch.empty(2 * L, B, H, device=dev), torch.empty(T, B, 2, 4 * H, device=dev)
        gs, g_hn = [new(T, B, 2 * H) for _ in range(L - 1)] + [new(T, B, H)], new(2 * L, B, H)
        runs = {'forward' if L == 2 else f'forward_layers{L}': lambda: enc.run(x, lens, native=True),
                f'forward_train_layers{L}': lambda: nat.check(lib.dsp_bigru_forward_train(handle, x.data_ptr(), T, B, d_len.data_ptr(), None, y.data_ptr(),
                                                                                          hn.data_ptr(), tape.data_ptr(), n.value, st()))}
        for l in range(L):
            runs[f'backward_layers{L}_layer{l}'] = lambda l=l: nat.check(lib.dsp_bigru_backward(
                handle, l, T, B, d_len.data_ptr(), tape.data_ptr(), n.value, gs[l].data_ptr(), g_hn[2 * l:].data_ptr(), da.data_ptr(), st()))
        with torch.no_grad():
            for f in runs.values():
                f()
            torch.cuda.synchronize()
            for k, f in runs.items():
                out[k] = [_time(f, 5) for _ in range(rounds)]
    print(json.dumps(out))


def _forward_ms_in_child(lib_path, rounds):
    import subprocess
    env = dict(os.environ, DSP_FRONTEND_LIB=lib_path)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--forward-rounds', str(rounds)], env=env, check=True,
                         capture_output=True, text=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


def ab(args, child=_forward_ms_in_child):
    """--ab: this process opens no GPU; four fresh processes per library, alternating, the parent's as two series (its 1st and
    3rd, its 2nd and 4th process).  Per call: the three medians, the bar |parent A - parent B| and whether this tree's median
    is within the bar of the parent's (the median of both series)."""
    from features import _native as nat
    runs = {'parent_a': {}, 'this_tree': {}, 'parent_b': {}}
    for i in range(4):
        for side, lib in (('parent_a' if i % 2 == 0 else 'parent_b', os.path.abspath(args.ab)), ('this_tree', nat.LIB_PATH)):
            for k, v in child(lib, args.rounds).items():
                runs[side].setdefault(k, []).extend(v)
    med = lambda v: sorted(v)[len(v) // 2]
    res = {}
    print(f"{'call':34s} {'parent A':>9s} {'parent B':>9s} {'parent':>9s} {'this tree':>9s} {'b - p':>8s} {'bar':>7s}  verdict (ms, medians)")
    for k in runs['this_tree']:
        a, b2, t = med(runs['parent_a'][k]), med(runs['parent_b'][k]), med(runs['this_tree'][k])
        p = med(runs['parent_a'][k] + runs['parent_b'][k])
        r = res[k] = {'parent_a_ms': a, 'parent_b_ms': b2, 'parent_ms': p, 'this_tree_ms': t, 'bar_ms': abs(a - b2), 'inside': t - p <= abs(a - b2)}
        print(f"{k:34s} {a:9.4f} {b2:9.4f} {p:9.4f} {t:9.4f} {t - p:+8.4f} {r['bar_ms']:7.4f}  {'inside' if r['inside'] else 'BEYOND'}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


def train(args):
    from features import _native as nat
    from features.classifier import _DynEnc, HMRNNHead, RNNHead, fill_parameters, gru_param_grads
    dev = torch.device('cuda', 0)
    I, H, T = 39, 200, 200
    rng = np.random.default_rng(2)
    res = {'shape': {'input_size': I, 'hidden': H, 'T': T}, 'encoder_train': {}, 'heads_train': {}, 'forward_guard': {}}
    lib = nat.load()
    new = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as fh:
                json.dump(res, fh, indent=1)

    for L in (2, 3):
        torch.manual_seed(0)
        enc = _DynEnc(I, H, L)
        fill_parameters(enc, 1)
        enc = enc.to(dev)
        params = [p.detach() for p in enc._params()]
        for B in (8, 64, 512):
            x, g_y, g_hn = new(T, B, I), new(T, B, H), new(2 * L, B, H)
            xg = x.clone().requires_grad_(True)
            for kind, lens in (('full', np.full(B, T)), ('ragged', ragged_lengths(rng, B, T))):
                lens[0] = T                                                     # the same T rows on both paths
                d_len = torch.from_numpy(lens.astype(np.int32)).to(dev)

                def step(native):
                    y, hn = enc.run(xg, lens, native=native)
                    torch.autograd.backward([y, hn], [g_y, g_hn])
                    enc.zero_grad(set_to_none=True); xg.grad = None
                # the parts of the native step on raw buffers
                handle = enc._native_handle(dev)
                n, off = nat.c_i64(0), nat.c_i64(0)
                nat.check(lib.dsp_bigru_tape_bytes(handle, T, B, nat.C.byref(n)))
                tape = torch.empty(n.value // 4, device=dev)
                y, hn = torch.empty(T, B, H, device=dev), torch.empty(2 * L, B, H, device=dev)
                das = [torch.empty(T, B, 2, 4 * H, device=dev) for _ in range(L)]
                gs = [new(T, B, 2 * H) for _ in range(L - 1)] + [g_y]            # stand-ins of dx for the layers below the top
                rows = []
                for l in range(L):
                    nat.check(lib.dsp_bigru_tape_rows(handle, l, T, B, nat.C.byref(off)))
                    rows.append(tape[off.value // 4:off.value // 4 + T * B * 2 * H].view(T, B, 2 * H))
                st = lambda: torch.cuda.current_stream(dev).cuda_stream
                fwd = lambda: nat.check(lib.dsp_bigru_forward_train(handle, x.data_ptr(), T, B, d_len.data_ptr(), None, y.data_ptr(),
                                                                    hn.data_ptr(), tape.data_ptr(), n.value, st()))
                bwd = lambda l: (lambda: nat.check(lib.dsp_bigru_backward(handle, l, T, B, d_len.data_ptr(), tape.data_ptr(), n.value,
                                                                          gs[l].data_ptr(), g_hn[2 * l:].data_ptr(), das[l].data_ptr(), st())))

                def gemms():
                    for l in range(L):
                        gru_param_grads(params[8 * l:8 * l + 8], x if l == 0 else rows[l - 1], rows[l], das[l])
                runs = {'forward_train': (fwd, 3), **{f'backward_layer{l}': (bwd(l), 3) for l in range(L)}, 'gemms': (gemms, 3),
                        'native_step': (lambda: step(True), 2), 'nn_gru_step': (lambda: step(False), 2)}
                for f, _ in runs.values():
                    f()
                torch.cuda.synchronize()
                ts = {k: [] for k in runs}
                for _ in range(args.rounds):                                    # alternating
                    for k, (f, reps) in runs.items():
                        ts[k].append(_time(f, reps))
                r = {k: _stats(v) for k, v in ts.items()}
                r['tape_bytes'], r['mean_len'] = n.value, float(lens.mean())
                r['sum_of_parts_ms'] = sum(v['median_ms'] for k, v in r.items() if isinstance(v, dict) and not k.endswith('_step'))
                r['speedup'] = r['nn_gru_step']['median_ms'] / r['native_step']['median_ms']
                res['encoder_train'][f'layers{L}_B{B}_{kind}'] = r
                print(f"layers {L} B {B:4d} {kind:6s}: forward_train {r['forward_train']['median_ms']:.2f} + backward "
                      + ' + '.join(f"{r[f'backward_layer{l}']['median_ms']:.2f}" for l in range(L))
                      + f" + GEMMs {r['gemms']['median_ms']:.2f} = {r['sum_of_parts_ms']:.2f} ms; autograd step native "
                      f"{r['native_step']['median_ms']:.2f} ms, nn.GRU {r['nn_gru_step']['median_ms']:.2f} ms -> x{r['speedup']:.2f}; "
                      f"tape {n.value / 2**20:.0f} MiB", flush=True)
                del tape, das, rows
                write()
    # whole training steps at B = 512 on [200, 512, 39]: everything native against everything default
    B = 512
    inp = new(T, B, I)
    len0 = ragged_lengths(rng, B, T)
    len0[0] = T
    wl = new(B, 20)
    torch.manual_seed(0)
    hm, rn = HMRNNHead().to(dev), RNNHead().to(dev)

    def head_step(head, **kw):
        lo = head(inp, len0, **kw)
        ((lo[0] if isinstance(lo, tuple) else lo) * wl).sum().backward()
        head.zero_grad(set_to_none=True)
    runs = {'HMRNNHead_all_native': lambda: head_step(hm, dropout=True, native=True, native_enc=True),
            'HMRNNHead_native_hmlstm_nn_gru': lambda: head_step(hm, dropout=True, native=True, native_enc=False),
            'HMRNNHead_default': lambda: head_step(hm, dropout=True),
            'RNNHead_native_enc': lambda: head_step(rn, native_enc=True),
            'RNNHead_default': lambda: head_step(rn)}
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, f in runs.items():
            ts[k].append(_time(f, 1))
    for k in runs:
        res['heads_train'][k] = _stats(ts[k])
        print(f"{k} forward + backward (B = 512, ragged): {res['heads_train'][k]['median_ms']:.1f} ms", flush=True)
    write()
    if args.parent_lib:
        del hm, rn, inp
        torch.cuda.empty_cache()
        t_par, t_new = [], []
        for _ in range(2):                                                    # alternating processes
            t_par += _forward_ms_in_child(os.path.abspath(args.parent_lib), args.rounds)['forward']
            t_new += _forward_ms_in_child(nat.LIB_PATH, args.rounds)['forward']
        g = {'layers': 2, 'B': 512, 'parent': _stats(t_par), 'this_tree': _stats(t_new)}
        g['parent_spread_ms'] = g['parent']['max_ms'] - g['parent']['min_ms']
        g['difference_ms'] = g['this_tree']['median_ms'] - g['parent']['median_ms']
        res['forward_guard'] = g
        print(f"dsp_bigru_forward (2 layers, B = 512): parent {g['parent']['median_ms']:.3f} ms (min {g['parent']['min_ms']:.3f}, max "
              f"{g['parent']['max_ms']:.3f}), this tree {g['this_tree']['median_ms']:.3f} ms (min {g['this_tree']['min_ms']:.3f}, max "
              f"{g['this_tree']['max_ms']:.3f})", flush=True)
    write()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--kernel-only', type=int, default=0, metavar='B')
    ap.add_argument('--layers', type=int, default=2)
    ap.add_argument('--train', action='store_true')
    ap.add_argument('--parent-lib', default=None, help='with --train: a build of the parent commit, for the forward guard')
    ap.add_argument('--ab', default=None, metavar='PARENT_LIB', help='same-speed check against a build of the parent commit')
    ap.add_argument('--forward-rounds', type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.forward_rounds:
        return forward_rounds(args.forward_rounds)
    if args.ab:
        return ab(args)
    if args.train:
        return train(args)
    from features.classifier import _DynEnc, HMRNNHead, RNNHead, fill_parameters
    dev = torch.device('cuda', 0)
    I, H, T = 39, 200, 200
    rng = np.random.default_rng(2)

    def encoder(layers):
        torch.manual_seed(0)
        enc = _DynEnc(I, H, layers).eval()
        fill_parameters(enc, 1)
        return enc.to(dev)

    if args.kernel_only:
        enc = encoder(args.layers)
        x = torch.from_numpy(rng.standard_normal((T, args.kernel_only, I)).astype(np.float32)).to(dev)
        with torch.no_grad():
            for _ in range(11):
                enc.run(x, np.full(args.kernel_only, T), native=True)
        torch.cuda.synchronize()
        return
    res = {'shape': {'input_size': I, 'hidden': H, 'T': T}, 'encoder': {}, 'heads': {}}
    with torch.no_grad():
        for layers in (1, 2, 3):
            enc = encoder(layers)
            mac_col_step = 2 * 3 * H * ((I + H) + (layers - 1) * (2 * H + H))          # both directions
            for B in (8, 64, 512):
                x = torch.from_numpy(rng.standard_normal((T, B, I)).astype(np.float32)).to(dev)
                for kind, lens in (('full', np.full(B, T)), ('ragged', ragged_lengths(rng, B, T))):
                    nat = lambda: enc.run(x, lens, native=True)
                    gru = lambda: enc.run(x, lens, native=False)
                    nat(); gru()
                    torch.cuda.synchronize()
                    tn, tg = [], []
                    for _ in range(args.rounds):                                          # alternating
                        tn.append(_time(nat, 3)); tg.append(_time(gru, 3))
                    r = {'native': _stats(tn), 'nn_gru': _stats(tg), 'mean_len': float(lens.mean())}
                    r['speedup'] = r['nn_gru']['median_ms'] / r['native']['median_ms']
                    r['native_ahead_beyond_ranges'] = r['native']['max_ms'] < r['nn_gru']['min_ms']
                    if kind == 'full':
                        r['native_tflops'] = 2 * mac_col_step * B * T / (r['native']['median_ms'] * 1e-3) / 1e12
                        r['native_us_per_step_and_layer'] = r['native']['median_ms'] * 1e3 / (T * layers)
                    res['encoder'][f'layers{layers}_B{B}_{kind}'] = r
                    print(f"layers {layers} B {B:4d} {kind:6s}: native {r['native']['median_ms']:.3f} ms "
                          f"[{r['native']['min_ms']:.3f}, {r['native']['max_ms']:.3f}], nn.GRU {r['nn_gru']['median_ms']:.3f} ms "
                          f"[{r['nn_gru']['min_ms']:.3f}, {r['nn_gru']['max_ms']:.3f}] -> x{r['speedup']:.2f}", flush=True)
        # whole heads at B = 512 on [200, 512, 39]
        B = 512
        inp = torch.from_numpy(rng.standard_normal((T, B, I)).astype(np.float32)).to(dev)
        len0 = ragged_lengths(rng, B, T)
        len0[0] = T
        torch.manual_seed(0)
        hm, rn = HMRNNHead().eval().to(dev), RNNHead().eval().to(dev)
        runs = {'RNNHead_native_enc': lambda: rn(inp, len0, native_enc=True),
                'RNNHead_nn_gru': lambda: rn(inp, len0, native_enc=False),
                'HMRNNHead_native_enc': lambda: hm(inp, len0, dropout=True, native=True, native_enc=True),
                'HMRNNHead_nn_gru': lambda: hm(inp, len0, dropout=True, native=True, native_enc=False)}
        for f in runs.values():
            f()
        torch.cuda.synchronize()
        ts = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, f in runs.items():
                ts[k].append(_time(f, 3))
        for k in runs:
            res['heads'][k] = _stats(ts[k])
            print(f"{k} (B = 512, ragged): {res['heads'][k]['median_ms']:.2f} ms "
                  f"[{res['heads'][k]['min_ms']:.2f}, {res['heads'][k]['max_ms']:.2f}]", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
