#!/usr/bin/env python3
"""Timing of the HM-LSTM forward (features/classifier.py::HMLSTM): the native call (dsp_hmlstm_forward, one persistent HIP
launch) against the torch step loop on the same device in the same process, alternating, at the reference's sizes
(200, [200, 200]), T = 200, B in {8, 64, 512}; and the whole HMRNNHead at B = 512 next to RNNHead.

    python tools/kbench_hmlstm.py [--out profiles/hmlstm_kbench.json] [--rounds 5]
    python tools/kbench_hmlstm.py --kernel-only B      # one warm-up and ten native calls, for a rocprofv3 --kernel-trace run
    python tools/kbench_hmlstm.py --scan-seeds          # CPU only: the seeds of tests/test_gpu_hmlstm.py::LOOP_CASES
    python tools/kbench_hmlstm.py --train [--parent-lib LIB] [--out profiles/hmlstm_train_kbench.json]
                                                        # the training step: native forward_train / backward / GEMMs
                                                        # against the torch loop, the head, and the guard on the plain forward
    python tools/kbench_hmlstm.py --scan-train-seeds    # CPU only: the seeds of tests/test_gpu_hmlstm_train.py
    python tools/kbench_hmlstm.py --ab PARENT_LIB [--out FILE.json]
                                                        # same-speed check against a build of the parent commit (kbench_bigru.py's
                                                        # --ab): forward, forward_train, backward and the HMRNN head at B 512

Times are device-event times around calls on one stream, median over the rounds (min and max are kept beside it); every
shape is warmed up first.  The operation count is 2 (4H+1) (I + H2 + H1 + H1 + H2) per column and step.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'dsp-speech-recognition_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
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


def scan_seeds():
    """For every (B, T, shape) of the GPU test's table: the first seed from its base whose torch-loop run on the CPU leaves
    out at most 0.25 % of the decisions under the guard rule."""
    import hmrnn_cases as hc
    import test_gpu_hmlstm as tg
    from features.classifier import HMLSTM, fill_parameters
    for B, T, shape, _ in tg.LOOP_CASES:
        I, sizes = tg.SHAPES[shape]
        for seed in range(20260700, 20260700 + 200):
            torch.manual_seed(0)
            m = HMLSTM(1.0, I, list(sizes)).eval()
            fill_parameters(m, seed)
            x = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((T, B, I)).astype(np.float32))
            with torch.no_grad():
                zh = m.run(x, native=False).z_hat.numpy()
            share = hc.left_out_share(hc.cuts(zh), T)
            if share <= 0.0025:
                print(f"    ({B}, {T}, '{shape}', {seed}),   # left out {share:.4f}, boundary rates "
                      f"{(zh[:, 0] > 0.5).mean():.2f} / {(zh[:, 1] > 0.5).mean():.2f}", flush=True)
                break


def scan_train_seeds():
    """CPU only: the seed tables of tests/test_gpu_hmlstm_train.py -- for every gradient case the first seed from 20260900 at
    which the fp64 loop drops no column (in any variant the tests use), and the head's seed: no decision of the fp32 loop
    within 1e-3 of 0.5 or of the clamp's ends."""
    import hmrnn_cases as hc
    import test_gpu_hmlstm_train as tt
    for B, T, shape, _ in tt.GRAD_CASES:
        variants = [dict()] + ([dict(with_state=True), dict(lens_kind='edges')] if (B, T, shape) == (19, 7, 'c') else [])
        for seed in range(20260900, 20260900 + 200):
            cases = [tt.truth(B, T, shape, seed, **kw) for kw in variants]
            if all(c['keep'].all() for c in cases):
                print(f"    ({B}, {T}, '{shape}', {seed}),   # dropped 0, boundary rates {cases[0]['rates'][0]:.2f} / {cases[0]['rates'][1]:.2f}", flush=True)
                break
    for seed in range(20260900, 20260900 + 200):
        head, inp, len0, _ = tt._head_case(seed)
        with torch.no_grad():
            enc = head.enc1(torch.from_numpy(inp), len0)
            zh = head.enc2.run(enc, None, lens=len0, native=False).z_hat.numpy()
        if tt.kept_columns(zh, 1e-3).all():
            print(f'HEAD_SEED = {seed}   # boundary rates {(zh[:, 0] > 0.5).mean():.2f} / {(zh[:, 1] > 0.5).mean():.2f}', flush=True)
            break


def _forward_ms_in_child(lib, rounds):
    """The timed calls at B 512 in a fresh process on the given library -> {call: the rounds' times} (this process keeps its own)."""
    import subprocess
    env = dict(os.environ, DSP_FRONTEND_LIB=lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--forward-rounds', str(rounds)], env=env, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


def forward_rounds(rounds):
    """Child process of --train's guard and of --ab: 'forward' is dsp_hmlstm_forward through HMLSTM.run; forward_train and
    backward are the raw calls; the HMRNN head (native GRU encoder and HM-LSTM) forward and training step."""
    import ctypes
    from features import _native as nat
    from features.classifier import HMLSTM, HMRNNHead, fill_parameters
    probe = ctypes.CDLL(nat.LIB_PATH)
    for name in [n for n in nat.SIGNATURES if not hasattr(probe, n)]:     # a build of an older commit: these calls need none of them
        del nat.SIGNATURES[name]
    lib, dev = nat.load(), torch.device('cuda', 0)
    I, H1, H2, T, B = 200, 200, 200, 200, 512
    torch.manual_seed(0)
    m = HMLSTM(1.0, I, [H1, H2]).eval()
    fill_parameters(m, 1)
    m = m.to(dev)
    rng = np.random.default_rng(2)
    new = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)
    x, g1, g2, gl = new(T, B, I), new(B, T, H1), new(B, T, H2), new(B, H2)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    handle, n = m._native_handle(dev), nat.c_i64(0)
    nat.check(lib.dsp_hmlstm_tape_bytes(handle, T, B, nat.C.byref(n)))
    f32 = dict(dtype=torch.float32, device=dev)
    tape, h1, h2 = torch.empty(n.value // 4, **f32), torch.empty(B, T, H1, **f32), torch.empty(B, T, H2, **f32)
    z1, z2 = torch.empty(B, T, dtype=torch.uint8, device=dev), torch.empty(B, T, dtype=torch.uint8, device=dev)
    zhat, last, state = torch.empty(T, 2, B, **f32), torch.empty(B, H2, **f32), torch.empty((2 * H1 + 2 * H2 + 2) * B, **f32)
    d1, d2 = torch.empty(T, B, 4 * H1 + 1, **f32), torch.empty(T, B, 4 * H2 + 1, **f32)
    st = lambda: torch.cuda.current_stream(dev).cuda_stream
    inp, wl = new(T, B, 39), new(B, 20)
    len0 = rng.integers(20, T + 1, B)
    len0[0] = T
    torch.manual_seed(0)
    hm = HMRNNHead().to(dev)

    def head_forward():
        with torch.no_grad():
            hm(inp, len0, dropout=True, native=True, native_enc=True)

    def head_step():
        (hm(inp, len0, dropout=True, native=True, native_enc=True)[0] * wl).sum().backward()
        hm.zero_grad(set_to_none=True)

    def forward():
        with torch.no_grad():
            m.run(x, native=True)
    runs = {'forward': forward,
            'forward_train': lambda: nat.check(lib.dsp_hmlstm_forward_train(handle, x.data_ptr(), T, B, 1.0, lens.data_ptr(), None, state.data_ptr(),
                                                                            h1.data_ptr(), h2.data_ptr(), z1.data_ptr(), z2.data_ptr(), zhat.data_ptr(),
                                                                            last.data_ptr(), tape.data_ptr(), n.value, st())),
            'backward': lambda: nat.check(lib.dsp_hmlstm_backward(handle, T, B, 1.0, lens.data_ptr(), None, tape.data_ptr(), n.value, h1.data_ptr(),
                                                                  h2.data_ptr(), z1.data_ptr(), z2.data_ptr(), g1.data_ptr(), g2.data_ptr(),
                                                                  gl.data_ptr(), d1.data_ptr(), d2.data_ptr(), st())),
            'HMRNNHead_forward_all_native': head_forward, 'HMRNNHead_train_step_all_native': head_step}
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    print(json.dumps({k: [_time(f, 5) for _ in range(rounds)] for k, f in runs.items()}))


def train(args):
    """The training step: native forward_train, backward and the GEMMs (separately and as one autograd step) against the torch
    loop's forward + backward, alternating; the whole HMRNNHead at B 512; and the guard on dsp_hmlstm_forward against a build
    of the parent commit (--parent-lib, e.g. from tools/build_variants.sh), each library in a process of its own, alternating."""
    from features import _native as nat
    from features.classifier import HMLSTM, HMRNNHead, fill_parameters, hm_param_grads
    dev = torch.device('cuda', 0)
    I, sizes, T = 200, [200, 200], 200
    H1, H2 = sizes
    torch.manual_seed(0)
    m = HMLSTM(1.0, I, sizes)
    fill_parameters(m, 1)
    m = m.to(dev)
    rng = np.random.default_rng(2)
    res = {'shape': {'input_size': I, 'sizes': sizes, 'T': T}, 'hmlstm_train': {}, 'heads_train': {}, 'forward_guard': {}}
    lib = nat.load()
    for B in (8, 64, 512):
        new = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)
        x, g1, g2, gl = new(T, B, I), new(B, T, H1), new(B, T, H2), new(B, H2)
        xg = x.clone().requires_grad_(True)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)

        def step(native):
            r = m.run(xg, None, lens=lens.cpu().numpy(), native=native)
            torch.autograd.backward([r.h_1, r.h_2, r.last_h2], [g1, g2, gl])
            m.zero_grad(set_to_none=True); xg.grad = None
        # the three parts of the native step on raw buffers
        handle = m._native_handle(dev)
        n = nat.c_i64(0)
        nat.check(lib.dsp_hmlstm_tape_bytes(handle, T, B, nat.C.byref(n)))
        f32 = dict(dtype=torch.float32, device=dev)
        tape = torch.empty(n.value // 4, **f32)
        h1, h2 = torch.empty(B, T, H1, **f32), torch.empty(B, T, H2, **f32)
        z1, z2 = torch.empty(B, T, dtype=torch.uint8, device=dev), torch.empty(B, T, dtype=torch.uint8, device=dev)
        zhat, last, state = torch.empty(T, 2, B, **f32), torch.empty(B, H2, **f32), torch.empty((2 * H1 + 2 * H2 + 2) * B, **f32)
        d1, d2 = torch.empty(T, B, 4 * H1 + 1, **f32), torch.empty(T, B, 4 * H2 + 1, **f32)
        st = lambda: torch.cuda.current_stream(dev).cuda_stream
        fwd = lambda: nat.check(lib.dsp_hmlstm_forward_train(handle, x.data_ptr(), T, B, 1.0, lens.data_ptr(), None, state.data_ptr(),
                                                             h1.data_ptr(), h2.data_ptr(), z1.data_ptr(), z2.data_ptr(), zhat.data_ptr(),
                                                             last.data_ptr(), tape.data_ptr(), n.value, st()))
        bwd = lambda: nat.check(lib.dsp_hmlstm_backward(handle, T, B, 1.0, lens.data_ptr(), None, tape.data_ptr(), n.value, h1.data_ptr(),
                                                        h2.data_ptr(), z1.data_ptr(), z2.data_ptr(), g1.data_ptr(), g2.data_ptr(),
                                                        gl.data_ptr(), d1.data_ptr(), d2.data_ptr(), st()))
        params = [p.detach() for p in m._params()]
        gemms = lambda: hm_param_grads(params, x, None, h1, h2, z1, d1, d2)
        runs = {'forward_train': (fwd, 5), 'backward': (bwd, 5), 'gemms': (gemms, 5), 'native_step': (lambda: step(True), 3),
                'torch_loop_step': (lambda: step(False), 1)}
        for f, _ in runs.values():
            f()
        torch.cuda.synchronize()
        ts = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, (f, reps) in runs.items():
                ts[k].append(_time(f, reps))
        r = {k: _stats(v) for k, v in ts.items()}
        r['tape_bytes'] = n.value
        r['sum_of_parts_ms'] = sum(r[k]['median_ms'] for k in ('forward_train', 'backward', 'gemms'))
        r['speedup'] = r['torch_loop_step']['median_ms'] / r['native_step']['median_ms']
        res['hmlstm_train'][str(B)] = r
        print(f"B {B:4d}: forward_train {r['forward_train']['median_ms']:.2f} + backward {r['backward']['median_ms']:.2f} + GEMMs "
              f"{r['gemms']['median_ms']:.2f} = {r['sum_of_parts_ms']:.2f} ms; autograd step native {r['native_step']['median_ms']:.2f} ms, "
              f"torch loop {r['torch_loop_step']['median_ms']:.1f} ms -> x{r['speedup']:.1f}; tape {n.value / 2**20:.0f} MiB", flush=True)
        del tape, d1, d2
    B = 512
    inp = torch.from_numpy(rng.standard_normal((T, B, 39)).astype(np.float32)).to(dev)
    len0 = rng.integers(20, T + 1, B)
    len0[0] = T
    wl = torch.from_numpy(rng.standard_normal((B, 20)).astype(np.float32)).to(dev)
    torch.manual_seed(0)
    hm = HMRNNHead().to(dev)

    def head_step(native):
        lo, _ = hm(inp, len0, dropout=True, native=native)
        (lo * wl).sum().backward()
        hm.zero_grad(set_to_none=True)
    for nv in (True, False):
        head_step(nv)
    torch.cuda.synchronize()
    ts = {True: [], False: []}
    for _ in range(args.rounds):
        for nv in (True, False):
            ts[nv].append(_time(lambda: head_step(nv), 1))
    res['heads_train'] = {'HMRNNHead_native': _stats(ts[True]), 'HMRNNHead_torch_loop': _stats(ts[False])}
    print(f"HMRNNHead forward + backward (B = 512): native {res['heads_train']['HMRNNHead_native']['median_ms']:.1f} ms, torch loop "
          f"{res['heads_train']['HMRNNHead_torch_loop']['median_ms']:.1f} ms", flush=True)
    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as fh:
                json.dump(res, fh, indent=1)
    write()
    if args.parent_lib:
        del hm, inp
        torch.cuda.empty_cache()
        t_par, t_new = [], []
        for _ in range(2):                                                    # alternating processes
            t_par += _forward_ms_in_child(os.path.abspath(args.parent_lib), args.rounds)['forward']
            t_new += _forward_ms_in_child(nat.LIB_PATH, args.rounds)['forward']
        g = {'B': 512, 'parent': _stats(t_par), 'this_tree': _stats(t_new)}
        # the margin: the parent's own min-max spread of rounds as profiles/hmlstm_kbench.json records it (this job's is kept beside it)
        with open(os.path.join(ROOT, 'profiles', 'hmlstm_kbench.json')) as fh:
            rec = json.load(fh)['hmlstm']['512']['native']
        g['margin_ms'] = rec['max_ms'] - rec['min_ms']
        g['parent_spread_this_job_ms'] = g['parent']['max_ms'] - g['parent']['min_ms']
        g['no_slower'] = g['this_tree']['median_ms'] <= g['parent']['median_ms'] + g['margin_ms']
        res['forward_guard'] = g
        print(f"dsp_hmlstm_forward (B = 512): parent {g['parent']['median_ms']:.3f} ms (min {g['parent']['min_ms']:.3f}, max "
              f"{g['parent']['max_ms']:.3f}), this tree {g['this_tree']['median_ms']:.3f} ms -> no slower: {g['no_slower']}", flush=True)
    write()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--kernel-only', type=int, default=0, metavar='B')
    ap.add_argument('--scan-seeds', action='store_true')
    ap.add_argument('--scan-train-seeds', action='store_true')
    ap.add_argument('--train', action='store_true')
    ap.add_argument('--parent-lib', default=None, help='with --train: a build of the parent commit, for the forward guard')
    ap.add_argument('--ab', default=None, metavar='PARENT_LIB', help='same-speed check against a build of the parent commit')
    ap.add_argument('--forward-rounds', type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.forward_rounds:
        return forward_rounds(args.forward_rounds)
    if args.ab:
        import kbench_bigru
        return kbench_bigru.ab(args, _forward_ms_in_child)
    if args.scan_seeds:
        return scan_seeds()
    if args.scan_train_seeds:
        return scan_train_seeds()
    if args.train:
        return train(args)
    from features.classifier import HMLSTM, HMRNNHead, RNNHead, fill_parameters
    dev = torch.device('cuda', 0)
    I, sizes, T = 200, [200, 200], 200
    torch.manual_seed(0)
    m = HMLSTM(1.0, I, sizes).eval()
    fill_parameters(m, 1)
    m = m.to(dev)
    rng = np.random.default_rng(2)
    flop_col_step = 2 * ((4 * sizes[0] + 1) * (I + sizes[1] + sizes[0]) + (4 * sizes[1] + 1) * (sizes[0] + sizes[1]))
    if args.kernel_only:
        x = torch.from_numpy(rng.standard_normal((T, args.kernel_only, I)).astype(np.float32)).to(dev)
        with torch.no_grad():
            for _ in range(11):
                m.run(x, native=True)
        torch.cuda.synchronize()
        return
    res = {'shape': {'input_size': I, 'sizes': sizes, 'T': T}, 'hmlstm': {}, 'heads': {}}
    with torch.no_grad():
        for B in (8, 64, 512):
            x = torch.from_numpy(rng.standard_normal((T, B, I)).astype(np.float32)).to(dev)
            nat = lambda: m.run(x, native=True)
            seq_free = lambda: m._run_native(x, None, None, want_seq=False)      # state and z_hat only
            loop = lambda: m.run(x, native=False)
            nat(); seq_free(); loop()
            torch.cuda.synchronize()
            tn, ts, tl = [], [], []
            for _ in range(args.rounds):                                          # alternating
                tn.append(_time(nat, 5)); tl.append(_time(loop, 1)); ts.append(_time(seq_free, 5))
            flop = flop_col_step * B * T
            r = {'native': _stats(tn), 'native_no_sequence_outputs': _stats(ts), 'torch_loop': _stats(tl)}
            r['native_tflops'] = flop / (r['native']['median_ms'] * 1e-3) / 1e12
            r['speedup'] = r['torch_loop']['median_ms'] / r['native']['median_ms']
            res['hmlstm'][str(B)] = r
            print(f"B {B:4d}: native {r['native']['median_ms']:.3f} ms ({r['native_tflops']:.2f} TFLOP/s fp32), without sequence "
                  f"outputs {r['native_no_sequence_outputs']['median_ms']:.3f} ms, torch loop {r['torch_loop']['median_ms']:.2f} ms "
                  f"-> x{r['speedup']:.1f}", flush=True)
        # whole heads at B = 512 on [200, 512, 39]
        B = 512
        inp = torch.from_numpy(rng.standard_normal((T, B, 39)).astype(np.float32)).to(dev)
        len0 = rng.integers(20, T + 1, B)
        len0[0] = T
        torch.manual_seed(0)
        hm, rn = HMRNNHead().eval().to(dev), RNNHead().eval().to(dev)
        runs = {'HMRNNHead_native': lambda: hm(inp, len0, dropout=True, native=True),
                'HMRNNHead_torch_loop': lambda: hm(inp, len0, dropout=True, native=False),
                'RNNHead': lambda: rn(inp, len0)}
        for f in runs.values():
            f()
        torch.cuda.synchronize()
        ts = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, f in runs.items():
                ts[k].append(_time(f, 1 if 'loop' in k else 3))
        for k in runs:
            res['heads'][k] = _stats(ts[k])
            print(f"{k} (B = 512): {res['heads'][k]['median_ms']:.2f} ms", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
