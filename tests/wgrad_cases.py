"""A NumPy fp64 interpreter of the plans of features/wgrad.py, and the random cases the host and GPU tests share.

``interpret(plan, buffers, rows)`` computes every output of a plan from the products' DESCRIPTORS and nothing else: a buffer is
a flat array, an operand is (offset, t stride, b stride, columns), and only rows t < R are ever addressed (every index is formed
from ``range(R)``).  It is the yardstick of the GPU tests (tests/test_gpu_wgrad.py)."""
import numpy as np
import torch


def _flat(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).reshape(-1).astype(np.float64)


def plan_buffers(plan):
    """name -> flat fp64 array of every buffer of ``plan``."""
    return {k: _flat(v) for k, v in plan.buffers.items()}


def bound(rows, T):
    return T if rows is None else min(max(int(rows), 1), T)


def gather(buf, op, ts, B):
    """Rows ``ts`` of an operand -> [len(ts), B, cols]."""
    ts = np.asarray(ts, dtype=np.int64)
    idx = (op['offset'] + ts[:, None, None] * op['stride_t'] + np.arange(B, dtype=np.int64)[None, :, None] * op['stride_b']
           + np.arange(op['cols'], dtype=np.int64)[None, None, :])
    return buf[idx]


def interpret_product(p, buffers, T, B, rows=None):
    """One product -> (out or None, colsum or None) for 'wgrad', out for 'product'."""
    R = bound(rows, T)
    if p['kind'] == 'product':
        y = np.zeros((T, B, p['n']))
        for a, w in p['terms']:
            W = buffers[w['buf']][w['offset']:w['offset'] + a['cols'] * p['n']].reshape(a['cols'], p['n'])
            y[:R] += gather(buffers[a['buf']], a, range(R), B) @ W
        return y
    a, x, shift = p['a'], p['x'], p['shift']
    A = gather(buffers[a['buf']], a, range(R), B)                             # [R, B, m]
    X = np.zeros((R, B, x['cols']))
    src = np.arange(R) + shift
    ok = (src >= 0) & (src < R)
    if ok.any():
        X[ok] = gather(buffers[x['buf']], x, src[ok], B)
    if shift == -1 and p['init'] is not None:
        i = p['init']
        idx = i['offset'] + np.arange(B)[:, None] * i['stride_b'] + np.arange(x['cols'])[None, :]
        X[0] = buffers[i['buf']][idx]
    if p['scale'] is not None:
        s = p['scale']
        X = X * buffers[s['buf']][s['offset']:s['offset'] + R * B].reshape(R, B, 1)
    out = A.reshape(R * B, -1).T @ X.reshape(R * B, -1)
    return out, A.sum((0, 1))


def interpret(plan, buffers=None, rows=None):
    """Every output of ``plan`` -> name -> fp64 array."""
    buffers = plan_buffers(plan) if buffers is None else buffers
    outs = {}
    for p in plan.products:
        if p['kind'] == 'product':
            outs[p['out']] = interpret_product(p, buffers, plan.T, plan.B, rows)
        else:
            c, s = interpret_product(p, buffers, plan.T, plan.B, rows)
            if p['out'] is not None:
                outs[p['out']] = c
            if p['colsum'] is not None:
                outs[p['colsum']] = s
    return outs


def finish(plan, outs):
    """``plan.finish`` on the interpreter's arrays -> a tuple of fp64 arrays / None."""
    res = plan.finish({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in outs.items()})
    return tuple(None if r is None else r.numpy() for r in res)


def gru_case(seed, T=7, B=3, I=5, H=4, drop=False, dtype=torch.float64):
    """Random arguments of ``gru_param_grads``: (params, x, out, da, drop)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    params = []
    for _ in (0, 1):
        params += [r(3 * H, I), r(3 * H, H), r(3 * H), r(3 * H)]
    dr = (torch.rand(T, B, I, generator=g, dtype=dtype) < 0.7).to(dtype) / 0.7 if drop else None
    return params, r(T, B, I), r(T, B, 2 * H), r(T, B, 2, 4 * H), dr


def hm_case(seed, T=7, B=3, I=8, H1=4, H2=12, state=False, dtype=torch.float64):
    """Random arguments of ``hm_param_grads``: (params, x, state_in, h_1, h_2, z_1, dfs1, dfs2)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    params = [r(4 * H1 + 1, H1), r(4 * H1 + 1, H2), r(4 * H1 + 1, I), r(4 * H1 + 1), r(4 * H2 + 1, H2), r(4 * H2 + 1, H1), r(4 * H2 + 1)]
    z_1 = (torch.rand(B, T, generator=g) < 0.5).to(torch.uint8)
    state_in = None
    if state:
        state_in = r((2 * H1 + 2 * H2 + 2) * B)
        state_in[2 * H1 * B:(2 * H1 + 1) * B] = (state_in[2 * H1 * B:(2 * H1 + 1) * B] > 0).to(dtype)      # z1 is 0 / 1
    return params, r(T, B, I), state_in, r(B, T, H1), r(B, T, H2), z_1, r(T, B, 4 * H1 + 1), r(T, B, 4 * H2 + 1)


def _view(plan, name, rng, T, B, cols, layout):
    """A random fp32 buffer ``name`` in ``plan`` and the operand that views [T, B, cols] of it.  'tb': dense [T, B, cols]; 'off':
    the d = 1, column 2 .. view of a [T, B, 2, cols + 3] buffer (row stride above the columns, a column offset, as
    da[:, :, d, H:4 H]); 'bt': [B, T, cols], as h_1."""
    from features.wgrad import operand
    shape, op = {'tb': ((T, B, cols), operand(name, 0, B * cols, cols, cols)),
                 'off': ((T, B, 2, cols + 3), operand(name, cols + 3 + 2, B * 2 * (cols + 3), 2 * (cols + 3), cols)),
                 'bt': ((B, T, cols), operand(name, 0, cols, T * cols, cols))}[layout]
    plan.buffers[name] = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    return op


def wgrad_case(seed, m, n, T, B, shift=0, init=False, scale=False, colsum=True, la='tb', lx='tb'):
    """A Plan of ONE row reduction on random fp32 CPU buffers."""
    from features.wgrad import Plan
    rng = np.random.default_rng(seed)
    plan = Plan(T, B)
    a, x = _view(plan, 'a', rng, T, B, m, la), _view(plan, 'x', rng, T, B, n, lx)
    ini = sc = None
    if init:
        plan.buffers['init'] = torch.from_numpy(rng.standard_normal((B, n + 1)).astype(np.float32))
        ini = dict(buf='init', offset=0, stride_b=n + 1)
    if scale:
        plan.buffers['scale'] = torch.from_numpy(rng.integers(0, 2, (T, B)).astype(np.float32) * rng.uniform(0.5, 1.5, (T, B)).astype(np.float32))
        sc = dict(buf='scale', offset=0)
    plan.wgrad(a, x, shift=shift, init=ini, scale=sc, out='c', colsum='cs' if colsum else None)
    return plan


def product_case(seed, ks, n, T, B, layouts=('tb',)):
    """A Plan of ONE row product of len(ks) terms on random fp32 CPU buffers."""
    from features.wgrad import Plan
    rng = np.random.default_rng(seed)
    plan = Plan(T, B)
    terms = []
    for i, (k, lay) in enumerate(zip(ks, layouts)):
        a = _view(plan, f'a{i}', rng, T, B, k, lay)
        plan.buffers[f'w{i}'] = torch.from_numpy(rng.standard_normal((k, n)).astype(np.float32))
        terms.append((a, dict(buf=f'w{i}', offset=0)))
    plan.product(terms, n, 'y')
    return plan


def poisoned(plan, R):
    """The plan with NaN in every row t >= R of every operand and of the scale (buffers cloned; the initial row and the
    matrices stay)."""
    import copy
    new = copy.copy(plan)
    new.buffers = {k: v.clone() for k, v in plan.buffers.items()}
    ops = []
    for p in plan.products:
        ops += [p['a'], p['x']] if p['kind'] == 'wgrad' else [a for a, _ in p['terms']]
        if p['kind'] == 'wgrad' and p['scale'] is not None:
            new.buffers[p['scale']['buf']].view(-1)[p['scale']['offset'] + R * plan.B:] = float('nan')
    for op in ops:
        if R < plan.T:
            ts = np.arange(R, plan.T, dtype=np.int64)
            idx = (op['offset'] + ts[:, None, None] * op['stride_t'] + np.arange(plan.B, dtype=np.int64)[None, :, None] * op['stride_b']
                   + np.arange(op['cols'], dtype=np.int64)[None, None, :])
            new.buffers[op['buf']].view(-1)[torch.from_numpy(idx.reshape(-1))] = float('nan')
    return new


def truncated(plan, R):
    """The first R rows of every operand of ``plan`` as DENSE [R, B, cols] buffers of their own, and the plan over them with
    T = R: the unbounded call a bounded one must equal bit for bit, whatever the strides of the original were."""
    from features.wgrad import Plan, operand
    new = Plan(R, plan.B)
    B = plan.B

    def dense(op):
        name = f'd{len(new.buffers)}'
        flat = plan.buffers[op['buf']].reshape(-1).numpy()
        new.buffers[name] = torch.from_numpy(np.ascontiguousarray(gather(flat, op, range(R), B)))
        return operand(name, 0, B * op['cols'], op['cols'], op['cols'])

    def keep(ref):
        if ref is not None:
            new.buffers[ref['buf']] = plan.buffers[ref['buf']]
        return ref
    for p in plan.products:
        if p['kind'] == 'wgrad':
            sc = p['scale']
            if sc is not None:
                new.buffers['s' + sc['buf']] = plan.buffers[sc['buf']].reshape(-1)[sc['offset']:sc['offset'] + R * B].clone()
                sc = dict(buf='s' + sc['buf'], offset=0)
            new.wgrad(dense(p['a']), dense(p['x']), shift=p['shift'], init=keep(p['init']), scale=sc, out=p['out'], colsum=p['colsum'])
        else:
            new.product([(dense(a), keep(w)) for a, w in p['terms']], p['n'], p['out'])
    return new


def one_off_masks(n):
    """Every mask of n entries, then each with one entry off."""
    yield [True] * n
    for k in range(n):
        yield [j != k for j in range(n)]
