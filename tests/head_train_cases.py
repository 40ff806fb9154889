"""Shared by tests/test_head_train_host.py (CPU) and tests/test_gpu_head_train.py: NumPy restatements, in fp64 or fp32
(``dtype``), of the training entry points of the heads (include/dsp_frontend.h: dsp_head_pool_train_batch,
dsp_head_pool_backward_batch, dsp_selfattn_pool_rows_train_batch / dsp_selfattn_pool_rows_backward_batch) and the cases both
files run on top of tests/head_pool_cases.py.  Like the forward's restatement they read rows t < len (t < rows) only."""
import numpy as np

import head_pool_cases as hp


# ---- the restatements -------------------------------------------------------------------------------------------------------

def pool_train_ref(y, lens, rows=None, dtype=np.float64):
    """y [T, B, H] -> (avg [B, H], mx [B, H], arg [B, H] int64).  arg: the smallest t < len whose value the max column
    returned -- the first NaN row if there is one --, -1 where the padding's 0 won (len < rows and 0 > max over the active
    rows; a tie between an active 0.0 and the padding goes to the active row)."""
    y = np.asarray(y)
    T, B, H = y.shape
    rows = T if rows is None else min(int(rows), T)
    avg, mx = hp.pool_ref(y, lens, rows)
    arg = np.empty((B, H), dtype=np.int64)
    for b in range(B):
        n = int(np.clip(lens[b], 1, T))
        a = np.asarray(y[:n, b], dtype=np.float64)
        nan = np.isnan(a)
        first = np.where(nan.any(0), nan.argmax(0), np.where(nan, -np.inf, a).argmax(0))      # argmax: the first occurrence
        m = a[first, np.arange(H)]
        arg[b] = np.where((n < rows) & (0.0 > m), -1, first)                                  # (0 > NaN is False: the NaN stays)
    return avg.astype(dtype), mx.astype(dtype), arg


def pool_backward_ref(g_avg, g_max, lens, arg, T, dtype=np.float64):
    """g_avg [B, H] or None (col_avg < 0), g_max [B, H], arg [B, H] -> g_y [T, B, H] in ``dtype``, every operation in ``dtype``:
    t < len: (g_avg / len, formed once per (b, h), or 0) + (arg == t ? g_max : 0); t >= len: 0."""
    g_max = np.asarray(g_max, dtype=dtype)
    B, H = g_max.shape
    out = np.zeros((T, B, H), dtype=dtype)
    t = np.arange(T)[:, None]
    for b in range(B):
        n = int(np.clip(lens[b], 1, T))
        q = np.zeros(H, dtype=dtype) if g_avg is None else np.asarray(g_avg[b], dtype=dtype) / dtype(n)
        rows = q[None, :] + np.where(np.asarray(arg[b])[None, :] == t, g_max[b][None, :], dtype(0))
        out[:n, b] = rows[:n].astype(dtype)
    return out


def selfattn_rows_train_ref(y, rows, W, bW, v, c, g_out, dtype=np.float64):
    """layers.SelfAttn and its backward over the first r = clamp(rows, 1, T) rows of y [T, B, H], in ``dtype`` -> a dict of
    out [B, H], w [T, B], g_y [T, B, H], g_pre [T, B, H], g_e [T, B] (all zero at t >= r), gv_part [B, H] = sum_t g_e tanh(.),
    and the parameter gradients gW [H, H], gbW [H], gv [1, H], gc [1] as the sums over them."""
    y = np.asarray(y)
    T, B, H = y.shape
    r = max(1, min(int(rows), T))
    yy = y[:r].astype(dtype)
    W, bW, v = np.asarray(W, dtype=dtype), np.asarray(bW, dtype=dtype), np.asarray(v, dtype=dtype).reshape(-1)
    g_out = np.asarray(g_out, dtype=dtype)
    th = np.tanh(yy @ W.T + bW)                                                 # [r, B, H]
    e = th @ v + dtype(np.asarray(c).reshape(-1)[0])                            # [r, B]
    w = np.exp(e - e.max(0, keepdims=True))
    w = w / w.sum(0, keepdims=True)
    g_w = np.einsum('bh,tbh->tb', g_out, yy)
    g_e = w * (g_w - (w * g_w).sum(0, keepdims=True))
    g_pre = g_e[:, :, None] * v[None, None, :] * (1 - th * th)
    g_y = w[:, :, None] * g_out[None] + g_pre @ W
    pad = lambda a: np.concatenate([a, np.zeros((T - r,) + a.shape[1:], dtype=a.dtype)], 0).astype(dtype)
    return dict(out=np.einsum('tb,tbh->bh', w, yy).astype(dtype), w=pad(w), g_y=pad(g_y), g_pre=pad(g_pre), g_e=pad(g_e),
                gv_part=np.einsum('tb,tbh->bh', g_e, th).astype(dtype),
                gW=np.einsum('tbn,tbk->nk', g_pre, yy), gbW=g_pre.sum((0, 1)), gv=np.einsum('tb,tbh->h', g_e, th)[None, :],
                gc=g_e.sum().reshape(1))


# ---- the cases --------------------------------------------------------------------------------------------------------------

def grad_case(B, H, seed=0, exact=False, avg=True):
    """-> (g_avg [B, H] fp32 or None, g_max [B, H] fp32); ``exact``: on a 1/64 grid."""
    rng = np.random.default_rng(31 + 7 * B + H + seed)
    g = rng.standard_normal((2, B, H)).astype(np.float32)
    if exact:
        g = (np.round(g * 64) / 64).astype(np.float32)
    return (g[0] if avg else None), g[1]


def tie_variants(T, B, H):
    """The ``exact=True`` variants of a shape with ties for the maximum planted in every column of the batch that has six active
    rows and no other role (not all-negative, no NaN): in h = 0 at rows (t, t + 1) -- two waves of the kernel, which meet in the
    LDS combine --, in the last h at rows (t, t + 4) -- one wave, four rows apart -- and, where H >= 3, in h = 1 at rows
    (t + 1, t + 4), again two waves.  The smallest row must win every time.  -> the variants, each with ``ties``: a list of
    (b, h, smallest row)."""
    out = []
    for v in hp.pool_variants(T, B, H, exact=True):
        v = dict(v, y=v['y'].copy(), clean=v['clean'].copy(), ties=[])
        for b in range(B):
            n = int(v['lens'][b])
            if n < 6 or (v['nan_at'] is not None and v['nan_at'][1] == b) or b in v['neg_eq'] or b in v['neg_lt']:
                continue                                                           # (the all-negative columns keep their property)
            t = (n - 5) // 2
            top = np.float32(np.nanmax(v['y'][:n, b]) + 1.0)                       # on the grid, above every active value
            plant = [(0, (t, t + 1), t), (H - 1, (t, t + 4), t)] + ([(1, (t + 4, t + 1), t + 1)] if H >= 3 else [])
            for h, where, first in plant:
                if h in [p[1] for p in v['ties'] if p[0] == b]:
                    continue
                for key in ('y', 'clean'):
                    v[key][list(where), b, h] = top
                v['ties'].append((b, h, first))
        out.append(v)
    return out


def pow2_variants(T, B, H):
    """The ``exact=True`` variants with every length replaced by a power of two <= rows: g / len and the sum behind it are
    then exact in fp32 for gradients on the 1/64 grid, so any correct backward gives the fp32 restatement's BITS."""
    out = []
    for v in hp.pool_variants(T, B, H, exact=True):
        rng = np.random.default_rng(T + B + H + v['rows'])
        top = int(np.log2(v['rows']))
        lens = (2 ** rng.integers(0, top + 1, size=B)).astype(np.int32)
        lens[0] = 2 ** top
        y = rng.standard_normal((T, B, H)).astype(np.float32)
        y = (np.round(y * 64) / 64).astype(np.float32)
        clean = y.copy()
        for b in range(B):
            y[lens[b]:, b] = np.nan
            clean[lens[b]:, b] = 0.0
        out.append(dict(y=y, clean=clean, lens=lens, rows=v['rows'], neg_eq=[], neg_lt=[], nan_at=None))
    return out
