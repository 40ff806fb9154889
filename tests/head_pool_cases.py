"""Shared by tests/test_head_pool_host.py (CPU) and tests/test_gpu_head_pool.py: an fp64 NumPy restatement of the three head
entry points of include/dsp_frontend.h (dsp_head_lengths_batch, dsp_head_pool_batch, dsp_selfattn_pool_rows_batch) and the
cases both files run.  The restatement reads what the kernels read -- rows t < len only -- so NaNs planted behind an
utterance's end cannot reach it either."""
import numpy as np

POOL_SHAPES = [(1, 1, 4), (9, 5, 12), (33, 2, 3), (7, 3, 200), (40, 17, 200), (200, 5, 200)]      # (T, B, H)
LENGTH_B, LENGTH_HIR, LENGTH_T = (1, 5, 64, 65, 1000), (1, 5, 10), 200
ATTN_SHAPES = [(40, 3, 200), (9, 5, 12)]
ATTN_ROWS = lambda T: sorted({r for r in (1, 7, 16, 17, T) if r <= T})


# ---- the restatement --------------------------------------------------------------------------------------------------------

def lengths_ref(len0, T, hir):
    """-> (len0c [B], len1 [B], info [4]) as int64."""
    len0 = np.asarray(len0, dtype=np.int64)
    c = np.clip(len0, 1, T)
    mx = int(c.max())
    return c, (c + hir - 1) // hir, np.array([mx, (mx + hir - 1) // hir, int(np.sum(c != len0)), 0], dtype=np.int64)


def pool_ref(y, lens, rows=None):
    """y [T, B, H] -> (avg [B, H], mx [B, H]) in fp64; rows None = T.  Only y[:len[b], b] is read."""
    y = np.asarray(y, dtype=np.float64)
    T, B, H = y.shape
    rows = T if rows is None else min(int(rows), T)
    avg, mx = np.empty((B, H)), np.empty((B, H))
    for b in range(B):
        n = int(np.clip(lens[b], 1, T))
        a = y[:n, b]
        avg[b] = a.sum(0) / np.float64(n)
        m = np.where(np.isnan(a).any(0), np.nan, np.max(np.where(np.isnan(a), -np.inf, a), axis=0))     # torch.max: a NaN wins
        mx[b] = np.where(np.isnan(m), np.nan, np.maximum(m, 0.0)) if n < rows else m
    return avg, mx


def selfattn_rows_ref(y, rows, W, bW, v, c):
    """layers.SelfAttn over the first min(rows, T) rows of y [T, B, H], fp64 -> [B, H]."""
    y = np.asarray(y, dtype=np.float64)[:max(1, min(int(rows), y.shape[0]))]
    W, bW, v = np.asarray(W, dtype=np.float64), np.asarray(bW, dtype=np.float64), np.asarray(v, dtype=np.float64).reshape(-1)
    e = np.tanh(y @ W.T + bW) @ v + float(np.asarray(c).reshape(-1)[0])             # [rows, B]
    w = np.exp(e - e.max(0, keepdims=True))
    w /= w.sum(0, keepdims=True)
    return np.einsum('tb,tbh->bh', w, y)


# ---- the cases --------------------------------------------------------------------------------------------------------------

def pool_variants(T, B, H, seed=0, exact=False):
    """The runs of one shape: dicts (y fp32 [T, B, H] with NaNs planted in every row t >= len, clean: the same with exact zeros
    there -- what the encoders leave --, lens [B], rows, neg_eq / neg_lt: the all-negative columns with len == rows < T / with
    len < rows, nan_at: (t, b, h) of a NaN planted in an ACTIVE row or None).  Over its variants a shape has every property
    its size allows: len == rows < T and len < rows on all-negative columns (T >= 3), len = 1, len = T, and -- in the
    variant that holds len = T -- a NaN in an active row (last row, last column of batch column 0).  ``exact``: values on a
    1/64 grid, whose sums are exact in any order."""
    rng = np.random.default_rng(1000 * T + 10 * B + H + seed)
    props = []
    if T >= 3:
        r = max(2, T // 2 + 1) if T > 3 else 2
        props += [(r, ('eq', r)), (r, ('lt', int(rng.integers(1, r)))), (r, ('one', 1))]
    props += [(T, ('full', T)), (T, ('one', 1))]
    if T >= 2:
        props.append((T, ('lt', int(rng.integers(1, T)))))
    out = []
    for rows in sorted({p[0] for p in props}):
        mine = [p[1] for p in props if p[0] == rows]
        for k in range(0, len(mine), B):
            chunk = mine[k:k + B]
            lens = rng.integers(1, rows + 1, size=B)
            y = rng.standard_normal((T, B, H)).astype(np.float32)
            if exact:
                y = (np.round(y * 64) / 64).astype(np.float32)
            neg_eq, neg_lt = [], []
            for b, (kind, n) in enumerate(chunk):
                lens[b] = n
                if kind in ('eq', 'lt'):
                    y[:, b] = -np.abs(y[:, b]) - 0.125
                    (neg_eq if kind == 'eq' else neg_lt).append(b)
            clean = y.copy()
            for b in range(B):
                y[lens[b]:, b] = np.nan
                clean[lens[b]:, b] = 0.0
            out.append(dict(y=y, clean=clean, lens=lens.astype(np.int32), rows=int(rows), neg_eq=neg_eq, neg_lt=neg_lt, nan_at=None))
    full = next(v for v in out if v['rows'] == T)                 # its column 0 has len = T: every row is active
    full['nan_at'] = (T - 1, 0, H - 1)
    full['y'][full['nan_at']] = np.nan
    full['clean'][full['nan_at']] = np.nan
    return out


def length_case(B, T=LENGTH_T, seed=0):
    """len0 [B] int32 with the entries 0, -1 and T + 3 among them where B allows (they must be clamped and counted)."""
    rng = np.random.default_rng(77 + B + seed)
    len0 = rng.integers(1, T + 1, size=B).astype(np.int32)
    bad = [0, -1, T + 3][:min(3, B)]
    for k, v in enumerate(bad):
        len0[(k * 7 + 1) % B if B > 8 else k] = v
    return len0, len(bad)


def attn_case(T, B, H, seed=3):
    """-> (y fp32 [T, B, H], W [H, H], bW [H], v [1, H], c [1]): scores of order one, a softmax neither flat nor one-hot."""
    rng = np.random.default_rng(seed + T + B + H)
    f = lambda *s: rng.uniform(-0.3, 0.3, size=s).astype(np.float32)
    return rng.standard_normal((T, B, H)).astype(np.float32), f(H, H), f(H), f(1, H), f(1)
