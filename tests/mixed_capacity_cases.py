"""Shared by tests/test_mixed_capacity_host.py (CPU) and tests/test_gpu_mixed_capacity.py: a NumPy restatement of what
dsp_rate_groups_batch computes (include/dsp_frontend.h) -- the sanitised source table, the status word, and per table rate the
stable partition of the batch with its pick / placement columns, rebased offsets, jitter rows and pad slots -- and of what
dsp_gather_groups_batch leaves in a group's wave buffer.  Written out here; it calls nothing from the package under test."""
import numpy as np

import capacity_cases as cc

BIT_UNKNOWN_RATE = 16
PAD_VALUE = 1                    # DSP_GROUP_PAD_VALUE


def first_seen(rates):
    """The distinct rates of a batch in order of first appearance (the order of group_by_rate's groups)."""
    out = []
    for r in np.asarray(rates).reshape(-1).tolist():
        if int(r) not in out:
            out.append(int(r))
    return out


def partition(rates, so_in, table, pad, capacity, jitter=None):
    """-> dict(sanitised [B + 1], status, count [G], groups: one dict(pick, dst_col [B] int32, offsets [B + 1] int64,
    jitter [B, 2] int64 or None) per table rate).  Clip b belongs to the first table rate equal to rates[b]; a rate outside
    the table goes to group 0 and sets bit 4.  Slots count .. B - 1 of a group are pad slots: -1, ``pad`` samples, zero jitter."""
    rates = np.asarray(rates, dtype=np.int64).reshape(-1)
    so_in = np.asarray(so_in, dtype=np.int64).reshape(-1)
    B = len(rates)
    assert len(so_in) == B + 1 and 1 <= len(table) <= 4 and pad >= 1
    san = cc.sanitise(so_in, capacity)
    lens = np.diff(san)
    status = cc.status(so_in, capacity)
    member = np.full(B, -1, dtype=np.int64)
    for b in range(B):
        for g, r in enumerate(table):
            if rates[b] == r:
                member[b] = g
                break
        else:
            member[b] = 0
            status |= BIT_UNKNOWN_RATE
    groups, count = [], []
    for g in range(len(table)):
        idx = [b for b in range(B) if member[b] == g]               # batch order kept: a stable partition
        n = len(idx)
        pick = np.full(B, -1, dtype=np.int32)
        pick[:n] = idx
        off = np.zeros(B + 1, dtype=np.int64)
        off[1:n + 1] = np.cumsum(lens[idx]) if n else []
        off[n + 1:] = off[n] + pad * np.arange(1, B - n + 1)
        jit = None
        if jitter is not None:
            jit = np.zeros((B, 2), dtype=np.int64)
            jit[:n] = np.asarray(jitter, dtype=np.int64).reshape(B, 2)[idx]
        groups.append(dict(pick=pick, dst_col=pick.copy(), offsets=off, jitter=jit))
        count.append(n)
    return dict(sanitised=san, status=int(status), count=np.array(count, dtype=np.int32), groups=groups)


def gathered(wave, part, g, pad):
    """The first offsets[B] samples of group g's wave buffer: its clips (read through the sanitised table) one after the other,
    then ``pad`` samples of PAD_VALUE per pad slot."""
    grp, san = part['groups'][g], part['sanitised']
    out = np.full(int(grp['offsets'][-1]), PAD_VALUE, dtype=wave.dtype)
    for k, b in enumerate(grp['pick'].tolist()):
        if b >= 0:
            out[grp['offsets'][k]:grp['offsets'][k + 1]] = wave[san[b]:san[b + 1]]
    return out


def rate_vector(B, table, seed, absent=None):
    """A seeded assignment of table rates to B positions; ``absent``: a table rate that must not occur."""
    rng = np.random.default_rng(seed)
    pool = [r for r in table if r != absent]
    return np.array([pool[int(i)] for i in rng.integers(0, len(pool), B)], dtype=np.int32)
