"""Shared by tests/test_mixed_ensemble_host.py (CPU) and tests/test_gpu_mixed_ensemble.py: a NumPy restatement of what
dsp_scatter_group_rows_batch computes (include/dsp_frontend.h) -- the rate groups' per-slot rows brought back to batch order --
and the tables the two tests run it on.  Written out here; it calls nothing from the package under test."""
import numpy as np

import capacity_cases as cc
import mixed_capacity_cases as mc

SENT_BYTE = 0xA5                 # the fill of an output row nothing wrote
POOL = (44100, 48000, 16000, 8000)


def scatter_rows(group_rows, dst_cols, n_utt, row_bytes, out):
    """out[dst_cols[g][k]] = group_rows[g][k] for every group g and slot k < n_utt, on uint8 [n_utt, row_bytes] tables; a slot
    whose column is negative or >= n_utt is skipped.  ``out`` (uint8 [n_utt, row_bytes]) is changed in place and returned."""
    assert row_bytes % 4 == 0 and 4 <= row_bytes <= 256 and out.shape == (n_utt, row_bytes) and out.dtype == np.uint8
    for rows, cols in zip(group_rows, dst_cols):
        assert rows.shape == (n_utt, row_bytes) and rows.dtype == np.uint8 and len(cols) == n_utt
        for k in range(n_utt):
            col = int(cols[k])
            if 0 <= col < n_utt:
                out[col] = rows[k]
    return out


def tables(B, G, seed, kind='seeded'):
    """-> (rates [B], table of G rates, the dst_col tables [G][B] int32 of ``mixed_capacity_cases.partition``).  ``kind``:
    'seeded' any assignment; 'pads_alone' one table rate does not occur (its group is B pad slots); 'last_group' every clip has
    the table's last rate."""
    table = POOL[:G]
    if kind == 'last_group':
        rates = np.full(B, table[-1], dtype=np.int32)
    else:
        absent = table[seed % G] if kind == 'pads_alone' and G > 1 else None
        rates = mc.rate_vector(B, table, seed, absent=absent)
    so = cc.offsets_of(np.ones(B, dtype=np.int64))
    part = mc.partition(rates, so, table, 1, B)
    return rates, table, [grp['dst_col'].copy() for grp in part['groups']]


def group_rows(B, G, row_bytes, seed):
    """Seeded bytes for every slot of every group, pad slots included (none of them is the fill byte pattern of a whole row)."""
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, 256, (B, row_bytes), dtype=np.uint8) for _ in range(G)]
    for r in rows:
        r[:, 0] = np.where(r[:, 0] == SENT_BYTE, SENT_BYTE ^ 1, r[:, 0])       # no row equals the sentinel row
    return rows
