"""Shared by tests/test_capacity_layout_host.py (CPU) and tests/test_gpu_capacity_layout.py: a NumPy restatement of what
dsp_batch_offsets_batch computes (include/dsp_frontend.h) -- the sanitised sample offsets, the status word, the frame offsets of
sigproc.py:79-82 -- and of the bound dsp_frames_bound returns.  Written out here; it calls nothing from the package under test."""
import numpy as np

BIT_FIRST_NOT_ZERO, BIT_DECREASING, BIT_ABOVE_CAPACITY, BIT_EMPTY_CLIP = 1, 2, 4, 8


def frame_count(n, L, S):
    """sigproc.py:79-82: one frame up to L samples, then one more per started hop."""
    n, L, S = int(n), int(L), int(S)
    return 1 if n <= L else 1 + -(-(n - L) // S)


def frame_offsets(so, L, S):
    so = np.asarray(so, dtype=np.int64)
    return np.concatenate(([0], np.cumsum([frame_count(n, L, S) for n in np.diff(so)]))).astype(np.int64)


def frames_bound(capacity, n_utt, L, S):
    """T(n) <= n // S + 1 where L >= S, <= n // S + 2 always; sum_b (n_b // S) <= (sum_b n_b) // S <= capacity // S."""
    return int(capacity) // int(S) + (1 if L >= S else 2) * int(n_utt)


def sanitise(so_in, capacity):
    """out[0] = 0, out[b + 1] = clamp(in[b + 1], out[b], capacity)."""
    so_in = np.asarray(so_in, dtype=np.int64)
    out = np.zeros_like(so_in)
    for b in range(len(so_in) - 1):
        out[b + 1] = min(max(int(so_in[b + 1]), int(out[b])), int(capacity))
    return out


def status(so_in, capacity):
    """The status word, from the caller's table as it stands."""
    so_in = np.asarray(so_in, dtype=np.int64)
    d = np.diff(so_in)
    return ((BIT_FIRST_NOT_ZERO if so_in[0] != 0 else 0) | (BIT_DECREASING if np.any(d < 0) else 0) |
            (BIT_ABOVE_CAPACITY if np.any(so_in > capacity) else 0) | (BIT_EMPTY_CLIP if np.any(d == 0) else 0))


def offsets_of(lengths):
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)


def invalid_tables(so, capacity):
    """Four tables made from the valid ``so`` (clips of at least 3 samples, ``so[-1] <= capacity``), one per status bit: exactly
    that bit is set."""
    so = np.asarray(so, dtype=np.int64)
    assert len(so) >= 2 and so[0] == 0 and np.all(np.diff(so) >= 3) and so[-1] <= capacity
    first = so.copy()
    first[0] = 1                                   # in[0] != 0; the first clip keeps at least two samples
    dec = so.copy()
    dec[-1] = so[-2] - 1                           # the last pair decreases (one clip: [0, -1])
    above = so.copy()
    above[-1] = capacity + 5                       # the last offset alone
    empty = so.copy()
    empty[-1] = so[-2]                             # the last clip has no samples
    out = {BIT_FIRST_NOT_ZERO: first, BIT_DECREASING: dec, BIT_ABOVE_CAPACITY: above, BIT_EMPTY_CLIP: empty}
    for bit, t in out.items():
        assert status(t, capacity) == bit, (bit, status(t, capacity))
    return out
