#!/usr/bin/env python3
"""The NumPy restatement of ``dsp_rows_colsum`` (include/dsp_frontend.h; csrc/kernels_reduce.h): the partition of the rows over
chunks, workgroups and threads, and the order of every fp32 addition.  ``colsum`` gives the bits the kernels give; it is the
yardstick of tests/test_reduce_host.py (scratch sizes) and tests/test_gpu_reduce.py (bits).

    d_out[c] = sum_{t < R, b < B} a[t, b, c] * (x ? x[t, b, c] : 1)

* chunk k holds the time steps [k steps, (k + 1) steps) with steps = ``chunk_steps(B)``; row g of a chunk is (t0 + g // B, g % B);
* cols >= 64: thread (cg, rg) adds rows rg, rg + 16, .. of its four columns in order, then the 16 row groups are added in order;
* cols < 64: thread tid adds rows tid, tid + 256, .. in order; the 64 lanes of a wave are added by the xor tree 32, 16, .., 1, then
  the 4 waves in order;
* the chunks below ceil(R / steps) are added in order.

Run as a program it prints the partition of a shape: ``rows_sum_emul.py T B cols``."""
import sys

import numpy as np

CHUNK_ROWS, CHUNK_T_MAX, MAX_DIM = 4096, 8, 2048
THREADS, WIDE_MIN, WIDE_COLS, WIDE_ROWGROUPS, NARROW_COLS = 256, 64, 64, 16, 8


def chunk_steps(B):
    return min(max(CHUNK_ROWS // B, 1), CHUNK_T_MAX)


def chunks(T, B):
    return -(-T // chunk_steps(B))


def scratch_bytes(T, B, cols):
    """What ``dsp_rows_colsum_scratch_bytes`` gives: one fp32 partial per (chunk, column), rounded up to 16 bytes."""
    return ((chunks(T, B) * cols + 3) & ~3) * 4


def grid(T, B, cols):
    per = WIDE_COLS if cols >= WIDE_MIN else NARROW_COLS
    return -(-cols // per), chunks(T, B)


def _strided_sums(v, stride):
    """v [rows, cols] fp32 -> [stride, cols]: row j is v[j] + v[j + stride] + .. added in order, from +0.0."""
    rows, cols = v.shape
    n = -(-rows // stride)
    pad = np.zeros((n * stride, cols), np.float32)
    pad[:rows] = v
    pad = pad.reshape(n, stride, cols)
    acc = np.zeros((stride, cols), np.float32)
    for k in range(n):
        live = min(stride, rows - k * stride)                # threads behind the last row add nothing
        acc[:live] = acc[:live] + pad[k, :live]
    return acc


def _chunk_partial(v):
    """The partial sums of one chunk: v [rows, cols] fp32 terms -> [cols]."""
    cols = v.shape[1]
    if cols >= WIDE_MIN:
        acc = _strided_sums(v, WIDE_ROWGROUPS)
        s = acc[0].copy()
        for k in range(1, WIDE_ROWGROUPS):
            s = s + acc[k]
        return s
    acc = _strided_sums(v, THREADS).reshape(THREADS // 64, 64, cols)
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, idx ^ m]
    s = acc[0, 0].copy()
    for w in range(1, THREADS // 64):
        s = s + acc[w, 0]
    return s


def colsum(a, x=None, R=None):
    """a, x: [T, B, cols] arrays (x or None); R: the row bound or None -> [cols] fp32, the kernels' bits."""
    a = np.asarray(a, np.float32)
    T, B, cols = a.shape
    R = T if R is None else min(max(int(R), 1), T)
    v = a[:R] if x is None else a[:R] * np.asarray(x, np.float32)[:R]        # fp32 products, rounded before they are added
    steps = chunk_steps(B)
    out = None
    for k in range(-(-R // steps)):
        p = _chunk_partial(v[k * steps:(k + 1) * steps].reshape(-1, cols))
        out = p if out is None else out + p
    return out


if __name__ == '__main__':
    T, B, cols = (int(s) for s in sys.argv[1:4])
    gx, gy = grid(T, B, cols)
    print(f'T {T} B {B} cols {cols}: {chunk_steps(B)} time steps per chunk, grid ({gx}, {gy}), '
          f'{"wide" if cols >= WIDE_MIN else "narrow"} kernel, scratch {scratch_bytes(T, B, cols)} bytes')
