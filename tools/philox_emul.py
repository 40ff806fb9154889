#!/usr/bin/env python3
"""The generator and the dropout launches of csrc/kernels_dropout.h restated in NumPy integer arithmetic, rule for rule: the
yardstick between the published algorithm and the device.

  Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw, SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key increments
  0x9E3779B9 / 0xBB67AE85, the key bumped between rounds.
  key = (seed_lo, seed_hi);  counter = (element_index // 4, step_lo, step_hi, site);  output word element_index % 4.
  kept iff (word >> 8) < thr,  thr = llrint((1 - p) 2^24) in double;  kept: x * float32(1 / (1 - p)),  dropped: +0.0.

``python tools/philox_emul.py`` prints the three known-answer vectors."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MAX_ELEMS = 1 << 34

# counter, key -> output (the published known-answer vectors of Philox4x32-10)
KNOWN_ANSWERS = (
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) that broadcast; key: two.  -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)              # 32 x 32 -> 64: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def keep_rule(p):
    """-> (thr, scale): the threshold of the 24-bit draw and the float32 factor of a kept element.  p in [0, 1)."""
    p = float(p)
    if not (0.0 <= p < 1.0):
        raise ValueError(f'p {p} must be in [0, 1)')
    return int(np.rint((1.0 - p) * 16777216.0)), np.float32(1.0 / (1.0 - p))


def words(n, seed, step, site, first=0):
    """The uint32 word of each element_index in [first, first + n)."""
    if n < 0 or first < 0 or first + n > MAX_ELEMS:
        raise ValueError('element indices must lie in [0, 2^34)')
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    idx = np.arange(first, first + n, dtype=np.int64)
    blocks = np.arange(first // 4, (first + n + 3) // 4, dtype=np.uint64)
    out = philox4x32_10((blocks, step & MASK32, step >> 32, int(site)), (seed & MASK32, seed >> 32))
    table = np.stack(out, axis=1).reshape(-1)                            # block-major, word-minor: element order
    return table[idx - 4 * (first // 4)]


def keep_mask(n, p, seed, step, site):
    """bool [n]: which elements are kept."""
    thr, _ = keep_rule(p)
    return (words(n, seed, step, site) >> np.uint32(8)) < np.uint32(min(thr, MASK32))


def apply(x, p, seed, step, site):
    """dsp_dropout_apply on the row-major elements of x (float32): the same shape.  p = 0 returns the input's bits."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    thr, scale = keep_rule(p)
    if thr >= 1 << 24:
        return x.copy()
    keep = keep_mask(x.size, p, seed, step, site).reshape(x.shape)
    return np.where(keep, x * scale, np.float32(0.0)).astype(np.float32)


def multipliers(L, T, B, C, p, seed, step, site_base, rows=None):
    """dsp_dropout_multipliers: float32 [L, T, B, C]; rows t >= clamp(rows, 1, T) are +0.0 (rows None: all T drawn)."""
    _, scale = keep_rule(p)
    R = T if rows is None else min(max(int(rows), 1), T)
    m = np.zeros((L, T, B, C), dtype=np.float32)
    for l in range(L):
        keep = keep_mask(R * B * C, p, seed, step, site_base + l).reshape(R, B, C)
        m[l, :R] = np.where(keep, scale, np.float32(0.0))
    return m


if __name__ == '__main__':
    for ctr, key, want in KNOWN_ANSWERS:
        got = tuple(int(v) for v in philox4x32_10(ctr, key))
        print(' '.join(f'{v:08x}' for v in got), 'ok' if got == want else 'MISMATCH')
