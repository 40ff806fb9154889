"""A float64 NumPy restatement of the cepstral pitch path, written from its arithmetic (test infrastructure, like
oracle/): the checker of the random GPU batches, itself checked against the stored reference outputs
(tests/test_pitch_cepstrum_host.py).

    decimate to 10 kHz -> rectangular frames of 512 / hop 100, zero padded
    per frame: clip at the median of the non-negative samples; y = conv(clipped, taps)[:L] with the complex taps of
               the 50 - 1000 Hz band; row = |ifft(log|fft(y)|)|
    rows smoothed in place over [i - 2, i + 2); per row 80 peak widths; first arg-max -> Hz; two octave-repair sweeps
    p from the frame amplitudes, the longest smooth run either side of p, two line fits, two parabola fits, a median shift
"""
import numpy as np


def decimate(sig, src_rate, dst_rate=10000):
    """keep sample i when i * dst / src first exceeds k - 1 + 1e-8, k = 0, 1, ..."""
    sig = np.asarray(sig)
    n = len(sig)
    if n == 0 or dst_rate >= src_rate:
        return sig
    vals = (np.arange(n, dtype=np.int64) * int(dst_rate)) / int(src_rate)
    ticks = np.arange(-1, int(np.floor(vals[-1])) + 1, dtype=np.float64) + 1e-8
    idx = np.searchsorted(vals, ticks, side='right')
    return sig[idx[idx < n]]


def frames_of(sig, L=512, S=100):
    sig = np.asarray(sig, dtype=np.float64)
    n = len(sig)
    T = 1 if n <= L else 1 + -(-(n - L) // S)
    pad = np.zeros((T - 1) * S + L)
    pad[:n] = sig
    return pad[np.arange(T)[:, None] * S + np.arange(L)[None, :]]


def taps(L, rate=10000, lo=50, hi=1000):
    Hd = np.zeros(L)
    Hd[int(L * lo / rate):int(L * hi / rate)] = 1
    return 2 * np.pi * np.hamming(L) * np.fft.ifft(Hd, L)


def clip_rows(F):
    """x - med above med, x + med below -med, 0 between; med = median of the non-negative samples of the row (NaN if none)."""
    out = np.zeros_like(F)
    for t, f in enumerate(F):
        pos = f[f >= 0]
        if len(pos) == 0:
            continue
        med = np.median(pos)
        out[t] = np.where(f > med, f - med, np.where(f < -med, f + med, 0.0))
    return out


def cepstrum_rows(F, clip=True):
    F = np.asarray(F, dtype=np.float64)
    T, L = F.shape
    C = clip_rows(F) if clip else F
    h = taps(L)
    y = np.fft.ifft(np.fft.fft(C, 2 * L, axis=1) * np.fft.fft(h, 2 * L)[None, :], axis=1)[:, :L]   # linear convolution, truncated
    y[np.all(C == 0, axis=1)] = 0                                                                   # an exact zero stays one
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.abs(np.fft.ifft(np.log(np.abs(np.fft.fft(y, axis=1))), axis=1))


def smooth_rows(rows):
    g = np.array(rows, dtype=np.float64)
    T = len(g)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(T):
            left, right = max(i - 2, 0), (i + 2 if i + 2 < T else T - 1)
            acc = np.zeros(g.shape[1])
            for r in range(left, right):
                acc = acc + g[r] if r > left else g[r].copy()
            g[i] = acc / (right - left) if right > left else np.nan
    return g


def peak_scores(rows, lo=20, hi=100):
    """[T, 80] int: min(distance to the nearest larger value below i, not looking at column 0; the same above i, the
    row's end counting as larger).  A NaN at i scores 0."""
    rows = np.asarray(rows, dtype=np.float64)
    T, L = rows.shape
    out = np.zeros((T, hi - lo), dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for i in range(lo, hi):
            v = rows[:, i:i + 1]
            stop_l = ~(rows[:, 1:i] <= v)                            # columns 1 .. i - 1
            p = np.where(stop_l.any(axis=1), i - 1 - np.argmax(stop_l[:, ::-1], axis=1), 0)
            stop_r = ~(rows[:, i + 1:] <= v)
            q = np.where(stop_r.any(axis=1), i + 1 + np.argmax(stop_r, axis=1), L)
            s = np.minimum(i - p, q - i)
            s[~(v[:, 0] <= v[:, 0])] = 0
            out[:, i - lo] = s
    return out


def robust_track(scores, bias=20):
    pitch = 1 / (0.0001 * (bias + np.argmax(scores, axis=1)))
    for i in range(1, len(pitch)):
        if abs(2 * pitch[i] - pitch[i - 1]) < 50 and pitch[i] < 170:
            pitch[i] = 2 * pitch[i]
    for i in range(len(pitch) - 2, 0, -1):
        if abs(2 * pitch[i] - pitch[i + 1]) < 50 and pitch[i] < 170:
            pitch[i] = 2 * pitch[i]
    return pitch


def sub_endpoint(amp):
    amp = np.asarray(amp, dtype=np.float64)
    T = len(amp)
    idx = np.arange(10, T - 10)
    if len(idx) == 0:
        return T // 2
    near = amp[idx[:, None] + np.arange(-2, 3)[None, :]]
    ok = ~(near < amp[idx][:, None]).any(axis=1)
    D = amp[idx[:, None] + np.arange(-10, 11)[None, :]] - amp[idx][:, None]
    s = np.zeros(len(idx))
    for k in range(21):                                               # in order, as a running sum
        s = s + D[:, k]
    s = np.where(ok & (s > -1000), s, -np.inf)
    if not np.isfinite(s).any():
        return T // 2
    return int(idx[np.argmax(s)])


def smooth_subsequence(v, tor=3, thres=30.0):
    """-> (accepted values, start, end) of the longest run (the first on a tie); a run accepts values within `thres` of
    the last accepted one and ends at its `tor`-th rejection or at the end; the next run starts tor - 1 before that."""
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    best = ([], 0, 0)
    i = 0
    while i < n:
        acc, prev, left, j = [v[i]], v[i], tor, i + 1
        while j < n:
            if abs(v[j] - prev) > thres:
                left -= 1
                if left == 0:
                    break
            else:
                acc.append(v[j])
                prev = v[j]
            j += 1
        if len(acc) > len(best[0]):
            best = (acc, i, j)
        if j == n:
            break
        i = j - tor + 1
    return best


def features_of(pitch, amp):
    """-> dict(p, p_bias, seg1, idx1, seg2, idx2, feat, valid)"""
    pitch = np.asarray(pitch, dtype=np.float64)
    p = sub_endpoint(amp)
    p_bias = 5 if p > 15 else 0
    s1, a1, b1 = smooth_subsequence(pitch[p_bias:p])
    s2, a2, b2 = smooth_subsequence(pitch[p:])
    valid = len(s1) >= 3 and len(s2) >= 3
    feat = np.full(5, np.nan)
    if valid:
        x1, x2 = np.arange(len(s1)), np.arange(len(s2))
        feat = np.array([np.polyfit(x1, s1, 1)[0], np.polyfit(x2, s2, 1)[0], np.polyfit(x1, s1, 2)[0],
                         np.polyfit(x2, s2, 2)[0], np.median(s2) - np.median(s1)])
    return dict(p=p, p_bias=p_bias, seg1=np.array(s1), idx1=(a1 + p_bias, b1 + p_bias), seg2=np.array(s2),
                idx2=(a2 + p, b2 + p), feat=feat, valid=valid)


def full(sig, rate, L=512, S=100):
    """The whole path for one clip -> dict(rows, amp, scores, pitch, + features_of)."""
    s = decimate(np.asarray(sig).reshape(-1), rate)
    F = frames_of(s, L, S)
    rows = cepstrum_rows(F)
    scores = peak_scores(smooth_rows(rows))
    pitch = robust_track(scores)
    amp = np.abs(F).sum(axis=1)
    out = dict(rows=rows, amp=amp, scores=scores, pitch=pitch)
    out.update(features_of(pitch, amp))
    return out
