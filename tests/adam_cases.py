"""Cases and the fp64 NumPy restatement of the device-resident Adam (include/dsp_frontend.h: dsp_adam_*; features/optim.py):
what tests/test_adam_host.py holds against ``torch.optim.Adam`` in fp64 and what the GPU tests compare the kernel with.

The update, per element, with t the step count after the increment (weight_decay 0, amsgrad off):
    m = b1 m + (1 - b1) g;   v = b2 v + (1 - b2) g^2;   p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
"""
import numpy as np

K_STEPS = 6
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
BAR = 2e-5                       # the project's bar between an fp32 route and fp64
HEADS = ['RNNHead', 'HRNNHead', 'HRNNAttHead', 'TransformerHead', 'HMRNNHead']


def lengths(C):
    """The smallest tensors, every numel % 4, the chunk boundary on both sides, several chunks with a tail."""
    return [1, 3, 4, 5, 63, 64, 1023, C - 1, C, C + 1, 3 * C + 7]


def head_numels(kind):
    """numel of every trainable parameter of one of the five heads, in ``parameters()`` order (built on the CPU)."""
    from features import classifier as C
    return [int(p.numel()) for p in getattr(C, kind)().parameters() if p.requires_grad]


def make_case(lens, seed=0, steps=K_STEPS):
    """-> (p0: list of fp32 arrays uniform in +-0.1; grads: [steps] lists of fp32 arrays, N(0,1) 10^k with k an integer uniform in
    -6 .. 1 per element, one element in ten exactly 0)."""
    rng = np.random.default_rng(seed)
    p0 = [rng.uniform(-0.1, 0.1, n).astype(np.float32) for n in lens]
    grads = []
    for _ in range(steps):
        row = []
        for n in lens:
            g = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2, n)
            g[rng.random(n) < 0.1] = 0.0
            row.append(g.astype(np.float32))
        grads.append(row)
    return p0, grads


def make_moments(lens, seed=1):
    """Moments to load a checkpoint from: m of either sign, v >= 0, both fp32."""
    rng = np.random.default_rng(seed)
    m = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    v = [(0.01 * rng.random(n)).astype(np.float32) for n in lens]
    return m, v


def adam_ref(p0, grads, lr=LR, betas=BETAS, eps=EPS, step0=0, m0=None, v0=None):
    """fp64 Adam over ``grads`` ([steps] lists of arrays) from (p0, m0, v0, step0) -> (p, m, v) lists of fp64 arrays.
    ``lr`` may be a list, one value per step."""
    b1, b2 = betas
    p = [np.asarray(a, dtype=np.float64).copy() for a in p0]
    m = [np.zeros_like(a) for a in p] if m0 is None else [np.asarray(a, dtype=np.float64).copy() for a in m0]
    v = [np.zeros_like(a) for a in p] if v0 is None else [np.asarray(a, dtype=np.float64).copy() for a in v0]
    for k, row in enumerate(grads):
        t = step0 + k + 1
        lr_k = lr[k] if isinstance(lr, (list, tuple)) else lr
        step_size = lr_k / (1.0 - b1 ** t)
        bc2_sqrt = np.sqrt(1.0 - b2 ** t)
        for i, g in enumerate(row):
            g = np.asarray(g, dtype=np.float64)
            m[i] = b1 * m[i] + (1.0 - b1) * g
            v[i] = b2 * v[i] + (1.0 - b2) * g * g
            p[i] = p[i] - step_size * (m[i] / (np.sqrt(v[i]) / bc2_sqrt + eps))
    return p, m, v


def flat(arrays):
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays])


def moment_err(got, ref):
    """max |got - ref| / max |ref| over all tensors of the case."""
    got, ref = flat(got), flat(ref)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def p_bound(p0, steps, lr=LR):
    """steps (2^-24 max|p0| + 2e-5 lr): one rounding of an fp32 parameter per step plus the project's bar on an update of size lr."""
    return steps * (2.0 ** -24 * float(np.max(np.abs(flat(p0)))) + BAR * lr)


def p_err(got, ref):
    return float(np.max(np.abs(flat(got) - flat(ref))))


def chunk_table(nat, numel):
    """``dsp_adam_chunk_table`` -> (tensor int32 [nc], offset int64 [nc]).  Needs no device."""
    import ctypes as C
    lib = nat.load()
    arr = np.ascontiguousarray(numel, dtype=np.int64)
    nc = C.c_int64(-1)
    assert lib.dsp_adam_chunk_table(len(arr), arr.ctypes.data, 0, None, None, C.byref(nc)) == nat.OK, lib.dsp_last_error()
    tensor, offset = np.full(nc.value + 1, -7, dtype=np.int32), np.full(nc.value + 1, -7, dtype=np.int64)
    n2 = C.c_int64(-1)
    assert lib.dsp_adam_chunk_table(len(arr), arr.ctypes.data, nc.value, tensor.ctypes.data, offset.ctypes.data, C.byref(n2)) == nat.OK
    assert n2.value == nc.value and tensor[-1] == -7 and offset[-1] == -7          # nothing behind the capacity is written
    return tensor[:-1], offset[:-1]
