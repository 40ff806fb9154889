"""The products behind the GRU and HM-LSTM backward recurrences as native launches bounded by a row count read on the device
(include/dsp_frontend.h: dsp_rows_wgrad, dsp_rows_product; csrc/kernels_wgrad.h).

``classifier.gru_param_grads`` / ``classifier.hm_param_grads`` are torch: GEMMs and column sums over all T B rows of buffers whose
shapes the host fixed, plus the ``torch.cat`` copies that build their time-shifted operands.  Here the same arguments become a
PLAN -- a list of products whose operands are plain Python data: which buffer, an offset, a t stride and a b stride in floats,
a column count, a shift in time, an initial row, a row scale, the output each feeds.  Building a plan touches no device memory
(strides are host metadata; the few tensors it makes -- the permuted ``w_ih``, the [T, B] scale, the transposed initial rows --
are ordinary stream-ordered torch calls).  ``run_plan`` launches it; ``Plan.finish`` is what stays torch on small tensors: the
``r | z | n`` row permutation of the [3 H, .] results and ``dx * drop``.

tests/wgrad_cases.py holds a NumPy fp64 interpreter of a plan that uses the descriptors and nothing else.
"""
import torch


def operand(buf, offset, stride_t, stride_b, cols):
    """One [T, B, cols] view of the flat buffer ``buf``: element (t, b, c) at offset + t stride_t + b stride_b + c (floats)."""
    return dict(buf=buf, offset=int(offset), stride_t=int(stride_t), stride_b=int(stride_b), cols=int(cols))


class Plan:
    """T, B; ``buffers``: name -> contiguous tensor; ``products``: the list of products (dicts, below); ``outputs``: name -> shape
    of every tensor the products write; ``finish(outs)`` -> the tuple ``gru_param_grads`` / ``hm_param_grads`` return.

    A product is one of
      dict(kind='wgrad', a=operand, x=operand, shift=-1 | 0 | 1, init=None | dict(buf, offset, stride_b), scale=None | dict(buf, offset),
           out=name | None, colsum=name | None)
          out [a.cols, x.cols] = sum_{t < R, b} scale[t, b] a[t, b, :]^T (x) xs[t, b, :], xs the rows of x shifted in time (the
          initial row, or zeros, in front of t = 0; zeros from R on); colsum [a.cols] = sum_{t < R, b} a[t, b, :], unscaled.
          ``out`` None: only the column sums are wanted (the product is formed and dropped).
      dict(kind='product', terms=[(operand, dict(buf, offset)), ..], n=columns, out=name)
          out [T, B, n] = sum over the terms of a[t, b, :] @ w [a.cols, n] for t < R, zeros behind."""

    def __init__(self, T, B):
        self.T, self.B = int(T), int(B)
        self.buffers, self.products, self.outputs = {}, [], {}
        self.finish = None

    def wgrad(self, a, x, shift=0, init=None, scale=None, out=None, colsum=None):
        self.products.append(dict(kind='wgrad', a=a, x=x, shift=shift, init=init, scale=scale, out=out, colsum=colsum))
        if out is not None:
            self.outputs[out] = (a['cols'], x['cols'])
        if colsum is not None:
            self.outputs[colsum] = (a['cols'],)

    def product(self, terms, n, out):
        self.products.append(dict(kind='product', terms=terms, n=int(n), out=out))
        self.outputs[out] = (self.T, self.B, int(n))


def gru_wgrad_plan(params, x, out, da, drop=None, need=None):
    """The arguments of ``classifier.gru_param_grads`` (one layer: params = weight_ih, weight_hh, bias_ih, bias_hh of the forward
    direction, then of the reverse one; x [T, B, in]; out [T, B, 2 H]; da [T, B, 2, 4 H] = n_x | r | z | n_h; drop or None;
    ``need``: 9 booleans) -> the Plan of its products.  The hidden-state operand of the recurrent weights is ``out`` itself,
    shifted: t - 1 for the forward direction, t + 1 for the reverse one; a row outside [0, R) is zero, which is what
    ``torch.cat([out[1:], zero])`` reads on a buffer whose rows behind each column's end are zero."""
    T, B, I = x.shape
    H = out.shape[2] // 2
    need = [True] * 9 if need is None else list(need)
    plan = Plan(T, B)
    plan.buffers.update(x=x.contiguous(), out=out.contiguous(), da=da.contiguous())
    xo = operand('x', 0, B * I, I, I)
    terms = []
    for d in (0, 1):
        a_ih = operand('da', d * 4 * H, B * 8 * H, 8 * H, 3 * H)              # n_x | r | z
        a_hh = operand('da', d * 4 * H + H, B * 8 * H, 8 * H, 3 * H)          # r | z | n_h
        if need[0]:
            w_ih = params[4 * d]
            plan.buffers[f'w{d}'] = torch.cat([w_ih[2 * H:], w_ih[:2 * H]], 0).contiguous()        # rows n | r | z, as a_ih's columns
            terms.append((a_ih, dict(buf=f'w{d}', offset=0)))
        if need[1 + 4 * d] or need[3 + 4 * d]:
            plan.wgrad(a_ih, xo, out=f'w_ih{d}' if need[1 + 4 * d] else None, colsum=f'b_ih{d}' if need[3 + 4 * d] else None)
        if need[2 + 4 * d] or need[4 + 4 * d]:
            plan.wgrad(a_hh, operand('out', d * H, B * 2 * H, 2 * H, H), shift=-1 if d == 0 else 1,
                       out=f'w_hh{d}' if need[2 + 4 * d] else None, colsum=f'b_hh{d}' if need[4 + 4 * d] else None)
    if need[0]:
        plan.product(terms, I, 'dx')
    rzn = lambda v: torch.cat([v[H:], v[:H]], 0)            # rows n | r | z -> nn.GRU's r | z | n

    def finish(outs):
        res = [None] * 9
        for d in (0, 1):
            if need[1 + 4 * d]: res[1 + 4 * d] = rzn(outs[f'w_ih{d}'])
            if need[2 + 4 * d]: res[2 + 4 * d] = outs[f'w_hh{d}']
            if need[3 + 4 * d]: res[3 + 4 * d] = rzn(outs[f'b_ih{d}'])
            if need[4 + 4 * d]: res[4 + 4 * d] = outs[f'b_hh{d}']
        if need[0]:
            res[0] = outs['dx'] * drop if drop is not None else outs['dx']
        return tuple(res)
    plan.finish = finish
    return plan


def hm_wgrad_plan(params, x, state_in, h_1, h_2, z_1, dfs1, dfs2, need=None):
    """The arguments of ``classifier.hm_param_grads`` (params = U_11, U_21, W_01, bias of cell 1, U_11, W_01, bias of cell 2;
    x [T, B, I]; state_in: the flat h1 | c1 | z1 | h2 | c2 | z2 buffer or None; h_1 [B, T, H1], h_2 [B, T, H2], z_1 [B, T];
    dfs1 [T, B, 4 H1 + 1], dfs2 [T, B, 4 H2 + 1]; ``need``: 8 booleans) -> the Plan of its products.  h_1 and h_2 are read in
    their [B, T, H] layout through the strides; the initial rows h1_0 / h2_0 ([H, B] slabs of state_in) are transposed to
    [B, H] here (B H floats each), and the row scales z1 and z1 shifted by one step are built here as [T, B] tensors."""
    T, B, I = x.shape
    H1, H2 = h_1.shape[2], h_2.shape[2]
    need = [True] * 8 if need is None else list(need)
    dt = dfs1.dtype
    plan = Plan(T, B)
    plan.buffers.update(x=x.contiguous(), h1=h_1.contiguous(), h2=h_2.contiguous(), dfs1=dfs1.contiguous(), dfs2=dfs2.contiguous())
    init1 = init2 = None
    z1 = z_1.to(dt).t()                                                          # [T, B]
    if state_in is None:
        z1_0 = dfs1.new_zeros(1, B)
    else:
        plan.buffers['h1_0'] = state_in[:H1 * B].view(H1, B).t().to(dt).contiguous()
        plan.buffers['h2_0'] = state_in[(2 * H1 + 1) * B:(2 * H1 + 1 + H2) * B].view(H2, B).t().to(dt).contiguous()
        init1, init2 = dict(buf='h1_0', offset=0, stride_b=H1), dict(buf='h2_0', offset=0, stride_b=H2)
        z1_0 = state_in[2 * H1 * B:(2 * H1 + 1) * B].view(1, B).to(dt)
    if need[2]:
        plan.buffers['z1p'] = torch.cat([z1_0, z1[:-1]], 0).contiguous()
    if need[5]:
        plan.buffers['z1'] = z1.contiguous()
    d1, d2 = operand('dfs1', 0, B * (4 * H1 + 1), 4 * H1 + 1, 4 * H1 + 1), operand('dfs2', 0, B * (4 * H2 + 1), 4 * H2 + 1, 4 * H2 + 1)
    h1o, h2o = operand('h1', 0, H1, T * H1, H1), operand('h2', 0, H2, T * H2, H2)
    xo = operand('x', 0, B * I, I, I)
    if need[0]:
        plan.buffers['W01'] = params[2].contiguous()
        plan.product([(d1, dict(buf='W01', offset=0))], I, 'dx')
    # the column sums ride on the first product over the same rows; alone, they take the narrowest one
    first1 = 1 if need[1] else 2 if need[2] else 3
    first2 = 5 if need[5] else 6
    c1 = lambda k: 'b1' if need[4] and k == first1 else None
    c2 = lambda k: 'b2' if need[7] and k == first2 else None
    if need[1]: plan.wgrad(d1, h1o, shift=-1, init=init1, out='U11_1', colsum=c1(1))
    if need[2]: plan.wgrad(d1, h2o, shift=-1, init=init2, scale=dict(buf='z1p', offset=0), out='U21', colsum=c1(2))
    if need[3] or c1(3): plan.wgrad(d1, xo, out='W01_1' if need[3] else None, colsum=c1(3))
    if need[5]: plan.wgrad(d2, h2o, shift=-1, init=init2, scale=dict(buf='z1', offset=0), out='U11_2', colsum=c2(5))
    if need[6] or c2(6): plan.wgrad(d2, h1o, out='W01_2' if need[6] else None, colsum=c2(6))
    names = ('dx', 'U11_1', 'U21', 'W01_1', 'b1', 'U11_2', 'W01_2', 'b2')
    plan.finish = lambda outs: tuple(outs[n] if need[k] else None for k, n in enumerate(names))
    return plan


def _c_operand(nat, plan, op):
    t = plan.buffers[op['buf']]
    return nat.RowsOperand(t.data_ptr() + 4 * op['offset'], op['stride_t'], op['stride_b'], op['cols'], 0)


def _addr(plan, ref):
    return None if ref is None else plan.buffers[ref['buf']].data_ptr() + 4 * ref['offset']


def run_plan(plan, d_rows, stream):
    """Launch every product of ``plan`` on ``stream`` (a raw HIP stream, the one the buffers' producers ran on) -> name -> tensor
    for every output.  ``d_rows``: a one-element int32 tensor on the buffers' device, the row bound R = clamp(d_rows[0], 1, T)
    read when the kernels run, or None for R = T.  Nothing is read back or synchronised; outputs and scratch come from torch's
    allocator, so the call can be captured."""
    from . import _native as nat
    lib = nat.load()
    T, B = plan.T, plan.B
    some = next(iter(plan.buffers.values()))
    dev = some.device
    if not some.is_cuda:
        raise RuntimeError('run_plan: the buffers are not on a GPU')
    for name, t in plan.buffers.items():
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise TypeError(f'run_plan: buffer {name} must be a contiguous float32 tensor on {dev}')
    if d_rows is not None and not (torch.is_tensor(d_rows) and d_rows.dtype == torch.int32 and d_rows.numel() == 1 and d_rows.device == dev):
        raise TypeError("run_plan: d_rows must be a one-element int32 tensor on the buffers' device")
    rows = None if d_rows is None else d_rows.data_ptr()
    f32 = dict(dtype=torch.float32, device=dev)
    outs = {name: torch.empty(*shape, **f32) for name, shape in plan.outputs.items()}
    nbytes, worst = nat.c_i64(0), 0
    for p in plan.products:
        if p['kind'] == 'wgrad':
            nat.check(lib.dsp_rows_wgrad_scratch_bytes(T, B, p['a']['cols'], p['x']['cols'], nat.C.byref(nbytes)))
            worst = max(worst, nbytes.value)
    scratch = torch.empty(worst // 4, **f32) if worst else None             # one buffer: the launches run in stream order
    for p in plan.products:
        if p['kind'] == 'wgrad':
            a, x = _c_operand(nat, plan, p['a']), _c_operand(nat, plan, p['x'])
            c = outs[p['out']] if p['out'] is not None else torch.empty(p['a']['cols'], p['x']['cols'], **f32)
            nat.check(lib.dsp_rows_wgrad(nat.C.byref(a), nat.C.byref(x), p['shift'], _addr(plan, p['init']),
                                         p['init']['stride_b'] if p['init'] is not None else 0, _addr(plan, p['scale']), T, B, rows,
                                         c.data_ptr(), outs[p['colsum']].data_ptr() if p['colsum'] is not None else None,
                                         scratch.data_ptr(), worst, stream))
        else:
            ops = [_c_operand(nat, plan, a) for a, _ in p['terms']]
            ws = [_addr(plan, w) for _, w in p['terms']]
            assert 1 <= len(ops) <= 2, 'a row product sums one or two terms'
            nat.check(lib.dsp_rows_product(nat.C.byref(ops[0]), ws[0], nat.C.byref(ops[1]) if len(ops) > 1 else None,
                                           ws[1] if len(ops) > 1 else None, p['n'], T, B, rows, outs[p['out']].data_ptr(), stream))
    return outs


def gru_param_grads_native(params, x, out, da, drop=None, need=None, d_rows=None):
    """``classifier.gru_param_grads`` through the native launches, on torch's current stream."""
    plan = gru_wgrad_plan(params, x, out, da, drop, need)
    return plan.finish(run_plan(plan, d_rows, torch.cuda.current_stream(x.device).cuda_stream))


def hm_param_grads_native(params, x, state_in, h_1, h_2, z_1, dfs1, dfs2, need=None, d_rows=None):
    """``classifier.hm_param_grads`` through the native launches, on torch's current stream."""
    plan = hm_wgrad_plan(params, x, state_in, h_1, h_2, z_1, dfs1, dfs2, need)
    return plan.finish(run_plan(plan, d_rows, torch.cuda.current_stream(x.device).cuda_stream))


def rows_colsum(a, x=None, d_rows=None):
    """``sum_{t < R, b} a[t, b, :] * (x[t, b, :] if x is given else 1)`` as the two native launches of ``dsp_rows_colsum``
    (include/dsp_frontend.h; csrc/kernels_reduce.h) on torch's current stream -> a new [cols] tensor.

    ``a`` (and ``x``, of the same shape): a float32 device tensor [T, B, cols] read through its strides -- any view with a unit
    column stride is read where it lies (``da[:, :, d, :n]``), any other is copied first; a [B, cols] tensor is T = 1 and a
    [T, B] tensor of scalars is ``a.unsqueeze(2)``.  ``d_rows``: a one-element int32 tensor on the same device, the row bound
    R = clamp(d_rows[0], 1, T) read when the kernels run (rows behind it are never read), or None for R = T.  fp32 in a fixed
    order: the same bits on every run; no atomics, no memset, nothing read back or synchronised, so the call can be captured.
    The result and the scratch come from torch's allocator."""
    from . import _native as nat
    lib = nat.load()
    for name, t in (('a', a), ('x', x)):
        if t is None:
            continue
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
            raise TypeError(f'rows_colsum: {name} must be a float32 device tensor [T, B, cols]')
    if x is not None and (x.shape != a.shape or x.device != a.device):
        raise ValueError(f'rows_colsum: x {tuple(x.shape)} on {x.device} does not match a {tuple(a.shape)} on {a.device}')
    if d_rows is not None and not (torch.is_tensor(d_rows) and d_rows.dtype == torch.int32 and d_rows.numel() == 1 and d_rows.device == a.device):
        raise TypeError("rows_colsum: d_rows must be a one-element int32 tensor on a's device")
    a, x = _rows_view(a), None if x is None else _rows_view(x)
    T, B, cols = a.shape
    nbytes = nat.c_i64(0)
    nat.check_value(lib.dsp_rows_colsum_scratch_bytes(T, B, cols, nat.C.byref(nbytes)), 'rows_colsum: invalid sizes')
    out = torch.empty(cols, dtype=torch.float32, device=a.device)
    scratch = torch.empty(nbytes.value // 4, dtype=torch.float32, device=a.device)
    op = lambda t: nat.RowsOperand(t.data_ptr(), t.stride(0), t.stride(1), cols, 0)
    oa, ox = op(a), None if x is None else op(x)
    with torch.cuda.device(a.device):
        nat.check_value(lib.dsp_rows_colsum(nat.C.byref(oa), None if ox is None else nat.C.byref(ox), T, B,
                                            None if d_rows is None else d_rows.data_ptr(), out.data_ptr(), scratch.data_ptr(),
                                            nbytes.value, torch.cuda.current_stream(a.device).cuda_stream), 'rows_colsum: invalid argument')
    return out


def _rows_view(t):
    """A [T, B, cols] float32 device tensor as the launches read it: itself where its column stride is 1, else a copy."""
    return t if t.shape[2] == 1 or t.stride(2) == 1 else t.contiguous()


def rows_gemm(a, x, d_rows=None, colsum=False):
    """``a^T x`` over the rows: a [T, B, m], x [T, B, n] -> [m, n] = sum_{t < R, b} a[t, b, :]^T (x) x[t, b, :] as the two launches
    of ``dsp_rows_wgrad`` (no shift, no scale) on torch's current stream; with ``colsum`` also a's column sums [m] from the same
    launches -> (product, sums).  The operands are read through their strides (``rows_colsum`` has the rules); ``d_rows`` as
    there.  ``nn.Linear``'s dW / db is ``rows_gemm(g.unsqueeze(0), feat.unsqueeze(0), colsum=True)``."""
    from . import _native as nat
    lib = nat.load()
    for name, t in (('a', a), ('x', x)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
            raise TypeError(f'rows_gemm: {name} must be a float32 device tensor [T, B, cols]')
    if x.shape[:2] != a.shape[:2] or x.device != a.device:
        raise ValueError(f'rows_gemm: x {tuple(x.shape)} on {x.device} does not match a {tuple(a.shape)} on {a.device}')
    if d_rows is not None and not (torch.is_tensor(d_rows) and d_rows.dtype == torch.int32 and d_rows.numel() == 1 and d_rows.device == a.device):
        raise TypeError("rows_gemm: d_rows must be a one-element int32 tensor on a's device")
    a, x = _rows_view(a), _rows_view(x)
    T, B, m = a.shape
    n = x.shape[2]
    f32 = dict(dtype=torch.float32, device=a.device)
    nbytes = nat.c_i64(0)
    nat.check_value(lib.dsp_rows_wgrad_scratch_bytes(T, B, m, n, nat.C.byref(nbytes)), 'rows_gemm: invalid sizes')
    c, cs = torch.empty(m, n, **f32), torch.empty(m, **f32) if colsum else None
    scratch = torch.empty(nbytes.value // 4, **f32)
    oa, ox = nat.RowsOperand(a.data_ptr(), a.stride(0), a.stride(1), m, 0), nat.RowsOperand(x.data_ptr(), x.stride(0), x.stride(1), n, 0)
    with torch.cuda.device(a.device):
        nat.check_value(lib.dsp_rows_wgrad(nat.C.byref(oa), nat.C.byref(ox), 0, None, 0, None, T, B, None if d_rows is None else d_rows.data_ptr(),
                                           c.data_ptr(), None if cs is None else cs.data_ptr(), scratch.data_ptr(), nbytes.value,
                                           torch.cuda.current_stream(a.device).cuda_stream), 'rows_gemm: invalid argument')
    return (c, cs) if colsum else c
