"""``DeviceAdam``: the optimiser step of model.py:140-149 (``torch.optim.Adam(self.clf.parameters(), lr=lr)``, weight_decay 0,
amsgrad off) as native launches whose whole state -- moments, step count, hyper-parameters, pointer tables -- lives on the
device (csrc/kernels_optim.h, ``dsp_adam_*``).  A step is two launches on torch's current stream for ALL parameters, reads
nothing from the host and synchronises nothing, so it can be recorded: ``TrainBatch.capture(..., optimizer=opt)`` puts it behind
the backward, and ``set_lr`` between replays (model.py:231-234: ``lr *= 0.8`` / ``lr *= 0.5``) needs no re-capture.

One step counter is shared by all parameters (torch keeps one per parameter and skips a parameter without a gradient; every
parameter of every head gets a gradient, so ``step()`` refuses a missing ``.grad`` instead).  ``state_dict`` /
``load_state_dict`` speak ``torch.optim.Adam``'s layout for one parameter group, so a checkpoint moves between the two
optimisers in both directions.  There is no fallback: without the library or a GPU the constructor raises.
"""
from __future__ import annotations

from . import _native as nat


def _increment_version(tensors):
    import torch
    for t in tensors:
        torch.autograd.graph.increment_version(t)


class DeviceAdam:
    """``DeviceAdam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)``: ``params`` contiguous fp32 CUDA tensors on one device.
    ``exp_avg`` / ``exp_avg_sq`` are torch tensors this object owns, in the order of ``params``.  ``lr``, ``betas`` and ``eps``
    are host mirrors of what the device holds (``set_lr`` and ``load_state_dict`` keep them equal)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        import torch
        params = list(params)
        if not params:
            raise ValueError('DeviceAdam: no parameters')
        for i, p in enumerate(params):
            if not torch.is_tensor(p):
                raise TypeError(f'DeviceAdam: parameter {i} is a {type(p).__name__}, not a tensor')
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.numel() < 1:
                raise ValueError(f'DeviceAdam: parameter {i} ({p.dtype}, {p.device}, contiguous={p.is_contiguous()}, {p.numel()} elements) '
                                 'must be a non-empty contiguous float32 CUDA tensor')
            if p.device != params[0].device:
                raise ValueError(f'DeviceAdam: parameter {i} is on {p.device}, parameter 0 on {params[0].device}: one device only')
        if len({id(p) for p in params}) != len(params):
            raise ValueError('DeviceAdam: a parameter appears twice')
        nat.require_device()
        self.params, self.device = params, params[0].device
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in params]
        self._bound = None                                     # the gradient addresses the device table holds
        self._handle = None
        n = len(params)
        numel = (nat.c_i64 * n)(*[p.numel() for p in params])
        h = nat.c_vp(0)
        with torch.cuda.device(self.device):                   # (the handle belongs to the parameters' device)
            nat.check_value(nat.load().dsp_adam_create(n, numel, self._ptrs(params), self._ptrs(self.exp_avg), self._ptrs(self.exp_avg_sq),
                                                       self.lr, self.betas[0], self.betas[1], self.eps, nat.C.byref(h)), 'dsp_adam_create')
        self._handle = h.value

    @staticmethod
    def _ptrs(tensors):
        return (nat.c_vp * len(tensors))(*[t.data_ptr() for t in tensors])

    def __del__(self):
        if getattr(self, '_handle', None) is not None:
            try:                                               # (at interpreter shutdown even the import may fail)
                nat.load().dsp_adam_destroy(self._handle)
            except Exception:
                pass
            self._handle = None

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- the step ---------------------------------------------------------------------------------------------------
    def _check_grads(self, grads):
        import torch
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                raise RuntimeError(f'DeviceAdam.step: parameter {i} has no gradient (.grad is None): one step counter serves all parameters, '
                                   'none is skipped')
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                raise ValueError(f'DeviceAdam.step: the gradient of parameter {i} ({g.dtype}, {g.device}, {tuple(g.shape)}, '
                                 f'contiguous={g.is_contiguous()}) must be a contiguous float32 tensor of the parameter\'s shape and device')

    def _launch(self, grads, zero_grads, rebind='changed'):
        """Bind (``rebind='changed'``: only where an address differs from the table's; ``'always'``: a recorded sequence carries
        its own binding) and step, on torch's current stream."""
        import torch
        self._check_grads(grads)
        ptrs = tuple(g.data_ptr() for g in grads)
        lib = nat.load()
        with torch.cuda.device(self.device):
            st = self._stream()
            if rebind == 'always' or ptrs != self._bound:
                nat.check_value(lib.dsp_adam_bind_grads(self._handle, (nat.c_vp * len(ptrs))(*ptrs), st), 'dsp_adam_bind_grads')
                self._bound = ptrs
            nat.check_value(lib.dsp_adam_step(self._handle, 1 if zero_grads else 0, st), 'dsp_adam_step')

    def step(self, zero_grads=False):
        """One Adam step on the parameters' ``.grad``s, on torch's current stream; nothing is synchronised.  The gradient
        addresses are uploaded only when one changed since the last bind.  ``zero_grads=True``: the same launch writes
        ``+0.0`` over every gradient after reading it (``zero_grad(set_to_none=False)``, fused).  Afterwards the parameters'
        version counters are bumped, so that the native handles of the modules that own them repack on their next use."""
        grads = [p.grad for p in self.params]
        self._launch(grads, zero_grads)
        _increment_version(self.params)
        if zero_grads:
            _increment_version(grads)

    def _after_replay(self, grads):
        """A graph that recorded ``_launch(grads, False, 'always')`` has run: the table holds its addresses, the parameters were written."""
        self._bound = tuple(g.data_ptr() for g in grads)
        _increment_version(self.params)

    def zero_grad(self, set_to_none=True):
        """``torch.optim.Optimizer.zero_grad``."""
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()

    # ---- hyper-parameters and state ---------------------------------------------------------------------------------
    def _set_hyper(self, lr, betas, eps):
        import torch
        with torch.cuda.device(self.device):
            nat.check_value(nat.load().dsp_adam_set_hyper(self._handle, float(lr), float(betas[0]), float(betas[1]), float(eps), self._stream()),
                            'dsp_adam_set_hyper')
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)

    def set_lr(self, lr):
        """The learning rate of every later step, recorded ones included: one launch on the current stream that writes the
        device's copy, nothing else but this object's mirror."""
        self._set_hyper(lr, self.betas, self.eps)

    def reset(self):
        """A fresh Adam in place (model.py:140 makes a new one every epoch; a recorded step is bound to this one): the step
        count to 0 and both moments to zero, on the current stream.  Addresses, hyper-parameters and the gradient binding stay,
        so a recorded step goes on replaying, and the next step equals the first step of a new ``DeviceAdam``."""
        import torch
        with torch.cuda.device(self.device):
            nat.check_value(nat.load().dsp_adam_set_step(self._handle, 0, self._stream()), 'dsp_adam_set_step')
        with torch.no_grad():
            torch._foreach_zero_(self.exp_avg + self.exp_avg_sq)

    def device_state(self):
        """-> (step, lr, beta1, beta2, eps) as the device holds them.  Synchronises the current stream."""
        import torch
        step, hyper = nat.c_i64(0), (nat.c_f64 * 4)()
        with torch.cuda.device(self.device):
            nat.check(nat.load().dsp_adam_get_state(self._handle, nat.C.byref(step), hyper, self._stream()))
        return (step.value,) + tuple(hyper)

    def state_dict(self):
        """``torch.optim.Adam``'s state dict for one parameter group: per parameter ``step`` (a float32 scalar tensor, as torch
        keeps it), ``exp_avg`` and ``exp_avg_sq`` (copies); the group's keys are those the installed torch's Adam writes.
        Synchronises the current stream (the step count is read from the device)."""
        import torch
        step = self.device_state()[0]
        group = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps).state_dict()['param_groups'][0]
        group['params'] = list(range(len(self.params)))
        state = {}
        if step > 0:                                           # (torch's Adam has no state before its first step)
            for i, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq)):
                state[i] = {'step': torch.tensor(float(step), dtype=torch.float32), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        """A state dict of ``torch.optim.Adam`` (or of this class) over the same parameters, one group.  Refuses what this
        optimiser does not do (weight decay, amsgrad, maximize) and per-parameter steps that differ."""
        import torch
        groups = sd['param_groups']
        if len(groups) != 1:
            raise ValueError(f'DeviceAdam.load_state_dict: {len(groups)} parameter groups; one is served')
        grp = groups[0]
        if len(grp['params']) != len(self.params):
            raise ValueError(f'DeviceAdam.load_state_dict: the group has {len(grp["params"])} parameters, this optimiser {len(self.params)}')
        if grp.get('weight_decay', 0) != 0 or grp.get('amsgrad', False) or grp.get('maximize', False):
            raise ValueError('DeviceAdam.load_state_dict: weight_decay, amsgrad and maximize are not served')
        state = sd['state']
        entries = [state.get(k) for k in grp['params']]
        if any(e is None for e in entries) and any(e is not None for e in entries):
            raise ValueError('DeviceAdam.load_state_dict: some parameters have state and some have none: one step counter serves all')
        steps = {int(round(float(e['step']))) for e in entries if e is not None} or {0}
        if len(steps) != 1:
            raise ValueError(f'DeviceAdam.load_state_dict: the parameters\' steps differ ({sorted(steps)}): one step counter serves all')
        for e, m, v in zip(entries, self.exp_avg, self.exp_avg_sq):
            if e is not None and (tuple(e['exp_avg'].shape) != tuple(m.shape) or tuple(e['exp_avg_sq'].shape) != tuple(v.shape)):
                raise ValueError('DeviceAdam.load_state_dict: a moment tensor has another shape than its parameter')
        self._set_hyper(grp['lr'], grp['betas'], grp['eps'])
        with torch.no_grad():
            for e, m, v in zip(entries, self.exp_avg, self.exp_avg_sq):
                if e is None:
                    m.zero_()
                    v.zero_()
                else:
                    m.copy_(e['exp_avg'])
                    v.copy_(e['exp_avg_sq'])
        with torch.cuda.device(self.device):
            nat.check_value(nat.load().dsp_adam_set_step(self._handle, steps.pop(), self._stream()), 'dsp_adam_set_step')
