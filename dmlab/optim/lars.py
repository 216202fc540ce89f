"""LARS (layer-wise adaptive rate scaling, You et al. 2017) and its warm-up + polynomial
learning-rate schedule: the large-batch recipe for the data-parallel ResNet workload.

Per step, for every parameter tensor with weights ``w``, raw gradient ``g`` and momentum
buffer ``b`` (zero-initialised; there is no first-step special case)::

    g'  = c * grad_scale * g                       # c = 1 unless clipping
    adapted:   r = eta*|w| / (|g'| + wd*|w| + eps)  if |w| > 0 and |g'| > 0 else 1
               d = r * (g' + wd*w)
    otherwise: d = g'                               # r = 1, no weight decay
    b   = mu*b + d
    w  -= lr * (d + mu*b  if nesterov else  b)

``exclude_1d`` (default) leaves every parameter with ``ndim <= 1`` (BatchNorm scale and
shift, biases) non-adapted.  With ``max_grad_norm``, ``c = min(1, max_grad_norm / (G + 1e-6))``
where ``G`` is the L2 norm of ``grad_scale * g`` over all tensors (``clip_grad_norm_``
followed by LARS).

When the parameters are exactly one :class:`~dmlab.nn.flat.FlatParams` on a HIP device the
step is three launches of ``csrc/lars.hip`` whatever the number of tensors; the learning
rate lives in a small device tensor, so a step captured in a hipGraph follows a schedule.
Any other parameter set takes a per-tensor torch loop with the same formulas.
"""
from __future__ import annotations

import torch

from .optimizers import BaseOptimizer


class LARS(BaseOptimizer):
    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, trust_coefficient=0.001,
                 eps=1e-9, nesterov=False, exclude_1d=True, max_grad_norm=None):
        super().__init__(params, lr)
        self.momentum, self.weight_decay = momentum, weight_decay
        self.trust_coefficient, self.eps = trust_coefficient, eps
        self.nesterov, self.exclude_1d = nesterov, exclude_1d
        self.max_grad_norm = max_grad_norm
        # per-tensor records (adapted, stats rows) follow the flat buffer's order when
        # there is one: that is the order of the device tables
        self.tensors = self.flat.params if self.flat is not None else self.params
        self.adapted = [not (exclude_1d and p.ndim <= 1) for p in self.tensors]
        n = len(self.params)
        dev = self.flat.device if self.flat is not None else (
            self.params[0].device if self.params else torch.device("cpu"))
        # logging outputs, written by every step without a host synchronisation
        self._stats = torch.zeros(n, 3, device=dev)
        self._gnorm = torch.zeros(1, device=dev)
        self._hyper = None
        if self.flat is not None:
            self.buf = torch.zeros_like(self.flat.data)
        else:
            self.bufs = [torch.zeros_like(p) for p in self.params]
        if self._native():
            from dmlab.ops._native import lib

            f = self.flat
            seg, chunks = lib().lars_table(list(f.offsets), [p.numel() for p in f.params],
                                           self.adapted, f.numel)
            self._seg, self._chunks = seg.to(dev), chunks.to(dev)
            m = chunks.shape[0]
            self._partial = torch.zeros(2 * m, device=dev)
            self._tot = torch.zeros(2 * n, device=dev)
            self._hyper_host = self._hyper_values()
            self._hyper = torch.tensor(self._hyper_host, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------ device hyper-parameters
    def _hyper_values(self):
        """The order of the hyper-parameter slots in csrc/lars.hip."""
        mg = self.max_grad_norm
        return [float(self.lr), float(self.momentum), float(self.weight_decay),
                float(self.trust_coefficient), float(self.eps), float(self.grad_scale),
                float(mg) if mg is not None else -1.0]

    def _sync_hyper(self):
        """Write the slots whose host value changed: one fill launch each, by value, so
        nothing is allocated, nothing waits, and an unchanged step launches nothing extra
        (a captured step therefore never carries a stale rate with it)."""
        vals = self._hyper_values()
        for i, (new, old) in enumerate(zip(vals, self._hyper_host)):
            if new != old:
                self._hyper[i:i + 1].fill_(new)
                self._hyper_host[i] = new

    @property
    def lr(self):
        return self._groups[0]["lr"]

    @lr.setter
    def lr(self, v):
        self._groups[0]["lr"] = v
        if getattr(self, "_hyper", None) is not None:
            self._sync_hyper()  # at once: the next graph replay reads the device scalar

    def stats(self):
        """``(stats, grad_norm)``: ``stats[i] = (|w_i|, |g'_i|, r_i)`` of the last step for
        ``opt.tensors[i]`` (the flat buffer's order when there is one) and the
        global norm ``G`` as a 1-element tensor.  Device tensors, no synchronisation."""
        return self._stats, self._gnorm

    def _state_tensors(self):
        if self.flat is not None:
            return {"buf": self.buf}
        return {f"buf{i}": b for i, b in enumerate(self.bufs)}

    # ------------------------------------------------------------ step
    def step(self):
        self.step_count += 1
        if self._native():
            from dmlab.ops._native import lib

            f = self.flat
            self._sync_hyper()
            lib().lars_step(f.data, f.grad, self.buf, self._seg, self._chunks, self._hyper,
                            self._partial, self._tot, self._stats, self._gnorm, self.nesterov)
            f.mark_updated()
            return
        with torch.no_grad():
            if self.flat is not None:
                f = self.flat
                items = [(i, f.data_view(i), f.grad_view(i),
                          self.buf[o:o + p.numel()].view_as(p))
                         for i, (p, o) in enumerate(zip(f.params, f.offsets))]
            else:
                items = [(i, p, p.grad, self.bufs[i]) for i, p in enumerate(self.params)
                         if p.grad is not None]
            if not items:
                return
            gs, mu, wd, lr = self.grad_scale, self.momentum, self.weight_decay, self.lr
            eta, eps = self.trust_coefficient, self.eps
            G = torch.stack([(g * gs).square().sum() for _, _, g, _ in items]).sum().sqrt()
            self._gnorm.copy_(G.reshape(1))
            one = torch.ones((), device=G.device, dtype=G.dtype)
            c = one if self.max_grad_norm is None else \
                torch.clamp(self.max_grad_norm / (G + 1e-6), max=1.0)
            for i, w, g, b in items:
                gp = g * (c * gs)
                wn, gn = w.norm(), gp.norm()
                if self.adapted[i]:
                    r = torch.where((wn > 0) & (gn > 0), eta * wn / (gn + wd * wn + eps),
                                    one.to(wn.dtype))
                    d = r * (gp + wd * w)
                else:
                    r, d = one.to(wn.dtype), gp
                b.mul_(mu).add_(d)
                w.sub_(lr * (d + mu * b if self.nesterov else b))
                self._stats[i].copy_(torch.stack([wn, gn, r]))


class WarmupPolyLR:
    """Linear warm-up from 0 to the optimiser's base rate over ``warmup_steps``, then
    ``end_lr + (base - end_lr) * (1 - (t - warmup) / (total - warmup)) ** power``.

    The constructor sets the rate of step 0; call :meth:`step` after each optimiser step.
    Pure host code: it only assigns ``opt.lr``."""

    def __init__(self, opt, warmup_steps, total_steps, power=2.0, end_lr=0.0):
        if not 0 <= warmup_steps <= total_steps:
            raise ValueError("need 0 <= warmup_steps <= total_steps")
        self.opt = opt
        self.base_lr = opt.lr
        self.warmup_steps, self.total_steps = int(warmup_steps), int(total_steps)
        self.power, self.end_lr = power, end_lr
        self.t = 0
        opt.lr = self.lr_at(0)

    def lr_at(self, t):
        t = min(max(int(t), 0), self.total_steps)
        if t < self.warmup_steps:
            return self.base_lr * t / self.warmup_steps
        span = self.total_steps - self.warmup_steps
        frac = (t - self.warmup_steps) / span if span > 0 else 1.0
        return self.end_lr + (self.base_lr - self.end_lr) * (1.0 - frac) ** self.power

    def step(self):
        self.t += 1
        lr = self.lr_at(self.t)
        self.opt.lr = lr
        return lr
