"""Cross-entropy loss (``nn.CrossEntropyLoss`` mean semantics) and evaluation metrics.

On a HIP device one fused kernel computes the mean loss AND the logits gradient
(softmax − onehot)/B during the forward; backward only scales it
by the incoming gradient.  CPU tensors use ``F.cross_entropy``.

``label_smoothing=ε`` trains against the target (1−ε)·onehot + ε/C (the large-batch
ResNet recipes use ε = 0.1): a second kernel of the same shape, one extra row sum, the
same two launches.  ε = 0 is the plain kernel, untouched.

A :class:`MixTarget` (two labels and the weight of the first per row, what mixup / CutMix
produce) trains against ``lam·smooth(ya) + (1−lam)·smooth(yb)``: a third kernel of the same
shape.  An int64 label tensor takes the paths above, untouched.

:class:`EvalMetrics` keeps top-1 / top-k hits and the test loss in a device-resident
state: one kernel pair per batch, one device-to-host read per evaluation.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        from dmlab.ops._native import lib

        logits = logits.contiguous()
        B = logits.shape[0]
        rowloss = torch.empty(B, device=logits.device, dtype=torch.float32)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        need = ctx.needs_input_grad[0]
        dlogits = torch.empty_like(logits) if need else None
        lib().cross_entropy(logits, labels.contiguous(), rowloss, loss, dlogits, 1.0 / B)
        ctx.save_for_backward(dlogits if need else None)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        if d is None:
            return None, None
        return d * g.to(d.dtype), None


class _SmoothCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, eps):
        from dmlab.ops._native import lib

        logits = logits.contiguous()
        B = logits.shape[0]
        rowloss = torch.empty(B, device=logits.device, dtype=torch.float32)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        need = ctx.needs_input_grad[0]
        dlogits = torch.empty_like(logits) if need else None
        lib().cross_entropy_smooth(logits, labels.contiguous(), rowloss, loss, dlogits, 1.0 / B,
                                   eps)
        ctx.save_for_backward(dlogits if need else None)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        if d is None:
            return None, None, None
        return d * g.to(d.dtype), None, None


class MixTarget(NamedTuple):
    """The target of a mixed batch: row ``i`` is ``lam[i]`` of class ``labels[i]`` and
    ``1 - lam[i]`` of class ``partner_labels[i]`` (int64 [B], int64 [B], float32 [B])."""

    labels: torch.Tensor
    partner_labels: torch.Tensor
    lam: torch.Tensor


class _MixCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, ya, yb, lam, eps):
        from dmlab.ops._native import lib

        logits = logits.contiguous()
        B = logits.shape[0]
        rowloss = torch.empty(B, device=logits.device, dtype=torch.float32)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        need = ctx.needs_input_grad[0]
        dlogits = torch.empty_like(logits) if need else None
        lib().cross_entropy_mix(logits, ya.contiguous(), yb.contiguous(),
                                lam.to(torch.float32).contiguous(), rowloss, loss, dlogits,
                                1.0 / B, eps)
        ctx.save_for_backward(dlogits if need else None)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        if d is None:
            return None, None, None, None, None
        return d * g.to(d.dtype), None, None, None, None


def _mix_cross_entropy_host(logits, target: MixTarget, eps: float, ignore_index: int = -100):
    """The mixed loss from ``F.cross_entropy(..., reduction="none")`` terms; a row with an
    invalid label in either slot has loss 0, and the mean is over all B rows."""
    x = logits.float() if logits.dtype != torch.float32 else logits
    B, C = x.shape
    ya, yb = target.labels, target.partner_labels
    valid = ((ya != ignore_index) & (ya >= 0) & (ya < C)
             & (yb != ignore_index) & (yb >= 0) & (yb < C))
    la = F.cross_entropy(x, torch.where(valid, ya, torch.zeros_like(ya)), reduction="none",
                         label_smoothing=eps)
    lb = F.cross_entropy(x, torch.where(valid, yb, torch.zeros_like(yb)), reduction="none",
                         label_smoothing=eps)
    lam = target.lam.to(torch.float32)
    row = torch.where(valid, lam * la + (1.0 - lam) * lb, torch.zeros_like(la))
    return row.sum() / B


def _check_smoothing(eps) -> float:
    eps = float(eps)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1], got {eps}")
    return eps


def cross_entropy(logits, labels, label_smoothing=0.0):
    """Mean cross-entropy of ``logits`` (B, C) against int64 labels [B] or a
    :class:`MixTarget`."""
    eps = _check_smoothing(label_smoothing)
    if isinstance(labels, MixTarget):
        if logits.is_cuda:
            return _MixCEFn.apply(logits, labels.labels, labels.partner_labels, labels.lam, eps)
        return _mix_cross_entropy_host(logits, labels, eps)
    if logits.is_cuda:
        if eps == 0.0:
            return _CEFn.apply(logits, labels)
        return _SmoothCEFn.apply(logits, labels, eps)
    return F.cross_entropy(logits.float() if logits.dtype != torch.float32 else logits, labels,
                           label_smoothing=eps)


class CrossEntropyLoss(nn.Module):
    def __init__(self, label_smoothing=0.0):
        super().__init__()
        self.label_smoothing = _check_smoothing(label_smoothing)

    def forward(self, logits, labels):
        return cross_entropy(logits, labels, self.label_smoothing)


@torch.no_grad()
def count_correct(logits, labels, counter=None):
    """Add the number of correct argmax predictions to a device counter (int64)."""
    if counter is None:
        counter = torch.zeros((), device=logits.device, dtype=torch.long)
    if logits.is_cuda:
        from dmlab.ops._native import lib

        lib().argmax_count(logits.contiguous(), labels.contiguous(), counter)
    else:
        counter += (logits.argmax(1) == labels).sum()
    return counter


class EvalMetrics:
    """Top-1 / top-k accuracy and mean (unsmoothed) cross-entropy over an evaluation.

    The label's rank in its row is ``#{c : x_c > x_y} + #{c < y : x_c == x_y}`` and a row
    hits at k iff ``rank < k``; at k = 1 that is :func:`count_correct`'s first-index argmax
    rule, and k >= C makes every valid row a hit.  A label outside [0, C) is a miss with
    loss 0; a NaN label logit is a miss.

    State, on ``device``: ``counts`` = int64 [n, top-1 hits, top-k hits] and ``loss_sum`` =
    float64 [sum of row losses].  ``update`` adds one batch without a host read (fixed
    summation order, no atomics: the same batches give the same bits; graph-capturable),
    ``all_reduce`` sums the state over the default process group, ``result`` reads it back.
    """

    def __init__(self, k=5, device=None):
        k = int(k)
        if k < 1:
            raise ValueError(f"k must be >= 1, got {k}")
        self.k = k
        self.device = torch.device(device if device is not None else "cpu")
        self.counts = torch.zeros(3, dtype=torch.long, device=self.device)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=self.device)

    def reset(self):
        self.counts.zero_()
        self.loss_sum.zero_()

    @torch.no_grad()
    def update(self, logits, labels):
        if logits.dim() != 2 or labels.shape != logits.shape[:1]:
            raise ValueError("EvalMetrics.update: logits (B, C) and labels (B,)")
        B, C = logits.shape
        if B == 0:
            return self
        if logits.is_cuda:
            from dmlab.ops._native import lib

            rowloss = torch.empty(B, device=logits.device, dtype=torch.float32)
            rowrank = torch.empty(B, device=logits.device, dtype=torch.int32)
            lib().eval_metrics(logits.contiguous(), labels.contiguous(), rowloss, rowrank, self.k,
                               self.counts, self.loss_sum)
            return self
        x = logits.float()
        valid = (labels >= 0) & (labels < C)
        y = labels.clamp(0, C - 1)
        xy = x.gather(1, y[:, None])
        cols = torch.arange(C, device=x.device)[None, :]
        rank = ((x > xy) | ((x == xy) & (cols < y[:, None]))).sum(1)
        ok = valid & ~torch.isnan(xy[:, 0])
        nll = torch.logsumexp(x.double(), 1) - xy[:, 0].double()
        nll = torch.where(valid, nll, torch.zeros_like(nll))
        self.counts += torch.stack([torch.tensor(B, device=x.device), (ok & (rank < 1)).sum(),
                                    (ok & (rank < self.k)).sum()])
        self.loss_sum += nll.sum()
        return self

    def all_reduce(self):
        """SUM the four state values over the default process group (no-op without one).
        One collective: the counts travel as float64, exact below 2**53."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()):
            return self
        packed = torch.cat([self.counts.double(), self.loss_sum])
        dist.all_reduce(packed, op=dist.ReduceOp.SUM)
        self.counts.copy_(packed[:3].round().long())
        self.loss_sum.copy_(packed[3:])
        return self

    def result(self):
        """One device-to-host read.  ``top1`` / ``topk`` are hit counts out of ``n`` rows,
        ``loss`` is the mean row loss."""
        n, c1, ck, ls = torch.cat([self.counts.double(), self.loss_sum]).tolist()
        n = int(n)
        return {"n": n, "top1": int(c1), "topk": int(ck), "k": self.k,
                "loss": ls / n if n else 0.0}
