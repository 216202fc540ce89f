"""Cross-rank ("synchronized") BatchNorm for :class:`ConvBN` / :class:`ConvBNPool`.

Data-parallel training normalises every layer over the rank's own shard; with
:func:`convert_sync_batchnorm` a program's BatchNorm layers use the statistics of the
whole global batch instead, so N ranks at batch B compute what one process at batch N*B
computes.

Per channel, rank ``r`` holds ``n_r`` elements.

Forward: each rank reduces its statistics to one float64 row ``[mean_r | M2_r | n_r]``
(``M2_r = Σ(y - mean_r)²``); the rows are all-gathered and every rank merges them in rank
order 0..ws-1 in double::

    N = Σ n_r     mean = Σ n_r mean_r / N     M2 = Σ [M2_r + n_r (mean_r - mean)²]

``var = M2/N`` gives ``invstd``, ``scale``, ``shift`` and the running statistics (unbiased
variance over N).  Same rows, same order: the results are bit-identical on all ranks, and
the ``n_r`` may differ between ranks.

Backward: the local sums ``S_r = Σdz`` and ``Q_r = Σdz·x̂`` (x̂ from the global mean and
invstd) give ``dbeta`` / ``dgamma`` as they are -- the data-parallel gradient average makes
them global -- and are all-reduced (SUM; one result for every rank) into ``S`` and ``Q`` for
``dy = γ·invstd·(dz - S/N - x̂·Q/N)``.

One all-gather per layer and forward, one all-reduce per layer and backward, issued under
whatever stream is current, in program order (the same on every rank).  Eval mode issues
none.
"""
from __future__ import annotations

import torch
import torch.distributed as dist


class SyncBNState:
    """What the synced layers of one program share: the process group (None: one rank, no
    group -- the sync kernels still run, no collective is issued) and the collective counter."""

    def __init__(self, group, ws):
        self.group = group
        self.ws = ws
        self.collectives = 0  # sync collectives issued so far (cf. DDP.buckets_launched)

    def __deepcopy__(self, memo):
        return self  # a copied program stays in the same group (process groups do not copy)

    def _check_capture(self, t):
        if (t.is_cuda and self.group is not None and torch.cuda.is_current_stream_capturing()
                and dist.get_backend(self.group) != "nccl"):
            raise RuntimeError(
                "synchronized BatchNorm inside a captured graph: the collectives of the "
                f"'{dist.get_backend(self.group)}' backend cannot be captured")

    def gather_rows(self, row):
        """row [L] -> rows [ws, L]: every rank's row, in rank order."""
        if self.group is None:
            return row.unsqueeze(0)
        self._check_capture(row)
        rows = torch.empty((self.ws, row.numel()), dtype=row.dtype, device=row.device)
        # asynchronous + wait: on RCCL the group's own stream carries the collective, ordered
        # after the current stream and joined back into it on the device (no host sync); the
        # layers issue from three streams, and one communicator must not run on two at once
        if dist.get_backend(self.group) == "nccl":
            dist.all_gather_into_tensor(rows, row, group=self.group, async_op=True).wait()
        else:
            dist.all_gather(list(rows.unbind(0)), row, group=self.group, async_op=True).wait()
        self.collectives += 1
        return rows

    def reduce_sums(self, sums):
        """In-place SUM over the ranks (every rank receives the same bits)."""
        if self.group is None:
            return sums
        self._check_capture(sums)
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.group, async_op=True).wait()
        self.collectives += 1
        return sums


def merge_rows(rows, C):
    """(mean, var, N) of the merged rows [ws, 2C+1] -- the reference form of the native
    ``bn_sync_finalize`` merge: rank order, double."""
    n = rows[:, 2 * C]
    N = n[0].clone()
    sm = n[0] * rows[0, :C]
    for r in range(1, rows.shape[0]):
        N = N + n[r]
        sm = sm + n[r] * rows[r, :C]
    mean = sm / N
    M2 = torch.zeros_like(mean)
    for r in range(rows.shape[0]):
        M2 = M2 + rows[r, C:2 * C] + n[r] * (rows[r, :C] - mean) ** 2
    return mean, M2 / N, N


class _SyncBatchNormFn(torch.autograd.Function):
    """Training-mode synchronized batch norm of an NCHW tensor through local autograd (the
    torch / CPU path of ConvBN); statistics and sums travel and merge in float64."""

    @staticmethod
    def forward(ctx, y, gamma, beta, layer, state):
        C = y.shape[1]
        yd = y.detach().double()
        n_r = y.numel() // C
        mean_r = yd.mean(dim=(0, 2, 3))
        m2_r = ((yd - mean_r.view(1, C, 1, 1)) ** 2).sum(dim=(0, 2, 3))
        row = torch.cat([mean_r, m2_r, torch.full((1,), float(n_r), dtype=torch.float64,
                                                  device=y.device)])
        mean, var, N = merge_rows(state.gather_rows(row), C)
        invstd = 1.0 / torch.sqrt(var + layer.eps)
        with torch.no_grad():
            unbiased = torch.where(N > 1, var * N / (N - 1), var)
            m = layer.momentum
            layer.running_mean.mul_(1 - m).add_(m * mean.to(layer.running_mean.dtype))
            layer.running_var.mul_(1 - m).add_(m * unbiased.to(layer.running_var.dtype))
        xhat = ((yd - mean.view(1, C, 1, 1)) * invstd.view(1, C, 1, 1)).to(y.dtype)
        ctx.save_for_backward(xhat, gamma, invstd, N)
        ctx.state = state
        return xhat * gamma.view(1, C, 1, 1).to(y.dtype) + beta.view(1, C, 1, 1).to(y.dtype)

    @staticmethod
    def backward(ctx, dz):
        xhat, gamma, invstd, N = ctx.saved_tensors
        C = dz.shape[1]
        dzd, xd = dz.double(), xhat.double()
        S = dzd.sum(dim=(0, 2, 3))
        Q = (dzd * xd).sum(dim=(0, 2, 3))
        dbeta, dgamma = S.to(gamma.dtype), Q.to(gamma.dtype)  # local: DDP averages them
        sums = ctx.state.reduce_sums(torch.cat([S, Q]))
        S, Q = sums[:C], sums[C:]
        a = (gamma.double() * invstd).view(1, C, 1, 1)
        dy = a * (dzd - (S / N).view(1, C, 1, 1) - xd * (Q / N).view(1, C, 1, 1))
        return dy.to(dz.dtype), dgamma, dbeta, None, None


def sync_batch_norm(y, layer):
    return _SyncBatchNormFn.apply(y, layer.bn_weight, layer.bn_bias, layer, layer._sync_bn)


def _synced_layers(program):
    from .layers import ConvBN

    return [m for m in program.modules() if isinstance(m, ConvBN)]


def convert_sync_batchnorm(program, process_group=None, force=False):
    """Mark every ``ConvBN`` / ``ConvBNPool`` of ``program`` as synchronized across the ranks
    of ``process_group`` and return the program.  Apply it before wrapping the model in DDP.

    EVERY rank must call it: with no ``process_group`` it creates a dedicated group over all
    ranks (a collective), so the small BatchNorm collectives do not queue behind DDP's 25 MB
    bucket all-reduces on the default group's stream.

    With no initialised process group, or at world size 1, it is a no-op unless ``force`` is
    set; then the sync kernels run, and the collectives too on the 1-rank group if there is
    one (as ``DDP(force_comm=True)``: a one-GPU box exercises the 8-GPU code).

    ``program.sync_bn_collectives`` counts the collectives issued so far."""
    init = dist.is_available() and dist.is_initialized()
    ws = dist.get_world_size(process_group) if init else 1
    if ws == 1 and not force:
        return program
    group = None
    if init:
        group = process_group if process_group is not None else dist.new_group()
    state = SyncBNState(group, ws)
    for m in _synced_layers(program):
        m._sync_bn = state
    program._sync_bn_state = state
    return program
