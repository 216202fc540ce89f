"""Gradient compression for the data-parallel exchange: the "q8" codec.

Block-wise int8 quantisation with error feedback.  One bucket is one contiguous fp32 slice
of ``n`` elements, processed in blocks of ``BLOCK = 256`` consecutive elements counted from
the slice's start (the last block may be partial).

Encode, per block (all arithmetic fp32, IEEE round-to-nearest-even):

* ``e = g + r`` (``r``: the persistent residual, zero at construction; without error
  feedback ``e = g`` and no residual exists);
* ``a = max |e|``, ``s = a / 127`` (a correctly rounded division);
* ``s == 0`` (``a`` zero, or ``a / 127`` underflows): every code 0, ``r = e``;
* ``a`` not finite: ``s = NaN``, every code 0, ``r = 0`` -- the block decodes to NaN on every
  rank, so a diverged run is seen and not hidden;
* otherwise ``q = clamp(rint(e / s), -127, 127)`` (a correctly rounded division, ties to
  even) and ``r = e - q*s`` (the product is rounded, then the difference: no FMA).

One rank's payload for one bucket is one contiguous ``uint8`` buffer: ``ceil(n/256)`` fp32
scales, then ``n`` int8 codes, then padding to a multiple of 16 bytes (:func:`payload_bytes`),
about 1/3.94 of the fp32 bytes.

Decode-mean of ``[ws, payload_bytes]`` (every rank's payload in rank order):
``out = c * sum_{rank = 0..ws-1} q[rank] * s[rank]``, accumulated in fp32 in that order (each
product rounded before it is added), so every rank computes bit-identical gradients.

On a HIP device both halves are kernels (``csrc/gradq.hip``); anywhere else the vectorised
torch implementation below runs the same formulas, operation for operation.
"""
from __future__ import annotations

import torch

BLOCK = 256


def n_blocks(n: int) -> int:
    return (int(n) + BLOCK - 1) // BLOCK


def payload_bytes(n: int) -> int:
    """Bytes of one rank's payload for a bucket of ``n`` elements."""
    return (4 * n_blocks(n) + int(n) + 15) // 16 * 16


def _check(payload, n):
    if payload.dtype != torch.uint8 or payload.dim() != 1 or payload.numel() != payload_bytes(n):
        raise ValueError(f"payload must be a 1-d uint8 tensor of payload_bytes({n}) = "
                         f"{payload_bytes(n)} bytes")


@torch.no_grad()
def encode_torch(g, r, payload):
    """The torch path of the encoder: ``g`` [n] fp32, ``r`` [n] fp32 or None (updated in
    place), ``payload`` [payload_bytes(n)] uint8."""
    n = g.numel()
    nb = n_blocks(n)
    _check(payload, n)
    e = g + r if r is not None else g
    ep = e.new_zeros(nb * BLOCK)
    ep[:n] = e
    ep = ep.view(nb, BLOCK)
    a = ep.abs().amax(dim=1)  # amax propagates NaN
    finite = torch.isfinite(a)
    # a tensor divisor: an element-wise IEEE division on every backend (a scalar divisor may be
    # turned into a multiplication by its reciprocal)
    s = torch.where(finite, a / torch.full_like(a, 127.0), torch.full_like(a, float("nan")))
    live = finite & (s != 0)
    sd = torch.where(live, s, torch.ones_like(s)).unsqueeze(1)
    lv = live.unsqueeze(1)
    q = torch.where(lv, torch.clamp(torch.round(ep / sd), -127.0, 127.0), torch.zeros_like(ep))
    payload[:4 * nb].view(torch.float32).copy_(s)
    payload[4 * nb:4 * nb + n].view(torch.int8).copy_(q.view(-1)[:n].to(torch.int8))
    if r is not None:
        res = torch.where(lv, ep - q * sd,
                          torch.where(finite.unsqueeze(1), ep, torch.zeros_like(ep)))
        r.copy_(res.view(-1)[:n])


@torch.no_grad()
def decode_mean_torch(gathered, out, scale):
    """The torch path of the decoder: ``gathered`` [ws, payload_bytes(n)] uint8 -> ``out`` [n]."""
    n = out.numel()
    nb = n_blocks(n)
    if gathered.dtype != torch.uint8 or gathered.dim() != 2 or \
            gathered.shape[1] != payload_bytes(n):
        raise ValueError(f"gathered must be [ws, payload_bytes({n})] uint8")
    acc = torch.zeros(n, dtype=torch.float32, device=out.device)
    for rk in range(gathered.shape[0]):
        row = gathered[rk]
        s = row[:4 * nb].view(torch.float32).repeat_interleave(BLOCK)[:n]
        q = row[4 * nb:4 * nb + n].view(torch.int8).to(torch.float32)
        acc = acc + q * s
    out.copy_(acc * torch.tensor(scale, dtype=torch.float32, device=out.device))


class Q8Compressor:
    """The q8 codec over one gradient buffer of ``numel`` elements.  Owns the error-feedback
    residual (training state: :meth:`state_dict` / :meth:`load_state_dict`), sized to the whole
    buffer; a bucket ``[lo, lo+n)`` uses its slice."""

    def __init__(self, numel: int, device, error_feedback: bool = True):
        self.numel = int(numel)
        self.device = torch.device(device)
        self.error_feedback = bool(error_feedback)
        self.residual = (torch.zeros(self.numel, dtype=torch.float32, device=self.device)
                         if self.error_feedback else None)

    @torch.no_grad()
    def encode(self, view, lo: int, payload):
        """Quantise ``view`` (the buffer's elements ``[lo, lo + view.numel())``) into
        ``payload``; the residual slice is read and replaced."""
        n = view.numel()
        if lo < 0 or lo + n > self.numel:
            raise ValueError(f"bucket [{lo}, {lo + n}) outside the buffer of {self.numel}")
        r = self.residual[lo:lo + n] if self.residual is not None else None
        if view.is_cuda:
            from dmlab.ops._native import lib

            lib().q8_encode(view, r, payload)
        else:
            encode_torch(view, r, payload)

    @torch.no_grad()
    def decode_mean(self, gathered, out, scale: float):
        if out.is_cuda:
            from dmlab.ops._native import lib

            lib().q8_decode_mean(gathered, out, float(scale))
        else:
            decode_mean_torch(gathered, out, float(scale))

    def state_dict(self):
        return {"error_feedback": self.error_feedback, "numel": self.numel,
                "residual": None if self.residual is None else self.residual.detach().clone()}

    def load_state_dict(self, sd):
        r = sd.get("residual")
        if self.residual is None or r is None:
            if (self.residual is None) != (r is None):
                raise ValueError("q8 state: error feedback is on in one of checkpoint / run "
                                 "and off in the other")
            return
        if r.numel() != self.numel:
            raise ValueError(f"q8 residual of {r.numel()} elements, buffer has {self.numel}")
        self.residual.copy_(r.to(self.residual.device, torch.float32))
