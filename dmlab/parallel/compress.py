"""Gradient compression for the data-parallel exchange: the "q8" codec (this docstring) and
the "topk" codec (block-wise sparsification, described above :class:`TopKCompressor` below).

q8: block-wise int8 quantisation with error feedback.  One bucket is one contiguous fp32 slice
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

    def payload_bytes(self, n: int) -> int:
        """Bytes of one rank's payload for a bucket of ``n`` elements."""
        return payload_bytes(n)

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


# ---------------------------------------------------------------------------------- topk
# The "topk" codec: block-wise sparsification with error feedback (Deep Gradient Compression /
# EF-SGD, block-wise so that the payload layout is fixed and the indices fit 16 bits).
#
# A bucket of ``n`` fp32 elements is cut into blocks of ``TOPK_BLOCK = 2048`` consecutive
# elements counted from the slice's start (the last one may hold ``m < 2048``); ``keep`` = K
# (1..256) entries are kept per block.  Encode, per block, fp32:
#
# * ``e = g + r`` (``e = g`` without error feedback);
# * ``key(i) = bits(e[i]) & 0x7fffffff``: the magnitude as an integer (+-0 -> 0, Inf above
#   every finite value, NaN above Inf: a non-finite entry is always sent);
# * the ``min(K, m)`` largest keys are selected, equal keys in ascending in-block index (zeros
#   like any other value), and emitted in ascending index: slot ``j`` holds ``e[i_j]`` bit for
#   bit and ``i_j`` as uint16; unused slots (``m < K`` only) hold index 0xFFFF and +0.0;
# * ``r = +0.0`` at the selected positions, ``e`` elsewhere.
#
# One rank's payload, ``nb = ceil(n/2048)``: ``nb*K`` fp32 values, ``nb*K`` uint16 indices,
# padding to 16 bytes: ``6K/8192`` of the fp32 bytes (K = 32: 1/42.7).
# Decode-mean of ``[ws, payload]``: ``acc = +0.0``; for rank 0..ws-1 in that order
# ``acc = acc + v`` where the rank's block lists the element; ``out = c * acc``, every element
# written.  On a HIP device both halves are kernels (``csrc/gradk.hip``).
TOPK_BLOCK = 2048
TOPK_MAX_KEEP = 256
_UNUSED = 0xFFFF


def _check_keep(keep):
    keep = int(keep)
    if not 1 <= keep <= TOPK_MAX_KEEP:
        raise ValueError(f"keep must be in 1..{TOPK_MAX_KEEP}, got {keep}")
    return keep


def topk_n_blocks(n: int) -> int:
    return (int(n) + TOPK_BLOCK - 1) // TOPK_BLOCK


def topk_payload_bytes(n: int, keep: int = 32) -> int:
    """Bytes of one rank's topk payload for a bucket of ``n`` elements."""
    return (6 * topk_n_blocks(n) * _check_keep(keep) + 15) // 16 * 16


def _topk_check(payload, n, keep):
    nbytes = topk_payload_bytes(n, keep)
    if payload.dtype != torch.uint8 or payload.dim() != 1 or payload.numel() != nbytes:
        raise ValueError(f"payload must be a 1-d uint8 tensor of topk_payload_bytes({n}, {keep}) "
                         f"= {nbytes} bytes")


@torch.no_grad()
def topk_encode_torch(g, r, payload, keep: int = 32):
    """The torch path of the topk encoder: ``g`` [n] fp32, ``r`` [n] fp32 or None (updated in
    place), ``payload`` [topk_payload_bytes(n, keep)] uint8 (its padding is left as it is)."""
    n = g.numel()
    K = _check_keep(keep)
    nb = topk_n_blocks(n)
    _topk_check(payload, n, K)
    if n == 0:
        return
    e = (g + r if r is not None else g).contiguous()
    keys = (e.view(torch.int32) & 0x7FFFFFFF).to(torch.int64)
    kp = keys.new_full((nb * TOPK_BLOCK,), -1)  # past the end: below every key
    kp[:n] = keys
    # one integer orders (key descending, index ascending): all distinct, so the K largest are
    # a defined set
    pos = torch.arange(TOPK_BLOCK, dtype=torch.int64, device=g.device)
    comp = kp.view(nb, TOPK_BLOCK) * TOPK_BLOCK + (TOPK_BLOCK - 1 - pos)
    top = torch.topk(comp, K, dim=1).values
    idx = torch.where(top >= 0, TOPK_BLOCK - 1 - top % TOPK_BLOCK,
                      torch.full_like(top, _UNUSED))
    idx = torch.sort(idx, dim=1).values  # ascending index, the unused slots last
    used = idx != _UNUSED
    flat = (idx + TOPK_BLOCK * torch.arange(nb, dtype=torch.int64,
                                            device=g.device).unsqueeze(1))[used]
    vals = torch.zeros((nb, K), dtype=torch.float32, device=g.device)
    vals[used] = e[flat]
    payload[:4 * nb * K].view(torch.float32).copy_(vals.view(-1))
    # 0xFFFF as int16 is -1
    payload[4 * nb * K:6 * nb * K].view(torch.int16).copy_(
        torch.where(used, idx, torch.full_like(idx, -1)).view(-1).to(torch.int16))
    if r is not None:
        r.copy_(e)
        r[flat] = 0.0


@torch.no_grad()
def topk_decode_mean_torch(gathered, out, scale, keep: int = 32):
    """The torch path of the topk decoder: ``gathered`` [ws, topk_payload_bytes(n, keep)] uint8
    -> ``out`` [n]."""
    n = out.numel()
    K = _check_keep(keep)
    nb = topk_n_blocks(n)
    if gathered.dtype != torch.uint8 or gathered.dim() != 2 or \
            gathered.shape[1] != topk_payload_bytes(n, K):
        raise ValueError(f"gathered must be [ws, topk_payload_bytes({n}, {K})] uint8")
    acc = torch.zeros(nb * TOPK_BLOCK, dtype=torch.float32, device=out.device)
    base = TOPK_BLOCK * torch.arange(nb, dtype=torch.int64, device=out.device).unsqueeze(1)
    for rk in range(gathered.shape[0]):
        row = gathered[rk]
        vals = row[:4 * nb * K].view(torch.float32).view(nb, K)
        idx = row[4 * nb * K:6 * nb * K].view(torch.int16).to(torch.int64).view(nb, K) & 0xFFFF
        used = idx < TOPK_BLOCK
        flat = (idx + base)[used]
        # one rank's indices are distinct within a block: a plain gather, add, scatter
        acc[flat] = acc[flat] + vals[used]
    out.copy_(acc[:n] * torch.tensor(scale, dtype=torch.float32, device=out.device))


class TopKCompressor:
    """The topk codec over one gradient buffer of ``numel`` elements, with the interface of
    :class:`Q8Compressor`: owns the error-feedback residual, sized to the whole buffer; a bucket
    ``[lo, lo+n)`` uses its slice (its blocks count from ``lo``)."""

    def __init__(self, numel: int, device, keep: int = 32, error_feedback: bool = True):
        self.numel = int(numel)
        self.device = torch.device(device)
        self.keep = _check_keep(keep)
        self.error_feedback = bool(error_feedback)
        self.residual = (torch.zeros(self.numel, dtype=torch.float32, device=self.device)
                         if self.error_feedback else None)

    def payload_bytes(self, n: int) -> int:
        """Bytes of one rank's payload for a bucket of ``n`` elements."""
        return topk_payload_bytes(n, self.keep)

    @torch.no_grad()
    def encode(self, view, lo: int, payload):
        """Sparsify ``view`` (the buffer's elements ``[lo, lo + view.numel())``) into
        ``payload``; the residual slice is read and replaced."""
        n = view.numel()
        if lo < 0 or lo + n > self.numel:
            raise ValueError(f"bucket [{lo}, {lo + n}) outside the buffer of {self.numel}")
        r = self.residual[lo:lo + n] if self.residual is not None else None
        if view.is_cuda:
            from dmlab.ops._native import lib

            lib().topk_encode(view, r, payload, self.keep)
        else:
            topk_encode_torch(view, r, payload, self.keep)

    @torch.no_grad()
    def decode_mean(self, gathered, out, scale: float):
        if out.is_cuda:
            from dmlab.ops._native import lib

            lib().topk_decode_mean(gathered, out, self.keep, float(scale))
        else:
            topk_decode_mean_torch(gathered, out, float(scale), self.keep)

    def state_dict(self):
        return {"error_feedback": self.error_feedback, "numel": self.numel, "keep": self.keep,
                "residual": None if self.residual is None else self.residual.detach().clone()}

    def load_state_dict(self, sd):
        r = sd.get("residual")
        if self.residual is None or r is None:
            if (self.residual is None) != (r is None):
                raise ValueError("topk state: error feedback is on in one of checkpoint / run "
                                 "and off in the other")
            return
        if r.numel() != self.numel:
            raise ValueError(f"topk residual of {r.numel()} elements, buffer has {self.numel}")
        self.residual.copy_(r.to(self.residual.device, torch.float32))


CODECS = ("q8", "topk")


def make_compressor(codec: str, numel: int, device, error_feedback: bool = True, keep: int = 32):
    """The compressor object of a codec name (``q8`` | ``topk``)."""
    if codec == "q8":
        return Q8Compressor(numel, device, error_feedback)
    if codec == "topk":
        return TopKCompressor(numel, device, keep, error_feedback)
    raise ValueError(f"compress: one of {CODECS}, got {codec!r}")
