"""On-device crop / resize / flip augmentation for the device-resident loader.

The dataset never leaves the device (:mod:`dmlab.data.loader`), so the augmentation runs
there too: one native kernel (``csrc/augment.hip``) gathers a batch by dataset row and
applies a per-sample affine sampling window, taking the place of the loader's
``index_select``.  What the kernel does to sample ``b`` is written in one 32-byte row of
int32 parameters::

    X0, Y0, DX, DY, flags, xbox, ybox, 0

``X0 / Y0 / DX / DY`` are 16.16 fixed point (source coordinate of output pixel ``o`` is
``X0 + o * DX``), ``flags`` bit 0 flips horizontally, bit 1 makes taps outside the box read
as zero (clear: they are clamped to the box), ``xbox = xlo | xhi << 16`` (inclusive).

**Randomness is stateless and keyed by dataset index.**  The parameters of sample ``i`` at
epoch ``e`` are a pure function of ``(seed, i, e)`` (Philox4x32-10, counter = (i lo, i hi,
epoch, block), key = seed), computed on the host in numpy for the indices a rank will use.
The same sample at the same epoch therefore gets the same augmentation on every rank, at any
world size, batch size or sampler mode.  Block 0 of a sample holds ``flip, tx, ty, spare``;
blocks 1..10 are the tries of the random resized crop (``area, log-ratio, x-offset,
y-offset``).
"""
from __future__ import annotations

import math

import numpy as np
import torch

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
ZERO_FILL = 2
FLIP = 1


def philox4x32(counter, key, rounds: int = 10):
    """Philox4x32 (Random123): ``counter`` (..., 4) and ``key`` (..., 2) arrays of 32-bit
    words (broadcast against each other) -> (..., 4) uint32 output words."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., j] for j in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(rounds):
        if r:
            k0 = (k0 + _W0) & _MASK
            k1 = (k1 + _W1) & _MASK
        p0 = c0 * _M0  # 32 x 32 -> 64 bits, exact in uint64
        p1 = c2 * _M1
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK)
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def _uniform(seed: int, idx: np.ndarray, epoch: int, block: int) -> np.ndarray:
    """Four uniforms in (0, 1) per index: u = (word + 0.5) / 2^32 in float64."""
    i = idx.astype(np.uint64)
    ctr = np.stack([i & _MASK, i >> _S32, np.full_like(i, int(epoch) & 0xFFFFFFFF),
                    np.full_like(i, block)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return (philox4x32(ctr, key).astype(np.float64) + 0.5) / 4294967296.0


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def _fallback_box(H, W, ratio):
    """torchvision's RandomResizedCrop fallback: the centre crop with the aspect ratio
    clamped into ``ratio``."""
    in_ratio = W / H
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    w, h = min(max(w, 1), W), min(max(h, 1), H)
    return (W - w) // 2, (H - h) // 2, w, h


def _nhwc_view(x: torch.Tensor):
    """((N,H,W,C) view, was_nchw) of a channels_last (N,C,H,W) or contiguous (N,H,W,C)
    image tensor with C = 1 or 3.  A shape that fits both (a one-row image) is read as
    (N,C,H,W), as the native binding does."""
    if x.dim() != 4:
        raise ValueError(f"expected a 4-D image tensor, got shape {tuple(x.shape)}")
    if x.shape[1] in (1, 3) and x.permute(0, 2, 3, 1).is_contiguous():
        return x.permute(0, 2, 3, 1), True
    if x.shape[3] in (1, 3) and x.is_contiguous():
        return x, False
    raise ValueError("images must be (N,H,W,C) contiguous or (N,C,H,W) channels_last with "
                     f"C = 1 or 3 (shape {tuple(x.shape)}, strides {x.stride()})")


def image_size(images: torch.Tensor):
    """(H, W) of a channel-innermost image tensor (either accepted layout)."""
    v, _ = _nhwc_view(images)
    return int(v.shape[1]), int(v.shape[2])


class DeviceAugment:
    """A per-sample crop / resize / flip, drawn statelessly per (seed, dataset index, epoch).

    ``mode``:

    * ``"pad_crop"`` (``pad=P``): the image shifted by ``tx, ty`` uniform in ``[-P, P]``
      with zero fill: zero-padding by P and a random crop of the original size.
    * ``"rrc"`` (``out``, ``scale``, ``ratio``): torchvision's RandomResizedCrop box (area
      uniform in ``scale * H * W``, aspect log-uniform in ``ratio``, first of 10 tries that
      fits, else the ratio-clamped centre crop) resized bilinearly to ``out``.
    * ``"center"`` (``out``, ``frac``): the centred ``frac`` of each side resized to ``out``;
      deterministic, for evaluation.

    ``flip``: probability of a horizontal flip.  ``size=(H, W)`` is the source image size; a
    :class:`~dmlab.data.DeviceLoader` fills it in from its dataset."""

    MODES = ("pad_crop", "rrc", "center")

    def __init__(self, mode: str, *, pad: int = 4, out=None, scale=(0.08, 1.0),
                 ratio=(3.0 / 4.0, 4.0 / 3.0), frac: float = 0.875, flip: float = 0.0,
                 seed: int = 0, size=None):
        mode = {"pad-crop": "pad_crop", "random_resized_crop": "rrc"}.get(mode, mode)
        if mode not in self.MODES:
            raise ValueError(f"unknown augmentation mode {mode!r}")
        if not 0.0 <= flip <= 1.0:
            raise ValueError("flip probability must be in [0, 1]")
        if mode != "pad_crop" and out is None:
            raise ValueError(f"mode {mode!r} needs an output size (out=)")
        if mode == "pad_crop" and not 0 <= int(pad) < 16384:
            raise ValueError("pad must be in [0, 16384)")
        if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
            raise ValueError("scale and ratio must be positive (lo, hi) ranges")
        if not 0.0 < frac <= 1.0:
            raise ValueError("frac must be in (0, 1]")
        self.mode = mode
        self.pad = int(pad)
        self.out = _pair(out) if out is not None else None
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        self.frac = float(frac)
        self.flip = 0.0 if mode == "center" else float(flip)
        self.seed = int(seed)
        self.size = _pair(size) if size is not None else None

    # ---------------------------------------------------------------- constructors
    @classmethod
    def pad_crop(cls, pad: int = 4, **kw):
        return cls("pad_crop", pad=pad, **kw)

    @classmethod
    def random_resized_crop(cls, out, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), **kw):
        return cls("rrc", out=out, scale=scale, ratio=ratio, **kw)

    @classmethod
    def center(cls, out, frac: float = 0.875, **kw):
        return cls("center", out=out, frac=frac, **kw)

    def eval(self) -> "DeviceAugment":
        """The matching deterministic transform: the centre crop at the same output size
        for ``rrc``, the unshifted, unflipped image for ``pad_crop``."""
        if self.mode == "pad_crop":
            return DeviceAugment("pad_crop", pad=0, flip=0.0, seed=self.seed, size=self.size)
        return DeviceAugment("center", out=self.out, frac=self.frac, seed=self.seed,
                             size=self.size)

    def out_size(self, size=None):
        """(OH, OW) for a source of ``size`` = (H, W)."""
        if self.out is not None:
            return self.out
        size = size if size is not None else self.size
        if size is None:
            raise ValueError("the source image size is not known: pass size=(H, W)")
        return _pair(size)

    # ---------------------------------------------------------------- parameters
    def boxes(self, idx, epoch: int = 0, size=None):
        """(x0, y0, w, h) int64 arrays: the crop box of every index (the whole image for
        ``pad_crop``)."""
        H, W = self._size(size)
        i = self._idx(idx)
        n = i.shape[0]
        if self.mode == "pad_crop":
            return (np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, W, np.int64),
                    np.full(n, H, np.int64))
        if self.mode == "center":
            w = min(max(int(round(W * self.frac)), 1), W)
            h = min(max(int(round(H * self.frac)), 1), H)
            return (np.full(n, (W - w) // 2, np.int64), np.full(n, (H - h) // 2, np.int64),
                    np.full(n, w, np.int64), np.full(n, h, np.int64))
        fx0, fy0, fw, fh = _fallback_box(H, W, self.ratio)
        x0 = np.full(n, fx0, np.int64)
        y0 = np.full(n, fy0, np.int64)
        bw = np.full(n, fw, np.int64)
        bh = np.full(n, fh, np.int64)
        todo = np.arange(n)
        lr0, lr1 = math.log(self.ratio[0]), math.log(self.ratio[1])
        for t in range(1, 11):  # only the indices no earlier try has settled
            if todo.size == 0:
                break
            u = _uniform(self.seed, i[todo], epoch, t)
            area = H * W * (self.scale[0] + u[:, 0] * (self.scale[1] - self.scale[0]))
            ar = np.exp(lr0 + u[:, 1] * (lr1 - lr0))
            w = np.rint(np.sqrt(area * ar)).astype(np.int64)
            h = np.rint(np.sqrt(area / ar)).astype(np.int64)
            ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
            sel = todo[ok]
            bw[sel], bh[sel] = w[ok], h[ok]
            x0[sel] = np.minimum(np.floor(u[ok, 2] * (W - w[ok] + 1)).astype(np.int64), W - w[ok])
            y0[sel] = np.minimum(np.floor(u[ok, 3] * (H - h[ok] + 1)).astype(np.int64), H - h[ok])
            todo = todo[~ok]
        return x0, y0, bw, bh

    def params(self, idx, epoch: int = 0, size=None) -> torch.Tensor:
        """The int32 [B,8] parameter table (a host tensor) of dataset rows ``idx`` at
        ``epoch``; row b depends on ``(seed, idx[b], epoch)`` only."""
        H, W = self._size(size)
        OH, OW = self.out_size((H, W))
        i = self._idx(idx)
        n = i.shape[0]
        u = _uniform(self.seed, i, epoch, 0)
        flags = (u[:, 0] < self.flip).astype(np.int64) * FLIP
        x0, y0, w, h = self.boxes(i, epoch, (H, W))
        if self.mode == "pad_crop":
            span = 2 * self.pad + 1
            tx = np.minimum(np.floor(u[:, 1] * span).astype(np.int64), span - 1) - self.pad
            ty = np.minimum(np.floor(u[:, 2] * span).astype(np.int64), span - 1) - self.pad
            X0, Y0 = tx << 16, ty << 16
            DX = np.full(n, 65536, np.int64)
            DY = np.full(n, 65536, np.int64)
            flags = flags | ZERO_FILL
        else:
            DX = (w << 16) // OW
            DY = (h << 16) // OH
            X0 = (x0 << 16) + DX // 2 - 32768
            Y0 = (y0 << 16) + DY // 2 - 32768
        tab = np.zeros((n, 8), np.int64)
        tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3] = X0, Y0, DX, DY
        tab[:, 4] = flags
        tab[:, 5] = x0 | ((x0 + w - 1) << 16)
        tab[:, 6] = y0 | ((y0 + h - 1) << 16)
        return torch.from_numpy(tab.astype(np.int32))

    def _size(self, size):
        size = size if size is not None else self.size
        if size is None:
            raise ValueError("the source image size is not known: pass size=(H, W)")
        H, W = _pair(size)
        if not (1 <= H <= 16384 and 1 <= W <= 16384):
            raise ValueError("image sides must be in [1, 16384]")
        return H, W

    @staticmethod
    def _idx(idx) -> np.ndarray:
        if isinstance(idx, torch.Tensor):
            idx = idx.detach().cpu().numpy()
        return np.asarray(idx, dtype=np.int64).reshape(-1)

    # ---------------------------------------------------------------- application
    def apply(self, images: torch.Tensor, idx: torch.Tensor, params: torch.Tensor):
        """``out[b] = transform(params[b], images[idx[b]])`` as a fresh tensor in the layout
        of ``images`` ((B,C,OH,OW) channels_last or (B,OH,OW,C)).  On a HIP device this is
        one launch of the native kernel (the gather happens inside it); elsewhere a
        vectorised torch implementation of the same integer arithmetic."""
        v, nchw = _nhwc_view(images)
        OH, OW = self.out_size((v.shape[1], v.shape[2]))
        if images.is_cuda:
            from dmlab.ops._native import lib

            out = torch.empty((idx.numel(), OH, OW, v.shape[3]), device=images.device,
                              dtype=images.dtype)
            lib().augment_apply(v, idx, params, out)
        else:
            out = apply_reference(v, idx, params, OH, OW)
        return out.permute(0, 3, 1, 2) if nchw else out


def _axis(origin, step, flip, box, zero, n_out):
    """Tap positions (clamped into the box), validity and fraction of one axis: [B, n_out]."""
    o = torch.arange(n_out, dtype=torch.int64, device=origin.device)[None, :]
    if flip is not None:
        o = torch.where(flip[:, None], n_out - 1 - o, o)
    s = origin[:, None] + o * step[:, None]
    s = ((s + 2 ** 31) % 2 ** 32) - 2 ** 31  # int32 wrap, as the kernel computes it
    i0 = s >> 16
    i1 = i0 + 1
    f = (s >> 8) & 255
    lo = (box & 0xFFFF)[:, None]
    hi = ((box >> 16) & 0xFFFF)[:, None]
    z = zero[:, None]
    v0 = ~z | ((i0 >= lo) & (i0 <= hi))
    v1 = ~z | ((i1 >= lo) & (i1 <= hi))
    return (torch.minimum(torch.maximum(i0, lo), hi), torch.minimum(torch.maximum(i1, lo), hi),
            v0, v1, f)


def apply_reference(images: torch.Tensor, idx: torch.Tensor, params: torch.Tensor, OH: int,
                    OW: int) -> torch.Tensor:
    """The kernel's arithmetic in vectorised torch ops: ``images`` (N,H,W,C) (any strides),
    ``idx`` int64 [B], ``params`` int32 [B,8] -> (B,OH,OW,C) in the dtype of ``images``."""
    N, H, W, C = images.shape
    dev = images.device
    idx = idx.to(dev).long()
    p = params.to(dev).long()
    rowok = (idx >= 0) & (idx < N)
    n = torch.where(rowok, idx, torch.zeros_like(idx))
    flags = p[:, 4]
    flip, zero = (flags & FLIP) != 0, (flags & ZERO_FILL) != 0

    def clampbox(box, size):  # the box clamped to the image, as the kernel does
        hi = torch.clamp((box >> 16) & 0xFFFF, max=size - 1)
        lo = torch.minimum(box & 0xFFFF, hi)
        return lo | (hi << 16)

    x0, x1, vx0, vx1, fx = _axis(p[:, 0], p[:, 2], flip, clampbox(p[:, 5], W), zero, OW)
    y0, y1, vy0, vy1, fy = _axis(p[:, 1], p[:, 3], None, clampbox(p[:, 6], H), zero, OH)
    nb = n[:, None, None]

    def tap(y, x, vy, vx):
        t = images[nb, y[:, :, None], x[:, None, :]]  # [B,OH,OW,C]
        ok = (vy[:, :, None] & vx[:, None, :] & rowok[:, None, None])[..., None]
        return torch.where(ok, t, torch.zeros((), dtype=t.dtype, device=dev))

    p00, p01 = tap(y0, x0, vy0, vx0), tap(y0, x1, vy0, vx1)
    p10, p11 = tap(y1, x0, vy1, vx0), tap(y1, x1, vy1, vx1)
    fy, fx = fy[:, :, None, None], fx[:, None, :, None]
    w00, w01 = (256 - fy) * (256 - fx), (256 - fy) * fx
    w10, w11 = fy * (256 - fx), fy * fx
    if images.dtype == torch.uint8:
        acc = (w00 * p00.long() + w01 * p01.long() + w10 * p10.long() + w11 * p11.long()
               + 32768) >> 16
        return acc.to(torch.uint8)
    f = torch.float32  # separate multiplies and adds: torch's elementwise ops do not fuse
    top = w00.to(f) * p00.to(f) + w01.to(f) * p01.to(f)
    bot = w10.to(f) * p10.to(f) + w11.to(f) * p11.to(f)
    out = (top + bot) * (2.0 ** -16)
    out = torch.where(rowok[:, None, None, None], out, torch.zeros((), dtype=f, device=dev))
    return out.to(images.dtype)
