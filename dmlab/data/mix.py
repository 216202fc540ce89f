"""On-device mixup and CutMix for the device-resident loader.

A mixed sample is made of two dataset rows: mixup blends the two augmented images with a
weight λ, CutMix pastes a box of the second into the first; the target is both labels with
the weight ``lam`` of the first (:class:`~dmlab.nn.MixTarget`).  The mixing happens inside the
augmentation launch (``csrc/augment_mix.hip``): the batch is still written once, and what is
done to sample ``b`` is one 16-byte row of int32 parameters::

    partner, L, xbox, ybox

``partner`` is the batch position of the second sample (augmented by its OWN parameter row),
``L`` the pixel weight of the first in 1/65536, and the box ``lo | hi << 16`` (inclusive, in
output pixel coordinates; empty is ``lo=1, hi=0``) the region taken from the partner.  An
unmixed row is ``partner=b, L=65536``, an empty box and ``lam=1``.

**The draw is stateless**, as :class:`~dmlab.data.DeviceAugment`'s is: every column but the
partner is a pure function of ``(seed, dataset index, epoch, OH, OW)``.  The augmentation uses
Philox blocks 0..10 of a sample; here block 16 holds ``u_apply, u_kind, u_cx, u_cy`` and blocks
17..24 are up to eight tries of the Beta sampler (words 0 and 1 of a block are ``u, v``).  The
partner is position ``B-1-b`` of the same batch (the middle sample of an odd batch pairs with
itself), so it is the one thing that depends on how the indices are batched.

λ0 ~ Beta(α, α): for α > 0.5 the closed form ``½(1 + sqrt(1 − u^(2/(2α−1)))·cos 2πv)`` (Ulrich's
method, no rejection); for α ≤ 0.5 Jöhnk's method, ``x = u^(1/α), y = v^(1/α)``, the first of
eight tries with ``0 < x+y ≤ 1`` gives ``x/(x+y)``; a sample with no accepted try stays unmixed.
"""
from __future__ import annotations

import numpy as np
import torch

from .augment import DeviceAugment, _nhwc_view, _pair, _uniform, apply_reference

ONE = 65536
EMPTY_BOX = 1  # lo = 1, hi = 0
BLOCK_DRAW, BLOCK_BETA, BETA_TRIES = 16, 17, 8


def _pack_box(lo, hi):
    """[lo, hi) half-open -> the inclusive ``lo | hi << 16`` of the table (empty: lo=1, hi=0)."""
    empty = hi <= lo
    return np.where(empty, EMPTY_BOX, lo | ((hi - 1) << 16))


class DeviceMix:
    """Per-sample mixup / CutMix, drawn statelessly per (seed, dataset index, epoch).

    ``mixup_alpha`` / ``cutmix_alpha``: the Beta(α, α) parameter of each kind, 0 = that kind is
    off (at least one must be on).  A sample is mixed with probability ``prob``; with both
    kinds on it is CutMix with probability ``switch_prob``, else mixup."""

    def __init__(self, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
                 switch_prob: float = 0.5, seed: int = 0):
        mixup_alpha, cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        if mixup_alpha < 0.0 or cutmix_alpha < 0.0:
            raise ValueError("mixup_alpha and cutmix_alpha must be >= 0")
        if mixup_alpha == 0.0 and cutmix_alpha == 0.0:
            raise ValueError("DeviceMix needs mixup_alpha > 0 or cutmix_alpha > 0")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError("prob and switch_prob must be in [0, 1]")
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.prob = float(prob)
        self.switch_prob = float(switch_prob)
        self.seed = int(seed)

    # ---------------------------------------------------------------- the draw
    def _beta(self, idx: np.ndarray, epoch: int, alpha: float):
        """(λ0, accepted) of Beta(alpha, alpha) for every index."""
        n = idx.shape[0]
        if alpha > 0.5:
            u = _uniform(self.seed, idx, epoch, BLOCK_BETA)
            s = np.sqrt(1.0 - u[:, 0] ** (2.0 / (2.0 * alpha - 1.0)))
            return 0.5 * (1.0 + s * np.cos(2.0 * np.pi * u[:, 1])), np.ones(n, bool)
        lam = np.ones(n, np.float64)
        ok = np.zeros(n, bool)
        todo = np.arange(n)
        for t in range(BETA_TRIES):  # only the indices no earlier try has settled
            if todo.size == 0:
                break
            u = _uniform(self.seed, idx[todo], epoch, BLOCK_BETA + t)
            x, y = u[:, 0] ** (1.0 / alpha), u[:, 1] ** (1.0 / alpha)
            s = x + y
            acc = (s > 0.0) & (s <= 1.0)
            sel = todo[acc]
            lam[sel] = x[acc] / s[acc]
            ok[sel] = True
            todo = todo[~acc]
        return lam, ok

    def lambdas(self, idx, epoch: int = 0):
        """(λ0 float64, mixed, cutmix) per index: the Beta draw of the sample's kind, whether
        the sample is mixed at all, and whether its kind is CutMix."""
        i = DeviceAugment._idx(idx)
        u = _uniform(self.seed, i, epoch, BLOCK_DRAW)
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cut = u[:, 1] < self.switch_prob
        else:
            cut = np.full(i.shape[0], self.cutmix_alpha > 0.0)
        lam = np.ones(i.shape[0], np.float64)
        ok = np.zeros(i.shape[0], bool)
        for kind, alpha in ((False, self.mixup_alpha), (True, self.cutmix_alpha)):
            sel = np.nonzero(cut == kind)[0]
            if alpha > 0.0 and sel.size:
                lam[sel], ok[sel] = self._beta(i[sel], epoch, alpha)
        return lam, ok & (u[:, 0] < self.prob), cut

    def params(self, idx_batch, epoch: int, out_size):
        """``(mix int32 [B,4], lam float32 [B])`` (host tensors) of ONE batch of dataset rows
        at ``epoch`` for an (OH, OW) output.  Only column 0, the partner ``B-1-b``, depends
        on the batch."""
        OH, OW = _pair(out_size)
        i = DeviceAugment._idx(idx_batch)
        B = i.shape[0]
        lam0, mixed, cut = self.lambdas(i, epoch)
        u = _uniform(self.seed, i, epoch, BLOCK_DRAW)
        # mixup: the pixel weight in 1/65536 is the label weight
        L = np.rint(lam0 * ONE).astype(np.int64)
        lam = L.astype(np.float64) / ONE
        xbox = np.full(B, EMPTY_BOX, np.int64)
        ybox = np.full(B, EMPTY_BOX, np.int64)
        # CutMix: the box in output pixels, the label weight from its clipped area
        r = np.sqrt(1.0 - lam0)
        w, h = (OW * r).astype(np.int64), (OH * r).astype(np.int64)
        cx = np.floor(u[:, 2] * OW).astype(np.int64)
        cy = np.floor(u[:, 3] * OH).astype(np.int64)
        x1, x2 = np.clip(cx - w // 2, 0, OW), np.clip(cx + w // 2, 0, OW)
        y1, y2 = np.clip(cy - h // 2, 0, OH), np.clip(cy + h // 2, 0, OH)
        area = (x2 - x1) * (y2 - y1)
        mixed = mixed & (~cut | (area > 0))
        L = np.where(cut, ONE, L)
        lam = np.where(cut, 1.0 - area.astype(np.float64) / float(OH * OW), lam)
        xbox = np.where(cut, _pack_box(x1, x2), xbox)
        ybox = np.where(cut, _pack_box(y1, y2), ybox)
        tab = np.zeros((B, 4), np.int64)
        tab[:, 0] = np.where(mixed, B - 1 - np.arange(B), np.arange(B))
        tab[:, 1] = np.where(mixed, L, ONE)
        tab[:, 2] = np.where(mixed, xbox, EMPTY_BOX)
        tab[:, 3] = np.where(mixed, ybox, EMPTY_BOX)
        lam = np.where(mixed, lam, 1.0).astype(np.float32)
        return torch.from_numpy(tab.astype(np.int32)), torch.from_numpy(lam)

    def epoch_params(self, idx, epoch: int, out_size, batch_size: int):
        """The tables of a whole epoch's index list cut into batches of ``batch_size`` (the
        last one may be shorter and pairs within itself): ``mix`` [n,4], ``lam`` [n]."""
        i = DeviceAugment._idx(idx)
        parts = [self.params(i[s: s + batch_size], epoch, out_size)
                 for s in range(0, i.shape[0], batch_size)]
        if not parts:
            return torch.zeros((0, 4), dtype=torch.int32), torch.zeros(0, dtype=torch.float32)
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    # ---------------------------------------------------------------- application
    def apply(self, transform: DeviceAugment, images: torch.Tensor, idx: torch.Tensor,
              params: torch.Tensor, mix: torch.Tensor):
        """The mixed batch as a fresh tensor in the layout of ``images``: one launch of the
        native kernel on a HIP device, :func:`mix_reference` elsewhere."""
        v, nchw = _nhwc_view(images)
        OH, OW = transform.out_size((v.shape[1], v.shape[2]))
        if images.is_cuda:
            from dmlab.ops._native import lib

            out = torch.empty((idx.numel(), OH, OW, v.shape[3]), device=images.device,
                              dtype=images.dtype)
            lib().augment_mix_apply(v, idx, params, mix, out)
        else:
            out = mix_reference(v, idx, params, mix, OH, OW)
        return out.permute(0, 3, 1, 2) if nchw else out


def mix_reference(images: torch.Tensor, idx: torch.Tensor, params: torch.Tensor,
                  mix: torch.Tensor, OH: int, OW: int) -> torch.Tensor:
    """The mixing kernel's arithmetic in vectorised torch ops: ``images`` (N,H,W,C), ``idx``
    int64 [B], ``params`` int32 [B,8], ``mix`` int32 [B,4] -> (B,OH,OW,C)."""
    dev = images.device
    B = idx.numel()
    idx = idx.to(dev).long()
    params = params.to(dev)
    m = mix.to(dev).long()
    pok = (m[:, 0] >= 0) & (m[:, 0] < B)
    part = torch.where(pok, m[:, 0], torch.arange(B, device=dev))
    L = torch.where(pok, m[:, 1].clamp(0, ONE), torch.full_like(m[:, 1], ONE))
    u8 = images.dtype == torch.uint8
    # the float path blends the unrounded fp32 results: evaluate it on an fp32 copy (a bf16
    # pixel is exact in fp32, and apply_reference rounds once, into the dtype it is given)
    src = images if u8 else images.float()
    a = apply_reference(src, idx, params, OH, OW)
    p = apply_reference(src, idx[part], params[part], OH, OW)
    oy = torch.arange(OH, device=dev)[None, :, None, None]
    ox = torch.arange(OW, device=dev)[None, None, :, None]

    def col(c, shift):
        return ((m[:, c] >> shift) & 0xFFFF)[:, None, None, None]

    inbox = (pok[:, None, None, None] & (ox >= col(2, 0)) & (ox <= col(2, 16))
             & (oy >= col(3, 0)) & (oy <= col(3, 16)))
    Lb = L[:, None, None, None]
    if u8:
        blend = ((Lb * a.long() + (ONE - Lb) * p.long() + 32768) >> 16).to(torch.uint8)
    else:  # separate multiplies and adds: torch's elementwise ops do not fuse
        blend = (Lb.float() * a + (ONE - Lb).float() * p) * (2.0 ** -16)
    out = torch.where(inbox, p, torch.where(Lb == ONE, a, blend))
    return out.to(images.dtype)
