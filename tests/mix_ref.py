"""Oracle and shared cases for the mixup / CutMix tests (CPU and GPU).

``augment_ref`` (imported unchanged) gives the exact weighted sums S of every sample of a batch;
this module applies the mixing rules of csrc/augment_mix.hip to them.  For output pixel
(oy, ox) of sample b with mix row ``partner, L, xbox, ybox`` (box = lo | hi << 16, inclusive,
in output pixels), A from S[b] and P from S[partner]:

    inside the box              out = P as the augmentation stores it
    outside, L == 65536         out = A as the augmentation stores it
    otherwise, uint8            (L*a + (65536-L)*p + 32768) >> 16 on a, p = (S + 32768) >> 16
    otherwise, fp32 / bf16      ((float)L*a' + (float)(65536-L)*p') * 2^-16 on a', p' = S / 65536,
                                every operation rounded to fp32 on its own (numpy float32
                                scalars do exactly that), bf16 rounded once at the end

L is clamped to [0, 65536]; a partner outside [0, B) makes the row unmixed.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import augment_ref as R

ONE = 65536
EMPTY = 1  # lo = 1, hi = 0


def box(lo, hi):
    """Inclusive [lo, hi] packed as the table holds it."""
    return lo | (hi << 16)


def unmixed_row(b):
    return [b, ONE, EMPTY, EMPTY]


def planted_mix(OH, OW):
    """(name, partner or None = the mirrored position, L, xbox, ybox)."""
    return [
        ("unmixed", "self", ONE, EMPTY, EMPTY),
        ("L0", None, 0, EMPTY, EMPTY),
        ("L1", None, 1, EMPTY, EMPTY),
        ("L19661", None, 19661, EMPTY, EMPTY),
        ("L32768", None, 32768, EMPTY, EMPTY),
        ("L65535", None, 65535, EMPTY, EMPTY),
        ("full_image_box", None, ONE, box(0, OW - 1), box(0, OH - 1)),
        ("box_1x1_at_origin", None, ONE, box(0, 0), box(0, 0)),
        ("box_bottom_right", None, ONE, box(OW - 2, OW - 1), box(OH - 3, OH - 1)),
        ("box_hi_past_output", None, ONE, box(1, OW + 40), box(2, 0x7FFF)),
        ("box_and_blend", None, 19661, box(1, OW // 2), box(0, OH // 2)),
        ("partner_minus_1", -1, 32768, box(0, OW - 1), box(0, OH - 1)),
        ("partner_B", "B", 32768, box(0, OW - 1), box(0, OH - 1)),
        ("L_above_one", None, 70000, EMPTY, EMPTY),
        ("L_negative", None, -5, EMPTY, EMPTY),
    ]


def mix_rows(OH, OW, B, k):
    """The mix table of batch k: the planted kinds dealt round-robin over the batch slots."""
    kinds = planted_mix(OH, OW)
    rows = []
    for b in range(B):
        _, partner, L, xb, yb = kinds[(k * B + b) % len(kinds)]
        partner = {None: B - 1 - b, "self": b, "B": B}.get(partner, partner)
        rows.append([partner, L, xb, yb])
    return rows


def _planes(mixrow, b, B, OH, OW):
    """(partner or None, clamped L, inbox mask [OH,OW,1]) of one mix row."""
    partner, L, xb, yb = (int(v) for v in mixrow)
    if not 0 <= partner < B:
        return None, ONE, np.zeros((OH, OW, 1), bool)
    L = min(max(L, 0), ONE)
    ox = np.arange(OW)[None, :, None]
    oy = np.arange(OH)[:, None, None]
    inbox = ((ox >= (xb & 0xFFFF)) & (ox <= ((xb >> 16) & 0xFFFF))
             & (oy >= (yb & 0xFFFF)) & (oy <= ((yb >> 16) & 0xFFFF)))
    return partner, L, inbox


def expected(S, mix, dtype):
    """The kernel's result for integer-valued pixels from the exact sums S int64 [B,OH,OW,C]
    (for those, the unrounded fp32 blend of a sample is S / 65536 exactly)."""
    B, OH, OW, C = S.shape
    if dtype == torch.uint8:
        val = R.to_u8(S).astype(np.int64)
        out = np.empty(S.shape, np.uint8)
    else:
        val = (S.astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)
        out = np.empty(S.shape, np.float32)
    for b in range(B):
        partner, L, inbox = _planes(mix[b], b, B, OH, OW)
        a = val[b]
        if partner is None:
            out[b] = a
            continue
        p = val[partner]
        if L == ONE:
            blend = a
        elif dtype == torch.uint8:
            blend = (L * a + (ONE - L) * p + 32768) >> 16
        else:
            x = np.float32(L) * a            # float32 arrays: each operation is rounded once
            y = np.float32(ONE - L) * p
            blend = ((x + y).astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)
            assert x.dtype == np.float32 and y.dtype == np.float32
        out[b] = np.where(inbox, p, blend)
    t = torch.from_numpy(out)
    return t if dtype == torch.uint8 else t.to(dtype)


def expected_real(S, M, mix):
    """float64 evaluation for real-valued pixels: (want, largest |tap| behind each value) from
    ``augment_ref.ref_sums(..., tapmax=True)``."""
    B, OH, OW, C = S.shape
    val = R.to_real(S)
    want, tap = np.empty_like(val), np.empty_like(M)
    for b in range(B):
        partner, L, inbox = _planes(mix[b], b, B, OH, OW)
        if partner is None:
            want[b], tap[b] = val[b], M[b]
            continue
        lam = L / ONE
        blend = val[b] if L == ONE else lam * val[b] + (1.0 - lam) * val[partner]
        btap = M[b] if L == ONE else np.maximum(M[b], M[partner])
        want[b] = np.where(inbox, val[partner], blend)
        tap[b] = np.where(inbox, M[partner], btap)
    return want, tap


# the three small shapes of augment_ref (224 x 224 is left to the augmentation's own test)
SHAPES = [(src, out) for src, out, _ in R.SHAPES if src[1] < 100]
BATCHES = (1, 2, 5)
CASES = [(src, out, B, C) for src, out in SHAPES for B in BATCHES for C in (1, 3)]
CASE_IDS = [f"{s[1]}x{s[2]}to{o[0]}x{o[1]}-B{B}-C{C}" for s, o, B, C in CASES]


def n_batches(B):
    return -(-18 // B)  # augment_ref's planted parameter rows; >= the 15 mix kinds


@functools.lru_cache(maxsize=None)
def case(src, out, B, C):
    """(images uint8 numpy, [(idx, params, mix, S), ...]): every batch of augment_ref's planted
    parameter rows with the planted mix rows dealt over it; S computed once per process."""
    return R.source(src, C), [R.batch_rows(src, out, B, k) + (mix_rows(out[0], out[1], B, k),
                                                              R.batch_sums(src, out, B, C, k))
                              for k in range(n_batches(B))]


# ------------------------------------------------------------------ mixed cross-entropy
def _soft_target(y, C, eps):
    return F.one_hot(y, C).double() * (1 - eps) + eps / C


def mixed_ce_reference(x, ya, yb, lam, eps, ignore_index=-100):
    """float64 F.cross_entropy on explicit probability targets lam*smooth(ya) +
    (1-lam)*smooth(yb); a row with an invalid label in either slot has loss 0; mean over B."""
    B, C = x.shape
    valid = (ya >= 0) & (ya < C) & (yb >= 0) & (yb < C) & (ya != ignore_index) & (yb != ignore_index)
    a, b = ya.clamp(0, C - 1), yb.clamp(0, C - 1)
    lam = lam.double()[:, None]
    tgt = lam * _soft_target(a, C, eps) + (1 - lam) * _soft_target(b, C, eps)
    rows = F.cross_entropy(x.double(), tgt, reduction="none")
    return (rows * valid).sum() / B


def mixed_ce_rows(B, C, seed=0, device="cpu"):
    """Labels and weights with every planted kind of row: lam in {0, 1, 0.3, random}, equal
    labels, and (from 5 rows on) an invalid label in either slot."""
    g = torch.Generator().manual_seed(seed + 31 * B + C)
    ya = torch.randint(0, C, (B,), generator=g)
    yb = torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    i = torch.arange(B)
    lam[i % 4 == 0] = 0.0
    lam[i % 4 == 1] = 1.0
    lam[i % 4 == 2] = 0.3
    yb[i % 3 == 1] = ya[i % 3 == 1]
    if B >= 5:
        ya[2] = -100
        yb[3] = C
        yb[4] = -1
    return ya.to(device), yb.to(device), lam.to(device)
