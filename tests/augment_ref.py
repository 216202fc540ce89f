"""Oracle and shared cases for the augmentation tests (CPU and GPU).

:func:`ref_sums` is the kernel's formula (csrc/augment.hip, docs/KERNELS.md) as a plain
per-pixel loop over Python numbers, independent of the torch CPU path in
``dmlab.data.augment``: for output pixel (oy, ox) of sample b

    ox' = flip ? OW-1-ox : ox;  sx = X0 + ox'*DX;  xi = sx >> 16;  fx = (sx >> 8) & 255

(the same for y), taps (yi|yi+1, xi|xi+1) with weights (256-fy|fy)*(256-fx|fx); a tap outside
the inclusive box reads as zero (flags bit 1) or is clamped to the box.  It returns the
weighted sums S = sum w*p, exact for integer pixels (Python ints) and float64 for real ones;
the uint8 result is (S + 32768) >> 16 and the real-valued one S / 65536.

The planted parameter rows and shapes below are the cases the kernel tests share; each
reference is computed once per process (:func:`batch_sums`) and never modified.
"""
import functools

import numpy as np
import torch

FLIP, ZERO = 1, 2


def ref_sums(images, idx, params, OH, OW, tapmax=False):
    """``images`` (N,H,W,C) numpy (integer or float), ``idx`` ints [B], ``params`` [B][8] ints
    -> S [B,OH,OW,C] (int64 for integer images, float64 otherwise); with ``tapmax`` also the
    largest |tap| that entered each output value."""
    N, H, W, C = images.shape
    integer = np.issubdtype(images.dtype, np.integer)
    px = images.tolist()
    B = len(idx)
    S = [[[[0] * C for _ in range(OW)] for _ in range(OH)] for _ in range(B)]
    M = [[[[0.0] * C for _ in range(OW)] for _ in range(OH)] for _ in range(B)] if tapmax else None
    for b in range(B):
        n = int(idx[b])
        if not 0 <= n < N:
            continue  # a row outside the dataset is written as zeros
        X0, Y0, DX, DY, flags, xbox, ybox = (int(v) for v in params[b][:7])
        flip, zero = bool(flags & FLIP), bool(flags & ZERO)
        xlo, xhi = xbox & 0xFFFF, (xbox >> 16) & 0xFFFF
        ylo, yhi = ybox & 0xFFFF, (ybox >> 16) & 0xFFFF
        assert 0 <= xlo <= xhi < W and 0 <= ylo <= yhi < H, "box outside the image"
        img = px[n]

        def axis(origin, step, o, lo, hi):
            """The (position, weight) of the taps that are read; one that reads as zero
            contributes nothing and is left out."""
            s = origin + o * step
            assert -2 ** 31 <= s < 2 ** 31
            i, f = s >> 16, (s >> 8) & 255
            taps = []
            for t, w in ((i, 256 - f), (i + 1, f)):
                if zero and not lo <= t <= hi:
                    continue
                taps.append((min(max(t, lo), hi), w))
            return taps

        txs = [axis(X0, DX, OW - 1 - ox if flip else ox, xlo, xhi) for ox in range(OW)]
        for oy in range(OH):
            ty = axis(Y0, DY, oy, ylo, yhi)
            for ox in range(OW):
                acc = S[b][oy][ox]
                for y, wy in ty:
                    row = img[y]
                    for x, wx in txs[ox]:
                        p = row[x]
                        w = wy * wx
                        if C == 1:
                            acc[0] += w * p[0]
                        else:
                            for c in range(C):
                                acc[c] += w * p[c]
                        if tapmax:
                            m = M[b][oy][ox]
                            for c in range(C):
                                m[c] = max(m[c], abs(p[c]))
    out = np.array(S, dtype=np.int64 if integer else np.float64).reshape(B, OH, OW, C)
    if tapmax:
        return out, np.array(M, dtype=np.float64).reshape(B, OH, OW, C)
    return out


def to_u8(S):
    return ((S + 32768) >> 16).astype(np.uint8)


def to_real(S):
    return S.astype(np.float64) / 65536.0


def expected(S, dtype):
    """The oracle's result in a torch dtype.  For integer pixels 0..255 every product and
    sum of the float path is exact in fp32 (255 * 65536 < 2^24), so the fp32 result is
    S / 65536 exactly and the bf16 one its round-to-nearest-even."""
    if dtype == torch.uint8:
        return torch.from_numpy(to_u8(S))
    return torch.from_numpy(to_real(S)).to(torch.float32).to(dtype)


def box(lo, n):
    return lo | ((lo + n - 1) << 16)


def resize_row(x0, y0, w, h, OH, OW, flags=0):
    """The parameter row that resizes box (x0, y0, w, h) to (OH, OW), taps clamped."""
    DX, DY = (w << 16) // OW, (h << 16) // OH
    return [(x0 << 16) + DX // 2 - 32768, (y0 << 16) + DY // 2 - 32768, DX, DY, flags,
            box(x0, w), box(y0, h), 0]


def planted(H, W, OH, OW, P=2):
    """The planted parameter rows (name, row), each without and with the flip bit."""
    full = [box(0, W), box(0, H), 0]
    one = 65536
    rows = [
        ("identity", [0, 0, one, one, 0] + full),
        ("pad_shift_pos", [P * one, -P * one, one, one, ZERO] + full),
        ("pad_shift_neg", [-P * one, P * one, one, one, ZERO] + full),
        ("shift_whole_height", [0, H * one, one, one, ZERO] + full),
        ("negative_x0_clamped", [-3 * one + 0x4000, -one - 0x8000, one, one, 0] + full),
        ("box_1x1_upsampled", resize_row(min(2, W - 1), min(2, H - 1), 1, 1, OH, OW)),
        ("full_image_box", resize_row(0, 0, W, H, OH, OW)),
        ("box_at_right_bottom", resize_row(W - 3, H - 2, 3, 2, OH, OW)),
        ("interior_box", resize_row(1, 1, W - 2, H - 3, OH, OW)),
    ]
    out = []
    for name, r in rows:
        out.append((name, list(r)))
        f = list(r)
        f[4] |= FLIP
        out.append((name + "+flip", f))
    return out


# (N, H, W) -> (OH, OW), batch sizes
SHAPES = [
    ((3, 5, 7), (4, 6), (1, 5)),        # small, odd
    ((3, 13, 11), (13, 11), (1, 5)),    # a uint8 row of 33 bytes: a vector tail
    ((3, 9, 10), (17, 19), (1, 5)),     # upsampling
    ((3, 224, 224), (224, 224), (2,)),  # the workload's own row length
]


def n_batches(B):
    return -(-18 // B)  # planted() has 9 kinds x {plain, flipped}


# (src, out, B, C, ks): ks = the batches of planted rows one test case runs.  The small shapes
# run all of them in one case; at 224 x 224 the oracle loop takes ~0.5 s per batch, so every
# batch (one planted kind, plain and flipped) is a case of its own.
CASES = [(src, out, B, C, ks) for src, out, Bs in SHAPES for B in Bs for C in (1, 3)
         for ks in ([tuple(range(n_batches(B)))] if src[1] < 100
                    else [(k,) for k in range(n_batches(B))])]
CASE_IDS = [f"{s[1]}x{s[2]}to{o[0]}x{o[1]}-B{B}-C{C}" + (f"-k{ks[0]}" if len(ks) == 1 else "")
            for s, o, B, C, ks in CASES]


def images_u8(N, H, W, C, seed=0):
    g = np.random.default_rng(seed + 1000 * H + W + 7 * C)
    return g.integers(0, 256, size=(N, H, W, C), dtype=np.uint8)


def batch_idx(N, B, k):
    """Descending with repeats (never sorted ascending), varied per batch k."""
    base = [N - 1, N - 1, 1, 0, 0]
    return [base[(j + k) % 5] if B == 1 else base[j % 5] for j in range(B)]


@functools.lru_cache(maxsize=None)
def source(src, C):
    N, H, W = src
    im = images_u8(N, H, W, C)
    im.setflags(write=False)
    return im


def batch_rows(src, out, B, k):
    """(idx, params) of batch k: the planted rows of the shape packed B to a batch."""
    N, H, W = src
    rows = [r for _, r in planted(H, W, out[0], out[1])]
    assert len(rows) == 18
    while len(rows) % B:
        rows.append(rows[len(rows) % 7])
    return batch_idx(N, B, k), rows[k * B: (k + 1) * B]


@functools.lru_cache(maxsize=None)
def batch_sums(src, out, B, C, k):
    """The oracle's sums S int64 [B,OH,OW,C] of batch k, computed once per process and
    read-only."""
    idx, par = batch_rows(src, out, B, k)
    S = ref_sums(source(src, C), idx, par, out[0], out[1])
    S.setflags(write=False)
    return S


def case(src, out, B, C, ks):
    """(images uint8 numpy (N,H,W,C), [(idx list, params list, S), ...] for the batches ks)."""
    return source(src, C), [batch_rows(src, out, B, k) + (batch_sums(src, out, B, C, k),)
                            for k in ks]


def torch_images(im, dtype, device="cpu"):
    """The integer-valued image array in a torch dtype (0..255 is exact in bf16)."""
    return torch.from_numpy(np.array(im)).to(device).to(dtype)
