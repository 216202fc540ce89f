"""Element-exact references for the fused ResNet stem (csrc/stem_fused.hip).

The stem takes its normalisation (nsc, nbi) and its grid as arguments, so a test can feed raw
images that normalise to small integers exactly: every bf16 x bf16 product and every fp32
partial sum of the conv, of D = dz^T X and of G = X^T X is then an exact integer in any
accumulation order (MFMA order, images per workgroup, the fixed-order slab reduce), the kernel's
bf16 rounding of the conv output is the one round-to-nearest-even of torch, and dyadic BN
coefficients keep dW = wbeta dW0 + a D + b W G + cc G[93] exact in fp32.  This module draws such
operands, computes the float64 references from explicit tap and window loops (never a library
convolution or pooling), and never calls the code under test.  tests/test_exact_stem_cpu.py
asserts the conditions under which exactness holds for every case drawn here."""
import functools
import zlib
from types import SimpleNamespace

import torch

# ------------------------------------------------------------------ the cases
# (B, Nimg, H, W, grid): batch rows, image rows, image size, workgroups
SHAPES = [
    (5, 7, 32, 32, 2),    # Wout 16: a partial 32-pixel MFMA block, nt = 1; 3 + 2 images per workgroup
    (2, 2, 8, 32, 2),     # PH 2: the shortest step stream, rows 8, 9 staged from outside; M = 128
    (4, 4, 8, 64, 1),     # Wout 32: exactly one block; one workgroup walks 4 images; M = 512
    (3, 3, 12, 64, 3),    # PH 3 (odd), one image per workgroup
    (2, 3, 48, 96, 2),    # Wout 48: one block and a half, split 5 of 6
    (3, 3, 40, 32, 2),    # tall and narrow
    (3, 4, 8, 224, 2),    # Wout 112: the widest input, LDS at its limit, 2 raw units per thread
]
WORKLOAD_SHAPE = (2, 2, 224, 224, 2)  # the workload's geometry: run once (u8, identity index)
ALL_SHAPES = SHAPES + [WORKLOAD_SHAPE]
IDX_KINDS = ("id", "perm", "clamp")  # None; a permutation with a repeated row; -3 and Nimg + 5
DTYPES = ("u8", "bf16", "f32", "f32_affine")
WKINDS = ("small", "large")
TOTAL2 = 4096.0  # the crafted global element count of the global-sums path
PRE_ROWS = 3     # rows of the crafted pre_slab
SKP, SKH, GK, GONE, KDEF = 176, 192, 192, 93, 168  # the kernel's layout constants


REFUSED_SIZES = [(6, 32), (10, 32), (32, 48), (32, 256)]  # H < 8, H % 4, W % 32, W > 224


def stem_supported(H, W):
    """The sizes the fused stem takes (stem_fused_supported of the bindings)."""
    return H >= 8 and H % 4 == 0 and W % 32 == 0 and W <= 224


def shape_id(s):
    return "b%d_n%d_%dx%d_g%d" % tuple(s)


def grids_of(shape):
    return sorted({1, shape[4], shape[0]})


def pow2_m(shape):
    """M = B (H/2) (W/2) is a power of two: the local coefficients (1 / M in fp32) are exact."""
    M = shape[0] * (shape[2] // 2) * (shape[3] // 2)
    return M & (M - 1) == 0


POW2_SHAPES = [s for s in SHAPES if pow2_m(s)]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _choice(g, values, shape):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


# ------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def idx_vector(shape, kind):
    """The batch's row index (int64 [B]) or None; out-of-range values are clamped by the kernels."""
    B, Nimg = shape[0], shape[1]
    if kind == "id":
        return None
    g = _gen("idx", shape, kind)
    idx = torch.randperm(Nimg, generator=g)[:B].clone()
    if kind == "perm":
        idx[B - 1] = idx[0]  # a repeated row
    else:
        idx[0], idx[B - 1] = -3, Nimg + 5
    return idx


def gathered_rows(shape, kind):
    """The image row of every batch row, clamped to [0, Nimg - 1] as the kernels clamp."""
    idx = idx_vector(shape, kind)
    if idx is None:
        return torch.arange(shape[0])
    return idx.clamp(0, shape[1] - 1)


@functools.lru_cache(maxsize=None)
def image_bank(shape):
    """The normalised images [Nimg][H][W][3]: integers in [-2, 2]; a constant patch of +-2 over a
    quarter of every image lets dense weights drive |y| past 256, where its bf16 rounding
    matters (shared: do not modify)."""
    B, Nimg, H, W, _ = shape
    g = _gen("img", shape)
    x = _randint(g, -2, 2, (Nimg, H, W, 3))
    for n in range(Nimg):
        y0 = int(torch.randint(0, H // 2 + 1, (1,), generator=g))
        x0 = int(torch.randint(0, W // 2 + 1, (1,), generator=g))
        x[n, y0:y0 + H // 2, x0:x0 + W // 2, :] = 2.0 if n % 2 == 0 else -2.0
    return x


AFFINE_NSC, AFFINE_NBI = [0.5, 0.5, 0.5], [1.0, 0.0, -1.0]


def raw_image(shape, dtype):
    """(raw [Nimg][H][W][3], nsc, nbi): the stored image whose normalisation raw * nsc[c] + nbi[c]
    is image_bank(shape), one encoding per input type of the kernels."""
    x = image_bank(shape)
    if dtype == "u8":  # [0, 4]
        return (x + 2).to(torch.uint8), [1.0] * 3, [-2.0] * 3
    if dtype == "bf16":
        return x.to(torch.bfloat16), [1.0] * 3, [0.0] * 3
    if dtype == "f32":
        return x.clone(), [1.0] * 3, [0.0] * 3
    assert dtype == "f32_affine"  # even integers: a wrong channel's bias shows
    return 2 * (x - torch.tensor(AFFINE_NBI)), list(AFFINE_NSC), list(AFFINE_NBI)


def normalised(raw, nsc, nbi):
    return raw.double() * torch.tensor(nsc, dtype=torch.float64) + torch.tensor(nbi, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def weights(kind):
    """OIHW [64][3][7][7].  small: {-1, 0, 1}, about a quarter non-zero.  large: dense integers in
    [-3, 3]; four channels of one sign each, so the constant patches give |y| of several hundred."""
    g = _gen("w", kind)
    if kind == "small":
        return _choice(g, [-1.0, 1.0], (64, 3, 7, 7)) * (torch.rand(64, 3, 7, 7, generator=g) < 0.25)
    w = _randint(g, -3, 3, (64, 3, 7, 7))
    w[2], w[9], w[34], w[37] = 3.0, -3.0, 3.0, -2.0
    return w


def gamma_fwd():
    """The BN weight whose sign picks max or min pooling: positive, negative, +0.0 and -0.0 (both
    zeros pool with max); negatives in both halves of a channel pair and both 32-channel blocks."""
    g = _gen("gamma")
    ga = _choice(g, [2.0, 1.0, -1.0, -2.0, 0.0, -0.0], (64,))
    for c, v in ((0, -1.0), (3, -2.0), (34, -1.0), (37, -2.0), (5, 0.0), (6, -0.0), (40, -0.0),
                 (41, 0.0), (2, 1.0), (9, 2.0)):
        ga[c] = v
    return ga


# ------------------------------------------------------------------ float64 references
def bf16_round(v):
    """Round to nearest even to bf16 (through fp32, exact for |integers| < 2^24), as float64."""
    return v.float().to(torch.bfloat16).double()


def ref_pack_weights(w):
    """wk[co][ky*24 + kx*3 + c] = w[co][c][ky][kx]; zeros at kx*3 + c >= 21 and k >= 168."""
    wk = torch.zeros(64, SKP, dtype=torch.float64)
    for ky in range(7):
        for kx in range(7):
            for c in range(3):
                wk[:, ky * 24 + kx * 3 + c] = w[:, c, ky, kx].double()
    return wk


def ref_conv(x, w):
    """y[n, oy, ox, co] = sum_{ky, kx, c} x[n, 2oy - 3 + ky, 2ox - 3 + kx, c] w[co, c, ky, kx]."""
    B, H, W, _ = x.shape
    Ho, Wo = H // 2, W // 2
    xp = torch.nn.functional.pad(x.double(), (0, 0, 3, 3, 3, 3))
    wd = w.double()
    y = torch.zeros(B, Ho, Wo, 64, dtype=torch.float64)
    for ky in range(7):
        for kx in range(7):
            y += xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, :] @ wd[:, :, ky, kx].t()
    return y


def nibble(kh, kw):
    """The window code of position (kh, kw): the kernel's tie-break rank."""
    return (2 - kh) << 2 | (2 - kw)


def ref_pool(yb, gamma):
    """3x3/s2/p1 pooling of yb [B][Ho][Wo][64] over the in-image positions: the first maximum in
    (kh, kw) scan order, the first minimum where gamma < 0.  Returns the extremum, its code
    nibble, and whether two or more positions of the window hold the extremum."""
    B, Ho, Wo, C = yb.shape
    PH, PW = Ho // 2, Wo // 2
    sgn = torch.where(gamma < 0, -1.0, 1.0).double()  # gamma < 0 is false for both zeros
    ninf = float("-inf")
    zp = torch.full((B, Ho + 1, Wo + 1, C), ninf, dtype=torch.float64)  # row / column -1
    zp[:, 1:, 1:] = yb * sgn
    best = torch.full((B, PH, PW, C), ninf, dtype=torch.float64)
    code = torch.zeros(B, PH, PW, C, dtype=torch.long)
    win = [(kh, kw, zp[:, kh:kh + 2 * PH:2, kw:kw + 2 * PW:2]) for kh in range(3) for kw in range(3)]
    for kh, kw, v in win:
        first = v > best  # strictly greater: an equal later position never replaces the first
        best = torch.where(first, v, best)
        code = torch.where(first, torch.full_like(code, nibble(kh, kw)), code)
    hits = sum((v == best).long() for _, _, v in win)
    return sgn * best + 0.0, code, hits >= 2  # + 0.0: a zero extremum is +0.0


def pack_nibbles(code):
    """[..., 64] nibbles -> [..., 32] bytes, channel 2k in the low nibble of byte k."""
    c = code.to(torch.uint8)
    return c[..., 0::2] | (c[..., 1::2] << 4)


def unpack_nibbles(b):
    return torch.stack((b & 15, b >> 4), dim=-1).flatten(-2).long()


def ref_pool_apply(pext, code, scale, shift):
    """out = bf16(relu(scale * pext + shift)); code4 = code where that is > 0, else 15."""
    z = pext.double() * scale.double() + shift.double()
    return bf16_round(torch.where(z > 0, z, 0.0)), torch.where(z > 0, code, torch.full_like(code, 15))


def ref_dz(g, code4, Ho, Wo):
    """The pooled gradient routed to the conv pixel its window's code names (15: nowhere)."""
    B, PH, PW, C = g.shape
    dzp = torch.zeros(B, Ho + 1, Wo + 1, C, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            dzp[:, kh:kh + 2 * PH:2, kw:kw + 2 * PW:2] += g.double() * (code4 == nibble(kh, kw))
    return dzp[:, 1:, 1:].contiguous()


def ref_im2col(x):
    """X [B][Ho][Wo][168]: column ky*24 + kx*3 + c is tap (ky, kx, c) for kx*3 + c < 21; column
    ky*24 + 21 is 1 where input row 2oy - 3 + ky lies in the image; ky*24 + 22, 23 are 0."""
    B, H, W, _ = x.shape
    Ho, Wo = H // 2, W // 2
    xp = torch.nn.functional.pad(x.double(), (0, 0, 3, 3, 3, 3))
    X = torch.zeros(B, Ho, Wo, KDEF, dtype=torch.float64)
    oy = torch.arange(Ho)
    for ky in range(7):
        for kx in range(7):
            X[..., ky * 24 + kx * 3:ky * 24 + kx * 3 + 3] = xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, :]
        iy = 2 * oy - 3 + ky
        X[..., ky * 24 + 21] = ((iy >= 0) & (iy < H)).double().view(1, Ho, 1)
    return X


def dw_of_k(v):
    """[64][>= 168] in the kernel's k order -> OIHW [64][3][7][7]."""
    dw = torch.zeros(64, 3, 7, 7, dtype=torch.float64)
    for ky in range(7):
        for kx in range(7):
            for c in range(3):
                dw[:, c, ky, kx] = v[:, ky * 24 + kx * 3 + c]
    return dw


def upper_blocks():
    """[192][192] mask of G's defined part: upper-triangle 32-blocks, both indices < 168."""
    i = torch.arange(GK)
    return ((i.view(-1, 1) // 32) <= (i.view(1, -1) // 32)) & (i.view(-1, 1) < KDEF) & (i.view(1, -1) < KDEF)


# ------------------------------------------------------------------ the cases' references
@functools.lru_cache(maxsize=None)
def gathered_x(shape, kind):
    return image_bank(shape).index_select(0, gathered_rows(shape, kind)).double()


@functools.lru_cache(maxsize=None)
def fwd_refs(shape, kind, wkind):
    """Every reference of one forward case (shared: do not modify)."""
    r = SimpleNamespace()
    r.x = gathered_x(shape, kind)
    r.y = ref_conv(r.x, weights(wkind))
    r.yb = bf16_round(r.y)
    r.pext, r.code, r.tie = ref_pool(r.yb, gamma_fwd())
    r.stats = torch.stack([r.y.sum((0, 1, 2)), (r.y * r.y).sum((0, 1, 2))])  # of y, not of bf16(y)
    return r


@functools.lru_cache(maxsize=None)
def coef_case():
    """Dyadic BN operands and crafted sums: a = gamma invstd, b = -a invstd k2,
    cc = -a k1 - b mean are multiples of 1/8 of magnitude <= 2."""
    g = _gen("coef")
    c = SimpleNamespace()
    c.gamma = _choice(g, [1.0, -1.0, 0.5, -0.5], (64,))
    c.invstd = _choice(g, [0.5, 1.0], (64,))
    c.mean = _randint(g, -1, 1, (64,))
    c.k1 = _randint(g, -1, 1, (64,))
    c.k2 = _randint(g, -1, 1, (64,))
    c.a = c.gamma.double() * c.invstd.double()
    c.b = -c.a * c.invstd.double() * c.k2.double()
    c.cc = -c.a * c.k1.double() - c.b * c.mean.double()
    c.dw0 = _randint(g, -4, 4, (64, 3, 7, 7))
    c.dgamma0 = _randint(g, -4, 4, (64,))
    c.dbeta0 = _randint(g, -4, 4, (64,))
    return c


def pre_slab(M):
    """[PRE_ROWS][2][64] integers whose rows sum to (k1 M, k2 M): the pooled-domain sums."""
    c = coef_case()
    g = _gen("pre", M)
    s = _randint(g, -50, 50, (PRE_ROWS, 2, 64))
    s[PRE_ROWS - 1] = torch.stack([c.k1, c.k2]) * M - s[:PRE_ROWS - 1].sum(0)
    return s


@functools.lru_cache(maxsize=None)
def bwd_refs(shape, kind):
    """Every reference of one backward case, on the small weights (shared: do not modify).  The
    codes are the forward reference's through ref_pool_apply with integer scale / shift, so the
    backward is tested on reference inputs, not on the forward kernel's outputs."""
    B, Nimg, H, W, _ = shape
    Ho, Wo = H // 2, W // 2
    f, c = fwd_refs(shape, kind, "small"), coef_case()
    g = _gen("bwd", shape, kind)
    r = SimpleNamespace(M=B * Ho * Wo)
    r.scale = gamma_fwd().clone()  # integers in [-2, 2] with zeros: the sign the pooling assumed
    r.shift = _randint(g, -3, 3, (64,))
    r.out, r.code4 = ref_pool_apply(f.pext, f.code, r.scale, r.shift)
    r.g = _randint(g, -2, 2, (B, H // 4, W // 4, 64))
    r.dz = ref_dz(r.g, r.code4, Ho, Wo)
    r.X = ref_im2col(f.x).view(-1, KDEF)
    dzm = r.dz.view(-1, 64)
    r.D = dzm.t() @ r.X
    r.G = r.X.t() @ r.X
    r.wk = ref_pack_weights(weights("small"))[:, :KDEF]
    r.WG = r.wk @ r.G
    r.terms = (c.a[:, None] * r.D, c.b[:, None] * r.WG, c.cc[:, None] * r.G[GONE][None, :])
    r.d = dw_of_k(sum(r.terms))  # the gradient one call adds
    # the sums of the terms' absolute values (what bounds every partial sum)
    Xa = r.X.abs()
    r.D_abs = dzm.abs().t() @ Xa
    r.G_abs = Xa.t() @ Xa
    r.WG_abs = r.wk.abs() @ r.G.abs()
    return r


def want_dw(r, wbeta, calls=1):
    return wbeta * coef_case().dw0.double() + calls * r.d if wbeta else r.d


# ------------------------------------------------------------------ stem_pool_apply alone
APPLY_SHAPES = [(1, 3, 5, 64), (3, 7, 11, 64)]  # 120 chunks: below one 1024-chunk block; 1848: 1.8


@functools.lru_cache(maxsize=None)
def apply_case(shape):
    """pext integers exact in bf16 up to 192 (scale * pext + shift then needs rounding), every
    window code, integer scale in [-2, 2] and shift in [-3, 3]: many z are exactly 0."""
    g = _gen("apply", shape)
    c = SimpleNamespace()
    c.pext = _randint(g, -3, 3, shape) * _choice(g, [1.0, 1.0, 1.0, 32.0, 64.0], shape)
    c.code = _choice(g, [float(nibble(kh, kw)) for kh in range(3) for kw in range(3)], shape).long()
    c.scale = _randint(g, -2, 2, (64,))
    c.shift = _randint(g, -3, 3, (64,))
    c.scale[:4] = torch.tensor([0.0, -1.0, 2.0, -0.0])
    c.shift[:4] = torch.tensor([1.0, 2.0, -2.0, 0.0])
    c.out, c.code4 = ref_pool_apply(c.pext, c.code, c.scale, c.shift)
    c.z = c.pext.double() * c.scale.double() + c.shift.double()
    return c
