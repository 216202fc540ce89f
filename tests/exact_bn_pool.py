"""Element-exact references for the BatchNorm and pooling kernels (csrc/bn_pool.hip).

Tier A: operands are small integers and dyadic coefficients, so every intermediate of a kernel
is exactly representable; accumulation order, FMA contraction and the order of the fixed-order
reduces cannot change a result, which must equal the float64 reference bit for bit.  Tier B
(whole backward at an M that is no power of two) keeps the two sums exact and bounds dy element
by element.  This module draws the operands (*_case), computes the float64 references from
explicit loops over window taps (ref_*; never a library pooling or batch-norm call), asserts the
conditions under which exactness holds (*_preconditions) and holds the compare functions.
The references are device-agnostic torch code; the module never calls the code under test."""
import functools
import math
from types import SimpleNamespace

import torch

from exact_conv import pack_bits  # noqa: F401  (the kernels' 1-bit mask layout)

LIM_FP32 = 1 << 24
EPS = 1e-5
MOMENTUM = 0.1
SCALES = [1.0, -1.0, 2.0, 0.5, -0.5]

# ------------------------------------------------------------------ the cases
# (M, C): chunk counts around one and two 1024-chunk blocks of the flat streaming kernels,
# C8 = 1 (RL = 256) and C8 = 256 (RL = 1), partial blocks
APPLY_SHAPES = [(1, 8), (1023, 8), (1024, 8), (1025, 8), (2305, 8), (128, 64), (129, 64),
                (5, 2048), (3, 512)]
# (M, C) of the backward sums: one group / two groups of bn_bwd_groups, G = 258 (the <256, 4>
# finalize) and the G = 2048 cap
SUMS_SHAPES = [(1, 8), (4096, 8), (4097, 8), (512, 64), (513, 64), (37, 64), (64, 512),
               (65, 512), (16, 2048), (17, 2048), (4113, 2048)]
SUMS_SHAPE_BIG = (32785, 2048)
PRE_ROWS = [1, 256, 257, 2048, 2049]  # 16- / 4-channel finalize, the slab_colsum pre-pass
# (N, H, W, C, K, S, P)
MAXPOOL_GEOMS = [(2, 1, 1, 8, 3, 2, 1), (2, 5, 4, 24, 3, 2, 1), (1, 4, 7, 64, 3, 2, 1),
                 (2, 6, 6, 8, 2, 2, 0), (1, 5, 5, 16, 3, 1, 1)]
FUSED_HW = [(1, 1), (2, 2), (3, 3), (4, 6), (5, 4), (9, 14), (7, 2)]
FUSED_KSP = [(3, 2, 1), (2, 2, 0), (3, 1, 1)]
FUSED_GEOMS = [(2, H, W, C, K, S, P) for (H, W) in FUSED_HW for C in (8, 64)
               for (K, S, P) in FUSED_KSP if H + 2 * P >= K and W + 2 * P >= K]
AVG_HW = [1, 6, 7, 8, 13, 14, 15, 49]  # around the unroll-by-7 loop
AVG_C = [8, 24, 512]
STAT_T = [1, 7, 8, 9, 255, 256, 257, 2048, 2049, 8200]
STAT_C = [8, 24, 64, 512]
# mode 3: (N, H, W, K, S, P); even H and W with 3/2/1 take the quad kernels (38 x 54: 513 quads)
MODE3_QUAD = [(2, 2, 2, 3, 2, 1), (1, 4, 6, 3, 2, 1), (2, 6, 4, 3, 2, 1), (1, 38, 54, 3, 2, 1)]
MODE3_PIXEL = [(2, 3, 3, 3, 2, 1), (1, 5, 4, 3, 2, 1), (1, 4, 5, 3, 2, 1), (2, 7, 9, 3, 2, 1)]
MODE3_OTHER = [(1, 5, 5, 2, 2, 0), (1, 5, 5, 3, 1, 1)]  # K <= 2S fast path, general loop
MODE3_GEOMS = MODE3_QUAD + MODE3_PIXEL + MODE3_OTHER
TIERB_SHAPES = [(37, 64), (1000, 64), (513, 512), (17, 2048), (4097, 8)]
TIERB_MODE3 = [(2, 7, 9, 3, 2, 1), (1, 6, 4, 3, 2, 1)]
EVAL_C = [1, 8, 24, 64, 512, 1000]
TOTAL2 = 4096.0  # the crafted global element count of the stage-2 cases


def pool_out(H, W, K, S, P):
    return (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1


# ------------------------------------------------------------------ operands
def _gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device).float()


def _choice(g, values, shape):
    v = torch.tensor(values, dtype=torch.float32, device=g.device)
    return v[torch.randint(0, len(values), shape, generator=g, device=g.device)]


def _seed(*key):
    return (hash(tuple(int(k * 2) if isinstance(k, float) else int(k) for k in key)) & 0x7FFFFFF) + 11


@functools.lru_cache(maxsize=None)
def bn_case(M, C, device="cpu", seed=0):
    """Operands of one (M, C) BatchNorm case: the forward apply, both backward stages and the
    whole backward (fp32 tensors holding the values; shared: do not modify).  Channel 0 of row
    0 gives an exact zero before the ReLU and channel 1 a negative value, with and without the
    residual."""
    g = _gen(_seed(M, C, seed), device)
    c = SimpleNamespace(M=M, C=C)
    c.y = _randint(g, -8, 8, (M, C))
    c.res = _randint(g, -8, 8, (M, C))
    c.dout = _randint(g, -4, 4, (M, C))
    c.scale = _choice(g, SCALES, (C,))
    c.shift = _randint(g, -4, 4, (C,))
    c.y[0, 0], c.res[0, 0], c.shift[0] = 0.0, 0.0, 0.0
    c.y[0, 1], c.res[0, 1], c.scale[1], c.shift[1] = -8.0, 0.0, 1.0, 0.0
    c.mean = _randint(g, -2, 2, (C,))
    c.invstd = _choice(g, [0.5, 1.0, 2.0], (C,))
    c.dg0 = _randint(g, -4, 4, (C,))  # prior contents of the gradient slots
    c.db0 = _randint(g, -4, 4, (C,))
    # stage 2: crafted global sums k * total, dyadic gamma and invstd
    c.k1 = _randint(g, -1, 1, (C,))
    c.k2 = _randint(g, -1, 1, (C,))
    c.gamma2 = _choice(g, [1.0, -1.0, 2.0], (C,))
    c.invstd2 = _choice(g, [0.5, 1.0], (C,))
    # tier B: an inexact gamma (the stored fp32 value is the operand)
    c.gamma = torch.rand(C, generator=g, device=g.device) + 0.5
    c.invstdB = _choice(g, [0.5, 1.0, 2.0], (C,))
    return c


@functools.lru_cache(maxsize=None)
def pool_case(geom, seed=0):
    """Operands of one pooling geometry: x with frequent ties, dy, and a random code tensor
    over 0..K*K-1 that is independent of x (a pixel can then win every window over it)."""
    N, H, W, C, K, S, P = geom
    OH, OW = pool_out(H, W, K, S, P)
    g = _gen(_seed(*geom, seed))
    c = SimpleNamespace(geom=geom)
    c.x = _randint(g, -3, 3, (N, H, W, C))
    c.dy = _randint(g, -8, 8, (N, OH, OW, C))
    c.codes = torch.randint(0, K * K, (N, OH, OW, C), generator=g).to(torch.uint8)
    # BN + ReLU in front of the pool (the fused stem tail)
    c.y = _randint(g, -8, 8, (N, H, W, C))
    c.scale = _choice(g, SCALES, (C,))
    c.shift = _randint(g, -4, 4, (C,))
    c.y[0, 0, 0, 0], c.shift[0] = 0.0, 0.0
    c.y[0, 0, 0, 1], c.scale[1], c.shift[1] = -8.0, 1.0, 0.0
    return c


@functools.lru_cache(maxsize=None)
def mode3_case(geom, C, seed=0):
    """A BN backward through a following max pool: y [N][H][W][C], the pooled gradient and a
    random code tensor over {0..K*K-1, 15}, independent of y."""
    N, H, W, K, S, P = geom
    OH, OW = pool_out(H, W, K, S, P)
    c = bn_case(N * H * W, C, "cpu", seed + 7 * (K * 16 + S * 4 + P) + 1000 * W)
    c = SimpleNamespace(**vars(c))
    g = _gen(_seed(*geom, C, seed, 3))
    # K <= 2S: a pixel lies in at most 4 windows; the 3x3/s1 case in 9, so smaller gradients
    # keep dy = a*dz + b*y + c within 256 steps of its granularity
    lim = 4 if K <= 2 * S else 1
    c.geom, c.pdy = geom, _randint(g, -lim, lim, (N, OH, OW, C))
    pick = torch.tensor(list(range(K * K)) + [15], dtype=torch.uint8)
    c.codes = pick[torch.randint(0, K * K + 1, (N, OH, OW, C), generator=g)]
    return c


def tierb_of(c, seed=0):
    """The tier-B variant of a case: y redrawn as integers with 3|mean| <= |y| <= 8 per
    channel (any y where the mean is 0), everything else kept.

    Why: c = -a*s/M - b*mean can cancel (exactly, when s = invstd*q*mean), and then the fp32
    rounding of its two terms, up to 3 * 2^-24 * (|a*s/M| + |b*mean|) <= 2^-24 * (3|c| + 6|b*mean|),
    is not covered by a budget in |c|.  The other roundings of dy = a*dz + b*y + c cost at most
    2^-24 * (3|a*dz| + 6|b*y| + 3|c|) (a is exact: invstd is a power of two), so the bound's
    8 * 2^-24 * (|a*dz| + |b*y| + |c|) holds for every contraction order once
    6|b*mean| <= 2|b*y|, i.e. |y| >= 3|mean|."""
    t = SimpleNamespace(**vars(c))
    g = _gen(_seed(c.M, c.C, seed, 21), c.y.device)
    lo = (3 * c.mean.abs()).expand(c.M, c.C)
    mag = lo + torch.floor(torch.rand(c.M, c.C, generator=g, device=g.device) * (9 - lo))
    t.y = mag * _choice(g, [-1.0, 1.0], (c.M, c.C))
    assert (t.y.abs() >= lo).all() and float(t.y.abs().max()) <= 8 and torch.equal(t.y, t.y.round())
    return t


@functools.lru_cache(maxsize=None)
def avg_case(HW, C, seed=0):
    N = 3
    g = _gen(_seed(HW, C, seed, 5))
    return SimpleNamespace(x=_randint(g, -8, 8, (N, HW, C)), g=_randint(g, -8, 8, (N, C)), HW=HW)


@functools.lru_cache(maxsize=None)
def stat_case(T, C, seed=0):
    """An integer statistics slab [T][2][C] (sums in [0, 8], squares in [0, 64]) of 8 elements
    per row, with dyadic gamma (scale = gamma * invstd is then one rounding), integer beta and
    running statistics."""
    g = _gen(_seed(T, C, seed, 9))
    c = SimpleNamespace(T=T, C=C, count=8.0 * T)
    c.slab = torch.stack([_randint(g, 0, 8, (T, C)), _randint(g, 0, 64, (T, C))], 1).contiguous()
    c.gamma = _choice(g, SCALES, (C,))
    c.beta = _randint(g, -4, 4, (C,))
    c.rmean = _randint(g, -4, 4, (C,))
    c.rvar = _randint(g, 1, 4, (C,))
    return c


def pre_slab_case(rows, C, seed=0):
    """Pre-reduced partial rows [rows][2C] of a backward: integers in [-8, 8]."""
    g = _gen(_seed(rows, C, seed, 13))
    return _randint(g, -8, 8, (rows, 2 * C))


# ------------------------------------------------------------------ float64 references
def ref_apply(y, scale, shift, res=None, relu=True):
    """[relu](y * scale + shift [+ res]) per channel (last axis), float64."""
    v = y.double() * scale.double() + shift.double()
    if res is not None:
        v = v + res.double()
    return torch.relu(v) if relu else v


def _taps(H, W, K, S, P):
    OH, OW = pool_out(H, W, K, S, P)
    for kh in range(K):
        for kw in range(K):
            yield kh * K + kw, slice(kh, kh + S * (OH - 1) + 1, S), slice(kw, kw + S * (OW - 1) + 1, S)


def _pad_hw(a, p, value):
    return torch.nn.functional.pad(a, (0, 0, p, p, p, p), value=value)


def ref_maxpool_fwd(v, K, S, P, raw=None):
    """Window maximum of v [N][H][W][C] scanned in (kh, kw) order with a strict '>' (the first
    maximum wins; taps outside the image never win), its code kh*K + kw, and optionally `raw`
    at the winning tap.  float64 / int64."""
    N, H, W, C = v.shape
    OH, OW = pool_out(H, W, K, S, P)
    vp = _pad_hw(v.double(), P, -math.inf)
    rp = None if raw is None else _pad_hw(raw.double(), P, 0.0)
    best = torch.full((N, OH, OW, C), -math.inf, dtype=torch.float64)
    code = torch.zeros(N, OH, OW, C, dtype=torch.int64)
    arg = torch.zeros(N, OH, OW, C, dtype=torch.float64)
    for k, ys, xs in _taps(H, W, K, S, P):
        t = vp[:, ys, xs, :]
        win = t > best
        best = torch.where(win, t, best)
        code = torch.where(win, torch.full_like(code, k), code)
        if rp is not None:
            arg = torch.where(win, rp[:, ys, xs, :], arg)
    return (best, code) if raw is None else (best, code, arg)


def ref_fused_pool(y, scale, shift, K, S, P):
    """maxpool(relu(y*scale + shift)): pooled values, codes (15 where the window maximum is 0:
    no gradient passes) and the raw y at the winning tap."""
    best, code, arg = ref_maxpool_fwd(ref_apply(y, scale, shift), K, S, P, raw=y)
    return best, torch.where(best > 0, code, torch.full_like(code, 15)), arg


def ref_pool_gather(dy, codes, H, W, K, S, P):
    """dx[n, ih, iw, c] = the sum of dy over the windows (oh, ow) that contain (ih, iw) and whose
    code names it: code == (ih - (oh*S - P)) * K + (iw - (ow*S - P)).  Codes that name a
    position outside the image, or no window position, pass nothing.  float64."""
    N, OH, OW, C = dy.shape
    assert (OH, OW) == pool_out(H, W, K, S, P)
    dxp = torch.zeros(N, H + 2 * P + S, W + 2 * P + S, C, dtype=torch.float64, device=dy.device)
    d, cd = dy.double(), codes.long()
    for k, ys, xs in _taps(H, W, K, S, P):
        dxp[:, ys, xs, :] += d * (cd == k)
    return dxp[:, P:P + H, P:P + W, :].clone()


def ref_avg_fwd(x):
    """x [N][HW][C] -> the exact integer sum, one IEEE fp32 division, RNE to bf16.  (A float64
    quotient of two integers below 2^24 rounds to fp32 as the fp32 division does.)"""
    HW = x.shape[1]
    return (x.double().sum(1) / HW).float().bfloat16().double()


def ref_avg_bwd(g, HW):
    """g [N][C] -> g * fp32(1 / HW) rounded to fp32 (the product of an 8-bit and a 24-bit
    significand is exact in float64), then RNE to bf16, for each of the HW pixels."""
    inv = (torch.ones((), dtype=torch.float32) / HW).double()
    v = (g.double() * inv).float().bfloat16().double()
    return v[:, None, :].expand(g.shape[0], HW, g.shape[1])


def f32(v):
    """The float64 value of an fp32 number (of a Python float rounded to fp32)."""
    return float(torch.tensor(v, dtype=torch.float32))


def ref_finalize(S, Q, count, gamma, beta, rmean=None, rvar=None):
    """The forward finalize from exact column sums S, Q (float64), as one float64 expression
    per result: mean, invstd, scale, shift, running mean / var (momentum 0.1, unbiased variance
    unless count == 1).  eps and momentum are the fp32 values the kernels receive."""
    mean = S / count
    return ref_finalize_mv(mean, (Q / count - mean * mean).clamp_min(0), count, gamma, beta, rmean, rvar)


def ref_finalize_mv(mean, var, count, gamma, beta, rmean=None, rvar=None):
    """ref_finalize from the batch mean and biased variance (float64)."""
    r = SimpleNamespace(mean=mean, var=var)
    eps, m = f32(EPS), f32(MOMENTUM)
    r.invstd = 1.0 / torch.sqrt(r.var + eps)
    r.scale = gamma.double() * r.invstd
    r.shift_terms = torch.maximum(beta.double().abs(), (r.mean * r.scale).abs())
    r.shift = beta.double() - r.mean * r.scale
    if rmean is not None:
        unb = r.var * count / (count - 1) if count > 1 else r.var
        t0, t1 = (1 - m) * rmean.double(), m * r.mean
        r.rmean, r.rmean_terms = t0 + t1, torch.maximum(t0.abs(), t1.abs())
        t0, t1 = (1 - m) * rvar.double(), m * unb
        r.rvar, r.rvar_terms = t0 + t1, torch.maximum(t0.abs(), t1.abs())
    return r


def ref_sync_row(S, Q, count):
    """bn_sync_local's row [mean (C) | M2 (C) | n], float64."""
    m2 = (Q - S * S / count).clamp_min(0)
    return torch.cat([S / count, m2, torch.tensor([count], dtype=torch.float64)])


def ref_sync_merge(rows):
    """bn_sync_finalize's merge of the rows [ws][2C+1] in rank order: (mean, var, N)."""
    C = (rows.shape[1] - 1) // 2
    N = sum(float(r[2 * C]) for r in rows)
    mean = sum(float(r[2 * C]) * r[:C] for r in rows) / N
    M2 = sum(r[C:2 * C] + float(r[2 * C]) * (r[:C] - mean) ** 2 for r in rows)
    return mean, M2 / N, N


def keep_of(c, mode):
    """The ReLU mask of a backward mode: 0 none; 1 / 4 from the residual layer's stored
    output (out > 0, the bn_apply *reference*); 2 / 3 recomputed from y."""
    if mode == 0:
        return torch.ones_like(c.y, dtype=torch.bool)
    if mode in (1, 4):
        return ref_apply(c.y, c.scale, c.shift, res=c.res) > 0
    return ref_apply(c.y, c.scale, c.shift) > 0


def ref_dz(c, mode):
    """The ReLU-masked upstream gradient [M][C], float64 (mode 3: gathered from the pool)."""
    if mode == 3:
        N, H, W, K, S, P = c.geom
        d = ref_pool_gather(c.pdy, c.codes, H, W, K, S, P).reshape(c.M, c.C)
    else:
        d = c.dout.double()
    return d * keep_of(c, mode)


def ref_bwd_sums(dz, y, mean, invstd, absolute=False):
    """[sum dz, sum dz * (y - mean) * invstd] per channel -> [2][C]; absolute: of the terms'
    magnitudes."""
    t = dz * (y.double() - mean.double()) * invstd.double()
    if absolute:
        dz, t = dz.abs(), t.abs()
    return torch.stack([dz.sum(0), t.sum(0)])


def ref_grads(sums, c, gbeta):
    """dgamma, dbeta = gbeta * prior + sums (gbeta 0 discards the prior)."""
    return gbeta * c.dg0.double() + sums[1], gbeta * c.db0.double() + sums[0]


def ref_coef2(c):
    """Stage-2 coefficients from the crafted sums k * total: a, b, c exact dyadic numbers."""
    a = c.gamma2.double() * c.invstd2.double()
    b = -a * c.invstd2.double() * c.k2.double()
    return a, b, -a * c.k1.double() - b * c.mean.double()


def ref_coef(sums, M, gamma, mean, invstd):
    """The whole backward's coefficients from the stored fp32 gamma, mean, invstd, float64."""
    a = gamma.double() * invstd.double()
    b = -a * invstd.double() * sums[1] / M
    return a, b, -a * sums[0] / M - b * mean.double()


# ------------------------------------------------------------------ ulps and bounds
def ulp(v, bits):
    """The spacing of the `bits`-significand format at |v| (0 at v == 0), float64."""
    v = v.double().abs()
    e = torch.floor(torch.log2(torch.where(v > 0, v, torch.ones_like(v))))
    return torch.where(v > 0, torch.exp2(e - (bits - 1)), torch.zeros_like(v))


def assert_ulps(got, want, n, what, of=None):
    """|got - want| <= n fp32 ulps of `of` (default: of want), element by element."""
    g, w = got.detach().double().cpu(), want.double().cpu()
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}"
    tol = n * ulp(w if of is None else of.double().cpu(), 24)
    bad = ((g - w).abs() > tol) | torch.isnan(g)
    if bad.any():
        i = int(bad.nonzero()[0])
        worst = ((g - w).abs() / tol.clamp_min(1e-300)).max().item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements off by more than {n} "
                             f"fp32 ulps (worst {worst * n:.2f}); first at {i}: got {g[i].item()!r} "
                             f"want {w[i].item()!r}")


def tierb_bound(a, b, cc, dz, y):
    """ref = a*dz + b*y + c and the bound ulp_bf16(ref)/2 + 8 * 2^-24 * (|a*dz| + |b*y| + |c|):
    the final RNE rounding plus eight fp32 roundings on the term magnitudes."""
    t0, t1 = a * dz, b * y.double()
    ref = t0 + t1 + cc
    return ref, ulp(ref, 8) / 2 + 8 * 2.0 ** -24 * (t0.abs() + t1.abs() + cc.abs())


def assert_within(got, ref, bound, what):
    g = got.detach().double().cpu().reshape(ref.shape)
    err = (g - ref.cpu()).abs()
    bad = (err > bound.cpu()) | torch.isnan(g)
    if bad.any():
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements outside the bound "
                             f"(worst ratio {(err / bound.cpu()).max().item():.3f}); first at {idx}: got "
                             f"{g[tuple(idx)].item()!r} ref {ref[tuple(idx)].item()!r}")
    return (err / bound.cpu().clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------ preconditions
def _need_bf16(name, v):
    """Every value is a bf16 number (8 significand bits)."""
    v = v.double()
    assert torch.equal(v.float().bfloat16().double(), v), f"{name}: not representable in bf16"
    return float(v.abs().max())


def _need_fp32_sum(name, v, abs_terms, gran):
    """Sums whose terms are multiples of `gran`: every partial sum in any order is an exact fp32
    number when the sum of the terms' magnitudes stays below 2^24 granules."""
    v, a, gran = v.double(), abs_terms.double(), gran.double()
    assert torch.equal(v / gran, (v / gran).round()), f"{name}: not a multiple of its granularity"
    assert (a >= v.abs()).all()
    m = float((a / gran).max())
    assert m < LIM_FP32, f"{name}: sum of |terms| = {m} granules >= 2^24"
    return m


def apply_preconditions(c):
    seen = {}
    for n in ("y", "res", "scale", "shift"):
        _need_bf16(n, getattr(c, n))
    for res in (None, c.res):
        pre = ref_apply(c.y, c.scale, c.shift, res=res, relu=False)
        seen["out"] = max(seen.get("out", 0), _need_bf16("bn_apply out", pre))
        assert (pre == 0).any() and (pre < 0).any(), "exact zeros and negatives must occur"
    return seen


def sums_preconditions(c, modes=(0, 1, 2, 4), invstd=None):
    """The backward sums and the gradients built on them are exact in fp32 in any order."""
    seen = {}
    invstd = c.invstd if invstd is None else invstd
    gran = torch.minimum(invstd, torch.ones_like(invstd)).double()
    for n in ("y", "dout", "mean", "dg0", "db0"):
        _need_bf16(n, getattr(c, n))
    assert set(invstd.unique().tolist()) <= {0.5, 1.0, 2.0}
    for mode in modes:
        dz = ref_dz(c, mode)
        s = ref_bwd_sums(dz, c.y, c.mean, invstd)
        a = ref_bwd_sums(dz, c.y, c.mean, invstd, absolute=True) + 4  # + the prior slot
        # the kernels add d * (y - mean) * invstd term by term: the unscaled products count too
        a[1] = torch.maximum(a[1], a[1] / invstd.double())
        one = torch.ones_like(gran)
        seen[mode] = max(_need_fp32_sum(f"sum dz (mode {mode})", s[0], a[0], one / 2),
                         _need_fp32_sum(f"sum dz*xhat (mode {mode})", s[1], a[1], gran / 2))
    return seen


def apply2_preconditions(c, modes=(0, 1, 2, 4)):
    """Stage 2 with the crafted sums: dy = a*dz + b*y + c and dres = dz are bf16 numbers."""
    a, b, cc = ref_coef2(c)
    seen = {}
    for mode in modes:
        dz = ref_dz(c, mode)
        _need_bf16("dres", dz)
        seen[mode] = _need_bf16(f"dy (mode {mode})", a * dz + b * c.y.double() + cc)
    return seen


def pool_preconditions(c):
    N, H, W, C, K, S, P = c.geom
    seen = {"x": _need_bf16("x", c.x), "dy": _need_bf16("dy", c.dy)}
    best, code = ref_maxpool_fwd(c.x, K, S, P)
    ties = 0
    for k, ys, xs in _taps(H, W, K, S, P):
        ties += ((_pad_hw(c.x.double(), P, -math.inf)[:, ys, xs, :] == best) & (code != k)).sum().item()
    seen["ties"] = ties
    for cd in (code, c.codes.long()):
        seen["dx"] = _need_bf16("dx", ref_pool_gather(c.dy, cd, H, W, K, S, P))
    fb, fc, fa = ref_fused_pool(c.y, c.scale, c.shift, K, S, P)
    seen["fused"] = _need_bf16("fused out", fb)
    seen["code15"] = int((fc == 15).sum())
    return seen


def stat_preconditions(c):
    s = c.slab.double().sum(0)
    assert torch.equal(c.slab, c.slab.round()) and float(s.max()) < LIM_FP32
    assert float(c.slab[:, 0].max()) <= 8 and float(c.slab[:, 1].max()) <= 64
    return float(s.max())


def avg_preconditions(c):
    _need_bf16("x", c.x)
    _need_bf16("g", c.g)
    s = c.x.double().abs().sum(1)
    assert float(s.max()) < LIM_FP32
    return float(s.max())


# ------------------------------------------------------------------ fp32 emulation (tier B)
def _r32(v):
    return v.float().double()


def _fma32(a, b, c):
    return _r32(a * b + c)  # the product of two fp32 numbers is exact in float64


def emulate_whole_backward(sums, M, gamma, mean, invstd, dz, y, variant):
    """The kernels' fp32 formulas (fin_bwd_channel, bn_bwd_apply_kernel) step by step in
    float64 with a rounding to fp32 after every operation; variant 0 unfused, 1 to 3 ways the
    compiler may contract a*b + c into an FMA (3: c's first product fused into the subtraction,
    which leaves the rounding residue of b*mean where the terms of c cancel).  Returns dy
    rounded to bf16 (float64)."""
    g, mu, is_ = gamma.double(), mean.double(), invstd.double()
    s, q = _r32(sums[0]), _r32(sums[1])
    a = _r32(g * is_)
    inv_m = _r32(torch.tensor(1.0 / M, dtype=torch.float64))
    b = _r32(_r32(_r32(-a * is_) * q) * inv_m)
    t = _r32(_r32(-a * s) * inv_m)
    if variant == 3:
        cc = _fma32(_r32(-a * s), inv_m, -_r32(b * mu))
    else:
        cc = _r32(t - _r32(b * mu)) if variant == 0 else _fma32(-b, mu, t)
    yd = y.double()
    if variant in (0, 3):
        r = _r32(_r32(_r32(a * dz) + _r32(b * yd)) + cc)
    elif variant == 1:
        r = _r32(_fma32(b, yd, _r32(a * dz)) + cc)
    else:
        r = _fma32(a, dz, _fma32(b, yd, cc))
    return r.float().bfloat16().double()
