"""Preconditions and reference self-checks of the exact stem suite (tests/exact_stem.py), no GPU.

tests/test_exact_stem_gpu.py compares the fused stem's outputs with the float64 references bit
for bit.  That is only sound if every intermediate the kernels form is exactly representable
in any accumulation order; this file asserts those bounds for every case the GPU file draws
(both take their cases from exact_stem.py), that the window ties the code comparison lives on
are there, and that the references agree with independent formulations (library convolution,
library pooling, a brute-force window scan, autograd's weight gradient)."""
import pytest
import torch
import torch.nn.functional as F

import exact_stem as es
from exact_conv import LIM_BF16, LIM_FP32

CASES = [(s, k) for s in es.SHAPES for k in es.IDX_KINDS] + [(es.WORKLOAD_SHAPE, "id")]
case_id = lambda v: (es.shape_id(v) if len(v) == 5 else "x".join(map(str, v))) if isinstance(v, tuple) else str(v)
DW_UNIT = 8  # every dW term is a multiple of 1/8


def _is_int(v):
    return torch.equal(v, v.round())


def _calls(shape):
    """The most calls that accumulate into one dW: the doubled-result checks run on SHAPES."""
    return 1 if shape == es.WORKLOAD_SHAPE else 2


# ------------------------------------------------------------------ operands
@pytest.mark.parametrize("shape", es.ALL_SHAPES, ids=case_id)
def test_operands_are_small_integers_in_every_encoding(shape):
    x = es.image_bank(shape)
    assert _is_int(x) and x.abs().max() <= 2 and tuple(x.shape) == (shape[1], shape[2], shape[3], 3)
    assert es.stem_supported(shape[2], shape[3])
    for dt in es.DTYPES:
        raw, nsc, nbi = es.raw_image(shape, dt)
        assert torch.equal(es.normalised(raw, nsc, nbi), x.double()), dt
        assert torch.equal(raw.double(), raw.to(torch.bfloat16).double()), dt  # exact in bf16 too
    raw, _, _ = es.raw_image(shape, "u8")
    assert raw.dtype == torch.uint8 and raw.min() >= 0 and raw.max() <= 4
    raw, nsc, nbi = es.raw_image(shape, "f32_affine")
    assert torch.equal(raw % 2, torch.zeros_like(raw)) and len(set(nbi)) == 3
    # a bias taken from another channel changes the image
    assert not torch.equal(es.normalised(raw, nsc, nbi[1:] + nbi[:1]), x.double())


def test_weights_gamma_and_coefficients():
    ws, wl = es.weights("small"), es.weights("large")
    assert set(ws.unique().tolist()) == {-1.0, 0.0, 1.0} and 0.2 < (ws != 0).float().mean() < 0.3
    assert _is_int(wl) and wl.abs().max() == 3 and (wl != 0).float().mean() > 0.8
    ga = es.gamma_fwd()
    neg = ga < 0
    zero_bits = ga.view(torch.int32)[ga == 0].tolist()
    assert 0 in zero_bits and -(1 << 31) in zero_bits, "both +0.0 and -0.0"
    assert (ga > 0).any()
    for blk in (slice(0, 32), slice(32, 64)):  # both halves of a pair, both 32-channel blocks
        assert neg[blk][0::2].any() and neg[blk][1::2].any()
    c = es.coef_case()
    for v in (c.a, c.b, c.cc):
        assert _is_int(v * DW_UNIT) and v.abs().max() <= 2
    assert (c.a < 0).any() and (c.b != 0).any() and (c.cc != 0).any()
    for v in (c.dw0, c.dgamma0, c.dbeta0):
        assert _is_int(v) and v.abs().max() <= LIM_BF16
    # gamma * invstd, 1 / TOTAL2 and k * TOTAL2 are exact in fp32
    assert es.TOTAL2 == 2.0 ** 12


def test_index_vectors():
    for shape in es.SHAPES:
        B, Nimg = shape[0], shape[1]
        assert es.idx_vector(shape, "id") is None
        p = es.idx_vector(shape, "perm")
        assert p.dtype == torch.long and p.numel() == B and p.unique().numel() < B
        assert p.min() >= 0 and p.max() < Nimg
        cl = es.idx_vector(shape, "clamp")
        assert -3 in cl.tolist() and Nimg + 5 in cl.tolist()
        rows = es.gathered_rows(shape, "clamp")
        assert rows[0] == 0 and rows[B - 1] == Nimg - 1
    assert es.POW2_SHAPES == [(2, 2, 8, 32, 2), (4, 4, 8, 64, 1)]


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape,kind", CASES, ids=case_id)
def test_forward_preconditions(shape, kind):
    B, grid = shape[0], shape[4]
    r = es.fwd_refs(shape, kind, "small")
    assert _is_int(r.y) and r.y.abs().max() < LIM_FP32
    assert torch.equal(r.y, r.yb), "small weights: the conv output is exact in bf16"
    # the statistics: every partial sum of a workgroup (and of the whole batch, for grid = 1) is
    # an integer bounded by sum |y| <= sum y^2 < 2^24
    for wg in range(grid):
        y = r.y[wg::grid]
        s1, s2 = y.abs().sum((0, 1, 2)), (y * y).sum((0, 1, 2))
        assert (s1 <= s2).all() and s2.max() < LIM_FP32
    assert r.stats[1].max() < LIM_FP32
    # the ties the code comparison needs
    share = r.tie.float().mean().item()
    assert share >= 0.05, f"only {share:.3f} of the windows tie for the extremum"
    big = es.fwd_refs(shape, kind, "large")
    assert _is_int(big.y) and big.y.abs().max() > 2 * LIM_BF16 and big.y.abs().max() < LIM_FP32
    assert (big.y != big.yb).any(), "large weights: the bf16 rounding of y must matter"
    assert big.tie.any()
    for f in (r, big):  # every code value occurs; both pooling senses see ties
        assert set(f.code.unique().tolist()) == {es.nibble(kh, kw) for kh in range(3) for kw in range(3)}
        neg = es.gamma_fwd() < 0
        assert f.tie[..., neg].any() and f.tie[..., ~neg].any()


@pytest.mark.parametrize("shape,kind", CASES, ids=case_id)
@pytest.mark.parametrize("wkind", es.WKINDS)
def test_forward_reference_against_library_ops(shape, kind, wkind):
    r = es.fwd_refs(shape, kind, wkind)
    x = es.image_bank(shape).double()[es.gathered_rows(shape, kind)]
    y = F.conv2d(x.permute(0, 3, 1, 2), es.weights(wkind).double(), stride=2, padding=3)
    assert torch.equal(r.y, y.permute(0, 2, 3, 1))
    sgn = torch.where(es.gamma_fwd() < 0, -1.0, 1.0).double().view(1, 64, 1, 1)
    v = sgn * F.max_pool2d(sgn * r.yb.permute(0, 3, 1, 2), 3, 2, 1)
    assert torch.equal(r.pext, v.permute(0, 2, 3, 1))
    # the codes by a brute-force scan of sampled windows
    g = torch.Generator().manual_seed(5)
    B, PH, PW, C = r.code.shape
    tied = r.tie.nonzero()
    pick = tied[torch.randperm(tied.shape[0], generator=g)[:150]].tolist()
    pick += [[int(torch.randint(0, d, (1,), generator=g)) for d in (B, PH, PW, C)] for _ in range(50)]
    pick += [[0, 0, 0, c] for c in range(0, 64, 7)] + [[B - 1, PH - 1, PW - 1, c] for c in range(64)]
    Ho, Wo = 2 * PH, 2 * PW
    for n, i, j, c in pick:
        s = float(sgn[0, c, 0, 0])
        best, at = None, None
        for kh in range(3):
            for kw in range(3):
                oy, ox = 2 * i - 1 + kh, 2 * j - 1 + kw
                if 0 <= oy < Ho and 0 <= ox < Wo:
                    z = s * float(r.yb[n, oy, ox, c])
                    if best is None or z > best:
                        best, at = z, (kh, kw)
        assert int(r.code[n, i, j, c]) == es.nibble(*at) and float(r.pext[n, i, j, c]) == s * best


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("shape,kind", CASES, ids=case_id)
def test_backward_preconditions(shape, kind):
    r, c = es.bwd_refs(shape, kind), es.coef_case()
    assert _is_int(r.g) and r.g.abs().max() <= 2
    assert _is_int(r.scale) and _is_int(r.shift) and (r.scale == 0).any() and (r.scale < 0).any()
    assert (r.code4 == 15).any() and (r.code4 != 15).any()
    assert _is_int(r.out) and r.out.abs().max() <= LIM_BF16
    assert _is_int(r.dz) and r.dz.abs().max() <= LIM_BF16  # the dz tile is bf16
    assert r.dz.abs().max() >= 3, "some pixel must win several windows"
    # D, G and W G: integers, and the sums of their terms' absolute values below 2^24
    for v, a in ((r.D, r.D_abs), (r.G, r.G_abs), (r.WG, r.WG_abs)):
        assert _is_int(v) and (v.abs() <= a).all() and a.max() < LIM_FP32
    # dW: every term a multiple of 1/8, the sum of the absolute values below 2^(24 - 3)
    total = _calls(shape) * (c.a.abs()[:, None] * r.D_abs + c.b.abs()[:, None] * r.WG_abs +
                             c.cc.abs()[:, None] * r.G_abs[es.GONE][None, :])
    for t in r.terms:
        assert _is_int(t * DW_UNIT)
    assert total.max() + c.dw0.abs().max() < LIM_FP32 / DW_UNIT
    # the ones column: in-image rows only, and column 93 is all ones (the colsum row of G)
    X = r.X
    assert torch.equal(X[:, es.GONE], torch.ones(X.shape[0], dtype=torch.float64))
    for ky in range(7):
        assert set(X[:, ky * 24 + 21].unique().tolist()) <= {0.0, 1.0}
        assert not X[:, ky * 24 + 22:ky * 24 + 24].any()
    assert (X[:, 21] == 0).any() and (X[:, 6 * 24 + 21] == 0).any()  # rows above / below the image
    # the local path: sums of k M, exact for M a power of two
    if es.pow2_m(shape):
        ps = es.pre_slab(r.M)
        assert _is_int(ps) and ps.abs().max() < LIM_FP32
        assert torch.equal(ps.double().sum(0), torch.stack([c.k1, c.k2]).double() * r.M)
        assert 2 * ps.abs().sum(0).max() + 4 < LIM_FP32  # the doubled dgamma / dbeta


@pytest.mark.parametrize("shape,kind", CASES, ids=case_id)
def test_backward_reference_against_autograd_weight_gradient(shape, kind):
    """a D + b W G + cc G[93] is the weight gradient of dy = a dz + b y + cc: the ones-column
    algebra of the reference, proven against torch's conv2d_weight in float64."""
    r, c, f = es.bwd_refs(shape, kind), es.coef_case(), es.fwd_refs(shape, kind, "small")
    dy = c.a * r.dz + c.b * f.y + c.cc
    want = torch.nn.grad.conv2d_weight(f.x.permute(0, 3, 1, 2), (64, 3, 7, 7), dy.permute(0, 3, 1, 2),
                                       stride=2, padding=3)
    assert (r.d - want).abs().max() <= 1e-9 * want.abs().max()
    # dz against the definition: every unmasked window's gradient lands on the pixel it names
    B, PH, PW, C = r.g.shape
    dz = torch.zeros_like(r.dz)
    sel = (r.code4 != 15).nonzero()
    n, i, j, ch = sel.unbind(1)
    cd = r.code4[n, i, j, ch]
    dz.index_put_((n, 2 * i - 1 + (2 - (cd >> 2)), 2 * j - 1 + (2 - (cd & 3)), ch), r.g.double()[n, i, j, ch],
                  accumulate=True)
    assert torch.equal(dz, r.dz)


# ------------------------------------------------------------------ small helpers
def test_layout_helpers():
    w = es.weights("large")
    wk = es.ref_pack_weights(w)
    assert tuple(wk.shape) == (64, es.SKP) and not wk[:, es.KDEF:].any()
    for ky in range(7):
        assert not wk[:, ky * 24 + 21:ky * 24 + 24].any()
    assert wk[5, 2 * 24 + 4 * 3 + 1] == w[5, 1, 2, 4]
    assert torch.equal(es.dw_of_k(wk), w.double())
    code = torch.randint(0, 16, (3, 64))
    assert torch.equal(es.unpack_nibbles(es.pack_nibbles(code)), code)
    assert es.pack_nibbles(torch.tensor([[1, 2] + [0] * 62]))[0, 0] == 0x21
    ub = es.upper_blocks()
    assert ub[0, 167] and ub[40, 33] and not ub[33, 0] and not ub[0, 168] and ub[es.GONE, 100]


@pytest.mark.parametrize("shape", es.APPLY_SHAPES, ids=case_id)
def test_pool_apply_case(shape):
    c = es.apply_case(shape)
    assert torch.equal(c.pext, c.pext.to(torch.bfloat16).float()), "pext exact in bf16"
    assert c.z.abs().max() < LIM_FP32 and _is_int(c.z)
    assert (c.z == 0).float().mean() > 0.02 and (c.code4[c.z == 0] == 15).all()
    assert (c.code4[c.z > 0] == c.code[c.z > 0]).all()
    assert (c.out != c.z.clamp_min(0)).any(), "the bf16 rounding of the output must matter"
    assert (c.scale == 0).any() and (c.scale < 0).any()
    chunks = c.pext.numel() // 8
    assert (chunks < 1024) == (shape == es.APPLY_SHAPES[0]) and chunks % 1024 != 0
