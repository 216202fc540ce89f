"""Element-exact tests of the fused ResNet stem (csrc/stem_fused.hip).

Raw images that normalise to small integers, integer weights and dyadic BN coefficients make
every intermediate exactly representable (tests/test_exact_stem_cpu.py asserts the preconditions
of each case here), so the pooled extremum, every window code, the statistics, the D = dz^T X
and G = X^T X slabs and the final weight gradient must equal the float64 references of
tests/exact_stem.py bit for bit, whatever the grid, the input type or the batch's row index.
Outputs are NaN-prefilled views between guard regions (a missed element or a write past the
tensor shows); inputs sit between 0xFF guards.  No tolerance appears in this file.

Not asserted, because undefined: columns >= 168 of the D and G slabs and G's lower-triangle
32-blocks (the kernels compute finite values there, or leave them unwritten, and never use
them), and the statistics under the large weights (sums of squares past 2^24 depend on the
accumulation order)."""
import pytest
import torch

import exact_conv as ec
import exact_stem as es
from dmlab.ops._native import lib

pytestmark = pytest.mark.gpu

BF, F32, F64, U8, I64 = torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.long
sid = lambda v: (es.shape_id(v) if len(v) == 5 else "x".join(map(str, v))) if isinstance(v, tuple) else str(v)


class Bench:
    """Guarded device tensors of one test; done() checks every guard."""

    def __init__(self, dev):
        self.dev, self.outs, self.inputs = dev, [], []

    def inp(self, t, dtype=None, what="operand"):
        dtype = dtype or t.dtype
        v, chk = ec.guarded(tuple(t.shape), dtype, self.dev, "in")
        v.copy_(t.to(self.dev))
        self.inputs.append((chk, what))
        return v

    def out(self, shape, dtype, what="output"):
        v, chk = ec.guarded(tuple(shape), dtype, self.dev, "out")
        self.outs.append((chk, what))
        return v

    def done(self):
        for chk, what in self.outs + self.inputs:
            chk(what)
        self.outs = []


def _exact(got, want, what):
    """Bit-equal on the device; the element-wise report of assert_exact on a mismatch."""
    want = want.to(got.device)
    if got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want):
        return
    ec.assert_exact(got.reshape(want.shape), want, what, layout="")


def _exact_bf16(got, want, what):
    """got (bf16) against a float64 reference: the same bits, the sign of a zero included."""
    w = want.to(BF)
    assert torch.equal(w.double(), want), f"{what}: the reference is not a bf16 number"
    w = w.to(got.device)
    if torch.equal(got.view(torch.int16), w.view(torch.int16)):
        return
    ec.assert_exact(got, want, what, layout="")
    raise AssertionError(f"{what}: equal values, different bits (the sign of a zero)")


def _exact_codes(got, want, what):
    """got [..., 32] nibble-packed bytes against reference nibbles [..., 64]."""
    if torch.equal(got, es.pack_nibbles(want).to(got.device)):
        return
    ec.assert_exact(es.unpack_nibbles(got.cpu()), want, what, layout="")


def _image(b, shape, dt):
    """The raw image on the device; bf16 and the affine fp32 as (N, 3, H, W) channels_last views."""
    raw, nsc, nbi = es.raw_image(shape, dt)
    img = b.inp(raw, what=f"image {dt}")
    return (img.permute(0, 3, 1, 2) if dt in ("bf16", "f32_affine") else img), nsc, nbi


def _idx(b, shape, kind):
    idx = es.idx_vector(shape, kind)
    return None if idx is None else b.inp(idx, I64, "idx")


def _wk(b, wkind):
    return b.inp(es.ref_pack_weights(es.weights(wkind)), BF, "wk")


# ------------------------------------------------------------------ stem_pack_weights
@pytest.mark.parametrize("wkind", es.WKINDS)
def test_stem_pack_weights_exact(dev, wkind):
    """wk[64][176]: the taps at ky*24 + kx*3 + c, zeros at kx*3 + c >= 21 and k >= 168."""
    b = Bench(dev)
    w = b.inp(es.weights(wkind), F32, "w")
    wk = b.out((64, es.SKP), BF, "wk")
    lib().stem_pack_weights(w, wk)
    _exact_bf16(wk, es.ref_pack_weights(es.weights(wkind)), "wk")
    b.done()


# ------------------------------------------------------------------ forward
def _forward_runs(dev, shape, wkind, dtypes=es.DTYPES, kinds=es.IDX_KINDS, grids=None):
    """Every forward launch of one case: input types x index vectors x grids x train; yields
    (label, reference, grid, pext, code, stats or None) after the guards were checked."""
    B, Nimg, H, W, _ = shape
    b = Bench(dev)
    wk, gamma = _wk(b, wkind), b.inp(es.gamma_fwd(), F32, "gamma")
    for dt in dtypes:
        img, nsc, nbi = _image(b, shape, dt)
        for kind in kinds:
            r, idx = es.fwd_refs(shape, kind, wkind), _idx(b, shape, kind)
            for grid in grids or es.grids_of(shape):
                for train in (True, False):
                    pext = b.out((B, H // 4, W // 4, 64), BF, "pext")
                    code = b.out((B, H // 4, W // 4, 32), U8, "code")
                    stats = b.out((grid * 128,), F32, "stats") if train else None
                    lib().stem_fwd_fused(img, idx, nsc, nbi, wk, gamma, pext, code, stats, grid)
                    b.done()
                    yield f"{dt}, idx {kind}, grid {grid}, train={train}", r, grid, pext, code, stats


@pytest.mark.parametrize("wkind", es.WKINDS)
@pytest.mark.parametrize("shape", es.SHAPES, ids=sid)
def test_stem_forward_pext_exact(dev, shape, wkind):
    """The pooled extremum of bf16(y), max where gamma >= 0 (both zeros) and min where gamma < 0:
    the same bits as the reference for small and large weights (|y| up to 882: the kernel's bf16
    rounding of y is torch's), for u8 / bf16 / fp32 / per-channel-affine fp32 images, identity,
    repeated and clamped row indices, grid 1, the case's and B, with and without statistics."""
    for label, r, grid, pext, code, stats in _forward_runs(dev, shape, wkind):
        _exact_bf16(pext, r.pext, f"pext ({label})")


@pytest.mark.parametrize("wkind", es.WKINDS)
@pytest.mark.parametrize("shape", es.SHAPES, ids=sid)
def test_stem_forward_codes_exact(dev, shape, wkind):
    """Every window-code nibble (2 - kh) << 2 | (2 - kw) names the first extremum in (kh, kw)
    scan order over the in-image positions; at least 5 % of the windows tie on the small weights
    (asserted on the CPU), so the kernel's integer tie-break is what is compared.  No agreement
    threshold."""
    for label, r, grid, pext, code, stats in _forward_runs(dev, shape, wkind):
        _exact_codes(code, r.code, f"codes ({label})")


@pytest.mark.parametrize("shape", es.SHAPES, ids=sid)
def test_stem_forward_stats_exact(dev, shape):
    """The per-workgroup statistics rows summed in float64 are sum y and sum y^2 (of the fp32
    accumulators, before the bf16 rounding) exactly, on the small weights.  With the large
    weights sum y^2 passes 2^24 and depends on the order: not asserted."""
    for label, r, grid, pext, code, stats in _forward_runs(dev, shape, "small"):
        if stats is not None:
            _exact(stats.view(grid, 2, 64).double().sum(0), r.stats, f"statistics ({label})")


# ------------------------------------------------------------------ stem_pool_apply
@pytest.mark.parametrize("shape", es.APPLY_SHAPES, ids=sid)
def test_stem_pool_apply_exact(dev, shape):
    """out = bf16(relu(scale * pext + shift)) and every code4 nibble (15 where z <= 0, z == 0
    included) with integer scale / shift (zero and negative scales); below one 1024-chunk block
    and across a partial second one.  Without codes: the same out, nothing else written."""
    c, b = es.apply_case(shape), Bench(dev)
    pext = b.inp(c.pext, BF, "pext")
    code = b.inp(es.pack_nibbles(c.code), U8, "code")
    scale, shift = b.inp(c.scale, F32, "scale"), b.inp(c.shift, F32, "shift")
    out, code4 = b.out(shape, BF, "out"), b.out(shape[:3] + (32,), U8, "code4")
    lib().stem_pool_apply(pext, code, scale, shift, out, code4)
    _exact_bf16(out, c.out, "out")
    _exact_codes(code4, c.code4, "code4")
    b.done()
    out2 = b.out(shape, BF, "out, no codes")
    lib().stem_pool_apply(pext, None, scale, shift, out2)
    _exact_bf16(out2, c.out, "out, no codes")
    b.done()


# ------------------------------------------------------------------ backward
class Backward:
    """The operands of one backward case on the device and the call itself."""

    def __init__(self, dev, shape, b=None):
        self.shape, self.dev, self.b = shape, dev, b or Bench(dev)
        b, c = self.b, es.coef_case()
        self.c = c
        self.M = shape[0] * (shape[2] // 2) * (shape[3] // 2)
        self.wk = _wk(b, "small")
        self.mean, self.invstd = b.inp(c.mean, F32, "mean"), b.inp(c.invstd, F32, "invstd")
        self.gamma = b.inp(c.gamma, F32, "gamma")
        self.sums = b.inp(torch.cat([c.k1, c.k2]).double() * es.TOTAL2, F64, "sums")
        self.total = b.inp(torch.tensor([es.TOTAL2], dtype=F64), F64, "total")
        self.pre = b.inp(es.pre_slab(self.M).reshape(-1), F32, "pre_slab")
        self.imgs, self.grads = {}, {}

    def image(self, dt):
        if dt not in self.imgs:
            self.imgs[dt] = _image(self.b, self.shape, dt)
        return self.imgs[dt]

    def pooled(self, kind):
        """(idx, pdy, code4) of one index vector: the reference's pooled gradient and codes."""
        if kind not in self.grads:
            r = es.bwd_refs(self.shape, kind)
            self.grads[kind] = (_idx(self.b, self.shape, kind), self.b.inp(r.g, BF, "pdy"),
                                self.b.inp(es.pack_nibbles(r.code4), U8, "code4"))
        return self.grads[kind]

    def call(self, dt, kind, grid, wbeta, gbeta, local, dw=None, dgamma=None, dbeta=None, calls=1):
        """One stem_bwd_fused2 (or `calls` of them into the same gradients) on fresh guarded
        outputs; local: coefficients from pre_slab, else from the crafted global sums."""
        b, c, L = self.b, self.c, lib()
        r = es.bwd_refs(self.shape, kind)
        img, nsc, nbi = self.image(dt)
        idx, pdy, code4 = self.pooled(kind)
        o = SimpleOut()
        o.r = r
        o.dw = b.inp(c.dw0, F32, "dw") if wbeta else b.out((64, 3, 7, 7), F32, "dw")
        o.dgamma = b.inp(c.dgamma0, F32, "dgamma") if (gbeta or not local) else b.out((64,), F32, "dgamma")
        o.dbeta = b.inp(c.dbeta0, F32, "dbeta") if (gbeta or not local) else b.out((64,), F32, "dbeta")
        o.work = b.out((L.bn_bwd_work(self.M, 64),), F32, "work")
        o.dslab = b.out((L.stem_bwd_slab_len(grid),), F32, "dslab")
        extra = {} if local else dict(sums=self.sums, total=self.total)
        for _ in range(calls):
            L.stem_bwd_fused2(img, idx, nsc, nbi, self.wk, pdy, code4, self.mean, self.invstd, self.gamma,
                              o.dgamma, o.dbeta, gbeta, self.pre, es.PRE_ROWS, o.dw, wbeta, o.work,
                              o.dslab, grid, **extra)
        nd, ng = 64 * es.SKH, es.GK * es.GK
        o.dpart = o.dslab[:grid * nd].view(grid, 64, es.SKH)
        o.gpart = o.dslab[grid * nd:grid * (nd + ng)].view(grid, es.GK, es.GK)
        o.dsum = o.dslab[grid * (nd + ng):grid * (nd + ng) + nd].view(64, es.SKH)
        o.gsum = o.dslab[grid * (nd + ng) + nd:].view(es.GK, es.GK)
        b.done()
        return o


class SimpleOut:
    pass


def _variants(shape):
    """Input types x index vectors x grids of a backward case."""
    return [(dt, kind, grid) for dt in es.DTYPES for kind in es.IDX_KINDS for grid in es.grids_of(shape)]


def _check_slabs(o, label):
    """All four slab comparisons; every mismatch is reported, not only the first."""
    r = o.r
    ub = es.upper_blocks().to(o.gsum.device)
    G = torch.zeros(es.GK, es.GK, dtype=F64)
    G[:es.KDEF, :es.KDEF] = r.G
    G = torch.where(ub, G.to(o.gsum.device), 0.0)
    defined = lambda g: torch.where(ub, g.double(), 0.0)  # NaN where a block was never written
    bad = []
    for got, want, what in ((o.dsum[:, :es.KDEF], r.D, "dsum = dz^T X"),
                            (defined(o.gsum), G, "gsum = X^T X (row 93 = colsum X)"),
                            (o.dpart.double().sum(0)[:, :es.KDEF], r.D, "the D partials' sum"),
                            (defined(o.gpart.double().sum(0)), G, "the G partials' sum")):
        try:
            _exact(got, want, f"{what} ({label})")
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", es.SHAPES, ids=sid)
def test_stem_backward_slabs_exact(dev, shape):
    """dsum[:, :168] = dz^T X and gsum = X^T X on the upper-triangle 32-blocks below 168 (row and
    column 93 = colsum(X) and the ky*24 + 21 ones columns included), and the per-workgroup
    partials summed in float64, element by element.  Columns >= 168 and the lower-triangle blocks
    are undefined and ignored."""
    bw = Backward(dev, shape)
    for dt, kind, grid in _variants(shape):
        o = bw.call(dt, kind, grid, 0.0, 0.0, local=False)
        _check_slabs(o, f"{dt}, idx {kind}, grid {grid}")


@pytest.mark.parametrize("shape", es.SHAPES, ids=sid)
def test_stem_backward_dw_global_sums_exact(dev, shape):
    """Coefficients from crafted global sums k * total (dyadic gamma, invstd, mean): work[0:192)
    and dW = wbeta dW0 + a D + b W G + cc G[93] exact for wbeta 0 and 1, the same for every grid,
    input type and row index; dgamma / dbeta untouched; two accumulating calls add twice."""
    bw, c = Backward(dev, shape), es.coef_case()
    coef = torch.cat([c.a, c.b, c.cc])
    for dt, kind, grid in _variants(shape):
        for wbeta in (0.0, 1.0):
            o = bw.call(dt, kind, grid, wbeta, 0.0, local=False)
            label = f"{dt}, idx {kind}, grid {grid}, wbeta {wbeta}"
            _exact(o.dw, es.want_dw(o.r, wbeta), f"dW ({label})")
            _exact(o.work[:192], coef, f"coefficients ({label})")
            _exact(o.dgamma, c.dgamma0, f"dgamma untouched ({label})")
            _exact(o.dbeta, c.dbeta0, f"dbeta untouched ({label})")
    o = bw.call("u8", "perm", shape[4], 1.0, 0.0, local=False, calls=2)
    _exact(o.dw, es.want_dw(o.r, 1.0, calls=2), "dW, two accumulating calls")


@pytest.mark.parametrize("shape", es.POW2_SHAPES, ids=sid)
def test_stem_backward_dw_local_coefficients_exact(dev, shape):
    """Coefficients from a crafted integer pre_slab whose rows sum to (k1 M, k2 M), M a power of
    two: work[0:192) = (a, b, cc), dgamma = gbeta dgamma0 + k2 M, dbeta = gbeta dbeta0 + k1 M and
    dW exact for gbeta = wbeta in {0, 1}; two accumulating calls add twice."""
    bw, c = Backward(dev, shape), es.coef_case()
    coef = torch.cat([c.a, c.b, c.cc])
    M = bw.M
    for dt, kind, grid in _variants(shape):
        for beta in (0.0, 1.0):
            o = bw.call(dt, kind, grid, beta, beta, local=True)
            label = f"{dt}, idx {kind}, grid {grid}, beta {beta}"
            _exact(o.work[:192], coef, f"coefficients ({label})")
            _exact(o.dw, es.want_dw(o.r, beta), f"dW ({label})")
            _exact(o.dgamma, beta * c.dgamma0.double() + c.k2.double() * M, f"dgamma ({label})")
            _exact(o.dbeta, beta * c.dbeta0.double() + c.k1.double() * M, f"dbeta ({label})")
    o = bw.call("f32", "clamp", shape[4], 1.0, 1.0, local=True, calls=2)
    _exact(o.dw, es.want_dw(o.r, 1.0, calls=2), "dW, two accumulating calls")
    _exact(o.dgamma, c.dgamma0.double() + 2 * c.k2.double() * M, "dgamma, two accumulating calls")
    _exact(o.dbeta, c.dbeta0.double() + 2 * c.k1.double() * M, "dbeta, two accumulating calls")


# ------------------------------------------------------------------ the workload's geometry
def test_stem_workload_geometry_once(dev):
    """224 x 224 at B = 2, u8 images, identity index, one launch each way: pext, codes,
    statistics, the slabs and dW."""
    shape = es.WORKLOAD_SHAPE
    runs = _forward_runs(dev, shape, "small", dtypes=("u8",), kinds=("id",), grids=(shape[4],))
    label, r, grid, pext, code, stats = next(runs)  # train=True
    _exact_bf16(pext, r.pext, "pext")
    _exact_codes(code, r.code, "codes")
    _exact(stats.view(grid, 2, 64).double().sum(0), r.stats, "statistics")
    o = Backward(dev, shape).call("u8", "id", grid, 0.0, 0.0, local=False)
    _check_slabs(o, "224 x 224")
    _exact(o.dw, es.want_dw(o.r, 0.0), "dW")


# ------------------------------------------------------------------ refusals
def test_stem_refusals(dev):
    """Every argument the bindings must refuse raises before any launch (the other arguments are
    valid and sized for the call, so even an unguarded kernel would stay inside them)."""
    L, c = lib(), es.coef_case()
    f = dict(device=dev, dtype=F32)
    wk = es.ref_pack_weights(es.weights("small")).to(dev, BF)
    gamma = es.gamma_fwd().to(dev)
    one, zero = [1.0] * 3, [0.0] * 3

    def fwd(H=32, W=32, B=2, Nimg=2, grid=1, idx=None, wk=wk, pext=None, stats=True):
        img = torch.zeros(Nimg, H, W, 3, **f)
        pext = torch.empty(B, H // 4, W // 4, 64, device=dev, dtype=BF) if pext is None else pext
        code = torch.empty(pext.numel() // 2, device=dev, dtype=U8)
        st = torch.empty(max(grid, 1) * 128, **f) if stats else None
        L.stem_fwd_fused(img, idx, one, zero, wk, gamma, pext, code, st, grid)

    def bwd(H=32, W=32, B=2, Nimg=2, grid=1, idx=None, wk=wk, pdy=None, short=0, sums=None, total=None):
        img = torch.zeros(Nimg, H, W, 3, **f)
        pdy = torch.zeros(B, H // 4, W // 4, 64, device=dev, dtype=BF) if pdy is None else pdy
        code4 = torch.full((pdy.numel() // 2,), 0xFF, device=dev, dtype=U8)
        M = B * (H // 2) * (W // 2)
        v = [x.to(dev) for x in (c.mean, c.invstd, c.gamma, c.dgamma0, c.dbeta0)]
        L.stem_bwd_fused2(img, idx, one, zero, wk, pdy, code4, v[0], v[1], v[2], v[3], v[4], 0.0,
                          torch.zeros(es.PRE_ROWS * 128, **f), es.PRE_ROWS, torch.zeros(64, 3, 7, 7, **f),
                          0.0, torch.empty(L.bn_bwd_work(M, 64), **f),
                          torch.empty(L.stem_bwd_slab_len(max(grid, 1)) - short, **f), grid,
                          sums=sums, total=total)

    fwd(), bwd()  # the valid calls the refusals below vary
    torch.cuda.synchronize()
    idx32 = torch.zeros(2, device=dev, dtype=torch.int32)
    idx3 = torch.zeros(3, device=dev, dtype=I64)
    for call in (fwd, bwd):
        for H, W in es.REFUSED_SIZES:
            assert not L.stem_fused_supported(H, W) and not es.stem_supported(H, W)
            with pytest.raises(RuntimeError):
                call(H=H, W=W)
        for kw in (dict(grid=0), dict(grid=3), dict(wk=wk.flatten()[:-1]), dict(wk=torch.cat([wk.flatten(), wk[0]])),
                   dict(idx=idx32), dict(idx=idx3), dict(B=3, Nimg=2)):
            with pytest.raises(RuntimeError):
                call(**kw)
    for s in es.ALL_SHAPES:
        assert L.stem_fused_supported(s[2], s[3])
    bad = torch.zeros(2, 8, 4, 64, device=dev, dtype=BF)  # [B, H/4, W/4, 64] would be 2, 8, 8, 64
    with pytest.raises(RuntimeError):
        fwd(pext=bad)
    with pytest.raises(RuntimeError):
        bwd(pdy=bad)
    with pytest.raises(RuntimeError):
        bwd(short=1)
    with pytest.raises(RuntimeError):
        bwd(sums=torch.zeros(128, device=dev, dtype=F64))
    with pytest.raises(RuntimeError):
        bwd(total=torch.ones(1, device=dev, dtype=F64))
    p = torch.zeros(1, 2, 2, 64, device=dev, dtype=BF)
    sc = torch.ones(64, **f)
    with pytest.raises(RuntimeError):  # code without code4
        L.stem_pool_apply(p, torch.zeros(128, device=dev, dtype=U8), sc, sc, torch.empty_like(p))
    torch.cuda.synchronize()
