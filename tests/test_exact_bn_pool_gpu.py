"""Element-exact tests of the BatchNorm and pooling kernels (csrc/bn_pool.hip).

Tier A: small-integer operands and dyadic coefficients make every intermediate exactly
representable (tests/test_exact_bn_pool_cpu.py asserts the preconditions of each case here), so
every result must equal the float64 reference of tests/exact_bn_pool.py bit for bit, element
by element, whatever the accumulation order or FMA contraction.  Tier B: the whole backward at
an M that is no power of two, exact sums and an element-wise bound on dy.  Outputs are
NaN-prefilled views between guard regions (a missed element or a write past the tensor shows);
inputs sit between NaN guards.  The bindings' guards are checked with arguments that even an
unguarded kernel would have kept inside its allocations."""
import pytest
import torch

import exact_bn_pool as eb
import exact_conv as ec
from dmlab.ops._native import lib

pytestmark = pytest.mark.gpu

BF, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
ids = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


class Bench:
    """Guarded device tensors of one test; done() checks every guard."""

    def __init__(self, dev):
        self.dev, self.checks, self.inputs = dev, [], []

    def inp(self, t, dtype, shape=None, what="operand"):
        shape = tuple(t.shape) if shape is None else shape
        v, chk = ec.guarded(shape, dtype, self.dev, "in")
        v.copy_(t.reshape(shape).to(self.dev))
        self.inputs.append((chk, what))
        return v

    def out(self, shape, dtype, what="output"):
        v, chk = ec.guarded(tuple(shape), dtype, self.dev, "out")
        self.checks.append((chk, what))
        return v

    def done(self):
        for chk, what in self.checks + self.inputs:
            chk(what)
        self.checks = []


def _exact(got, want, what):
    ec.assert_exact(got.reshape(want.shape), want, what, layout="")


def _work(M, C, dev):
    return torch.empty(lib().bn_bwd_work(M, C), device=dev, dtype=F32)


# ------------------------------------------------------------------ bn_apply
@pytest.mark.parametrize("shape", eb.APPLY_SHAPES, ids=ids)
def test_bn_apply_exact(dev, shape):
    """All four RES / RELU variants, with and without the 1-bit mask: out and the mask bytes
    (out > 0 of the reference) at every element; partial and full 1024-chunk blocks."""
    M, C = shape
    c, b = eb.bn_case(M, C), Bench(dev)
    y = b.inp(c.y, BF, (1, 1, M, C), "y")
    res = b.inp(c.res, BF, (1, 1, M, C), "res")
    scale, shift = b.inp(c.scale, F32), b.inp(c.shift, F32)
    for use_res in (False, True):
        for relu in (False, True):
            want = eb.ref_apply(c.y, c.scale, c.shift, res=c.res if use_res else None, relu=relu)
            for with_mask in ((False, True) if relu else (False,)):
                out = b.out((1, 1, M, C), BF, "out")
                mask = b.out((M * C // 8,), U8, "mask") if with_mask else None
                lib().bn_apply(y, res if use_res else None, scale, shift, out, relu, mask=mask)
                _exact(out, want, f"bn_apply res={use_res} relu={relu} mask={with_mask}")
                if with_mask:
                    assert torch.equal(mask.cpu(), eb.pack_bits(want > 0)), "mask bytes"
                b.done()


# ------------------------------------------------------------------ max pool
@pytest.mark.parametrize("geom", eb.MAXPOOL_GEOMS, ids=ids)
def test_maxpool_exact(dev, geom):
    """Values and codes of the forward (first maximum wins); the backward as its definition,
    from the forward's codes and from a random code tensor (a pixel can win four windows)."""
    N, H, W, C, K, S, P = geom
    OH, OW = eb.pool_out(H, W, K, S, P)
    c, b = eb.pool_case(geom), Bench(dev)
    x = b.inp(c.x, BF, what="x")
    y, idx = b.out((N, OH, OW, C), BF, "y"), b.out((N, OH, OW, C), U8, "idx")
    lib().maxpool_fwd(x, y, idx, K, S, P)
    best, code = eb.ref_maxpool_fwd(c.x, K, S, P)
    _exact(y, best, "maxpool_fwd y")
    _exact(idx, code, "maxpool_fwd codes")
    dy = b.inp(c.dy, BF, what="dy")
    for name, cd in (("forward codes", code), ("random codes", c.codes)):
        dx = b.out((N, H, W, C), BF, "dx")
        lib().maxpool_bwd(dy, b.inp(cd.to(U8), U8, what="idx"), dx, K, S, P)
        _exact(dx, eb.ref_pool_gather(c.dy, cd, H, W, K, S, P), f"maxpool_bwd, {name}")
    b.done()


@pytest.mark.parametrize("geom", eb.FUSED_GEOMS, ids=ids)
def test_bn_relu_maxpool_exact(dev, geom):
    """The fused stem tail (3x3/s2/p1 pair kernel; the generic kernel through 2/2/0 and 3/1/1):
    pooled values, codes (15 where the window maximum is 0) and yarg at every element."""
    N, H, W, C, K, S, P = geom
    OH, OW = eb.pool_out(H, W, K, S, P)
    c, b = eb.pool_case(geom), Bench(dev)
    y = b.inp(c.y, BF, what="y")
    scale, shift = b.inp(c.scale, F32), b.inp(c.shift, F32)
    want, code, arg = eb.ref_fused_pool(c.y, c.scale, c.shift, K, S, P)
    for with_yarg in (True, False):
        out, idx = b.out((N, OH, OW, C), BF, "out"), b.out((N, OH, OW, C), U8, "idx")
        yarg = b.out((N, OH, OW, C), BF, "yarg") if with_yarg else None
        lib().bn_relu_maxpool(y, scale, shift, out, idx, K, S, P, yarg=yarg)
        _exact(out, want, "bn_relu_maxpool out")
        _exact(idx, code, "bn_relu_maxpool codes")
        if with_yarg:
            _exact(yarg, arg, "bn_relu_maxpool yarg")
        b.done()


# ------------------------------------------------------------------ average pool
@pytest.mark.parametrize("C", eb.AVG_C)
@pytest.mark.parametrize("HW", eb.AVG_HW)
def test_avgpool_exact(dev, HW, C):
    """Forward: the exact sum, one fp32 division, RNE to bf16.  Backward: g * fp32(1 / HW), RNE."""
    c, b = eb.avg_case(HW, C), Bench(dev)
    x = b.inp(c.x, BF, (3, 1, HW, C), "x")
    y = b.out((3, C), BF, "y")
    lib().avgpool_fwd(x, y)
    _exact(y, eb.ref_avg_fwd(c.x), "avgpool_fwd")
    dx = b.out((3, HW, 1, C), BF, "dx")
    lib().avgpool_bwd(b.inp(c.g, BF, what="g"), dx)
    _exact(dx, eb.ref_avg_bwd(c.g, HW), "avgpool_bwd")
    b.done()


# ------------------------------------------------------------------ forward finalize
def _check_finalize(got, fin, nb, nb_want):
    scale, shift, mean, invstd, rm, rv = got
    eb.assert_ulps(mean, fin.mean, 1, "mean")
    eb.assert_ulps(invstd, fin.invstd, 1, "invstd")
    eb.assert_ulps(scale, fin.scale, 1, "scale")
    eb.assert_ulps(shift, fin.shift, 4, "shift", of=fin.shift_terms)
    eb.assert_ulps(rm, fin.rmean, 4, "running_mean", of=fin.rmean_terms)
    eb.assert_ulps(rv, fin.rvar, 4, "running_var", of=fin.rvar_terms)
    assert int(nb.item()) == nb_want


@pytest.mark.parametrize("C", eb.STAT_C)
@pytest.mark.parametrize("T", eb.STAT_T)
def test_stats_finalize_and_sync_local(dev, T, C):
    """Integer slabs: the column sums are exact, so every result is one or a few roundings of a
    float64 expression.  T = 257 takes the 4-channel finalize, 2049 the slab_colsum pre-pass,
    8200 its 256-group cap with trailing empty groups.  T = 1 also runs count = 1 (no division
    by count - 1)."""
    c, b = eb.stat_case(T, C), Bench(dev)
    eb.stat_preconditions(c)
    slab = b.inp(c.slab, F32, (T * 2 * C,), "slab")
    gamma, beta = b.inp(c.gamma, F32), b.inp(c.beta, F32)
    S, Q = c.slab[:, 0].double().sum(0), c.slab[:, 1].double().sum(0)
    work = torch.empty(512 * C, device=dev, dtype=F32)
    for count in ([c.count, 1.0] if T == 1 else [c.count]):
        rm, rv = b.inp(c.rmean, F32), b.inp(c.rvar, F32)
        outs = [b.out((C,), F32, n) for n in ("scale", "shift", "mean", "invstd")]
        nb = torch.full((1,), 41, dtype=torch.int64, device=dev)
        lib().bn_stats_finalize(slab, T, count, gamma, beta, rm, rv, eb.MOMENTUM, eb.EPS, *outs, work, nb)
        _check_finalize(outs + [rm, rv], eb.ref_finalize(S, Q, count, c.gamma, c.beta, c.rmean, c.rvar), nb, 42)
        row = b.out((2 * C + 1,), F64, "row")
        lib().bn_sync_local(slab, T, count, C, row, work)
        want = eb.ref_sync_row(S, Q, count)
        got = row.cpu()
        assert ((got - want).abs() <= 2.0 ** -50 * want.abs()).all(), "bn_sync_local row"
        b.done()


@pytest.mark.parametrize("C", [8, 24, 512])
@pytest.mark.parametrize("ws", [1, 2, 3])
def test_sync_finalize(dev, ws, C):
    """The rank-order merge of ws rows of unequal counts against the float64 merge of the same
    rows.  (A rank with n = 0 cannot occur: bn_sync_local refuses count < 1 and the Python layer
    always passes its own N*OH*OW >= 1, so no all-zero row is tested.)"""
    b = Bench(dev)
    Ts, counts = [7, 257, 2049][:ws], [60.0, 2056.0 + 5, 2 * 16392.0][:ws]
    rows = b.out((ws, 2 * C + 1), F64, "rows")
    work = torch.empty(512 * C, device=dev, dtype=F32)
    for r in range(ws):
        sc = eb.stat_case(Ts[r], C, seed=r)
        lib().bn_sync_local(sc.slab.view(-1).to(dev), Ts[r], counts[r], C, rows[r], work)
    c = eb.stat_case(Ts[0], C)
    mean, var, N = eb.ref_sync_merge(rows.cpu())
    assert N == sum(counts)
    rm, rv = b.inp(c.rmean, F32), b.inp(c.rvar, F32)
    outs = [b.out((C,), F32, n) for n in ("scale", "shift", "mean", "invstd")]
    nb = torch.zeros(1, dtype=torch.int64, device=dev)
    total = b.out((1,), F64, "total")
    lib().bn_sync_finalize(rows, b.inp(c.gamma, F32), b.inp(c.beta, F32), rm, rv, eb.MOMENTUM, eb.EPS,
                           *outs, nb, total)
    assert total.item() == N
    _check_finalize(outs + [rm, rv], eb.ref_finalize_mv(mean, var, N, c.gamma, c.beta, c.rmean, c.rvar), nb, 1)
    b.done()


@pytest.mark.parametrize("C", eb.EVAL_C)
def test_bn_eval_coeffs(dev, C):
    """scale within 8 fp32 ulps of float64 (rsqrtf is not correctly rounded), shift within 8
    ulps of its largest term."""
    g = torch.Generator().manual_seed(C)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rmean, rvar = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    b = Bench(dev)
    scale, shift = b.out((C,), F32, "scale"), b.out((C,), F32, "shift")
    lib().bn_eval_coeffs(b.inp(gamma, F32), b.inp(beta, F32), b.inp(rmean, F32), b.inp(rvar, F32), eb.EPS,
                         scale, shift)
    want = gamma.double() / torch.sqrt(rvar.double() + eb.f32(eb.EPS))
    eb.assert_ulps(scale, want, 8, "scale")
    eb.assert_ulps(shift, beta.double() - rmean.double() * want, 8, "shift",
                   of=torch.maximum(beta.double().abs(), (rmean.double() * want).abs()))
    b.done()


# ------------------------------------------------------------------ backward, stage 1
class BwdOps:
    """Device operands of one backward case (c on the CPU or already on the device)."""

    def __init__(self, b, c, shape4):
        self.b, self.c = b, c
        self.y = b.inp(c.y, BF, shape4, "y")
        self.dout = b.inp(c.dout, BF, shape4, "dout")
        self.scale, self.shift = b.inp(c.scale, F32), b.inp(c.shift, F32)
        self.mean = b.inp(c.mean, F32)
        out = eb.ref_apply(c.y, c.scale, c.shift, res=c.res)
        self.out = b.inp(out, BF, shape4, "out")
        self.mask = b.inp(eb.pack_bits(out > 0), U8, what="mask")
        self.pdy = self.pidx = None
        self.ksp = (3, 2, 1)

    def call(self, mode, invstd, gamma, dg, db, gbeta, dy, dres, work, **kw):
        lib().bn_backward(None if mode == 3 else self.dout, self.out if mode == 1 else None, self.y,
                          self.mean, invstd, gamma, dg, db, gbeta, mode, self.scale, self.shift,
                          self.pdy, self.pidx, *self.ksp, dy, dres, work,
                          mask=self.mask if mode == 4 else None, **kw)


def _stage1(dev, c, shape4, modes, b=None, ops=None):
    M, C = c.M, c.C
    b = b or Bench(dev)
    ops = ops or BwdOps(b, c, shape4)
    invstd = b.inp(c.invstd, F32)
    gamma = torch.ones(C, device=dev)
    work = _work(M, C, dev)
    dy = torch.full(shape4, float("nan"), device=dev, dtype=BF)
    for mode in modes:
        want = eb.ref_bwd_sums(eb.ref_dz(c, mode), c.y, c.mean, c.invstd)
        for gbeta in (0.0, 1.0, 0.5):
            dg, db = b.inp(c.dg0, F32, what="dgamma"), b.inp(c.db0, F32, what="dbeta")
            sums = b.out((2 * C,), F64, "sums")
            ops.call(mode, invstd, gamma, dg, db, gbeta, dy, None, work, stage=1, sums=sums)
            _exact(sums, want, f"sums, mode {mode}")
            wdg, wdb = eb.ref_grads(want, c, gbeta)
            _exact(dg, wdg, f"dgamma, mode {mode}, gbeta {gbeta}")
            _exact(db, wdb, f"dbeta, mode {mode}, gbeta {gbeta}")
            b.done()
    assert bool(torch.isnan(dy).all()), "stage 1 applies nothing"
    return ops, b, invstd


@pytest.mark.parametrize("shape", eb.SUMS_SHAPES, ids=ids)
def test_bn_backward_sums_exact(dev, shape):
    """Stage "sums" of modes 0, 1, 2, 4: sums (float64), dgamma and dbeta for gbeta 0, 1, 0.5
    over integer prior contents; the part rows of bn_bwd_reduce_masked summed on the host."""
    M, C = shape
    c = eb.bn_case(M, C)
    ops, b, invstd = _stage1(dev, c, (1, 1, M, C), (0, 1, 2, 4))
    rows = lib().bn_bwd_rows(M, C)
    part = b.out((rows * 2 * C,), F32, "part")
    assert lib().bn_bwd_reduce_masked(ops.dout, ops.y, ops.mean, invstd, ops.scale, ops.shift, part) == rows
    want = eb.ref_bwd_sums(eb.ref_dz(c, 2), c.y, c.mean, c.invstd)
    _exact(part.view(rows, 2, C).double().sum(0), want, "bn_bwd_reduce_masked rows")
    b.done()


def test_bn_backward_sums_exact_at_the_group_cap(dev):
    """(32785, 2048): bn_bwd_groups reaches its cap of 2048.  The operands are drawn, and the
    float64 reference and its preconditions evaluated, on the device."""
    M, C = eb.SUMS_SHAPE_BIG
    assert -(-M // 16) > 2048 and lib().bn_bwd_rows(M, C) == 2048
    c = eb.bn_case.__wrapped__(M, C, str(dev))
    eb.sums_preconditions(c)
    _stage1(dev, c, (1, 1, M, C), (0, 1, 2, 4))


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("rows", eb.PRE_ROWS)
def test_bn_backward_pre_reduced_sums_exact(dev, rows, C):
    """Integer pre-reduced partial rows through bn_backward(stage 1, pre_slab) and bn_bwd_sums:
    the 16- and 4-channel finalizes and, past 2048 rows, the slab_colsum pre-pass."""
    M = 4
    c, b = eb.bn_case(M, C), Bench(dev)
    slab = eb.pre_slab_case(rows, C)
    want = slab.double().sum(0).view(2, C)
    ops = BwdOps(b, c, (1, 1, M, C))
    invstd, gamma = b.inp(c.invstd, F32), torch.ones(C, device=dev)
    pre = b.inp(slab, F32, (rows * 2 * C,), "pre_slab")
    dy = torch.empty(1, 1, M, C, device=dev, dtype=BF)
    for gbeta in (0.0, 1.0, 0.5):
        for entry in ("bn_backward", "bn_bwd_sums"):
            dg, db = b.inp(c.dg0, F32, what="dgamma"), b.inp(c.db0, F32, what="dbeta")
            sums = b.out((2 * C,), F64, "sums")
            if entry == "bn_backward":
                ops.call(2, invstd, gamma, dg, db, gbeta, dy, None, _work(M, C, dev), stage=1, sums=sums,
                         pre_slab=pre, pre_rows=rows)
            else:
                lib().bn_bwd_sums(pre, rows, C, dg, db, gbeta, torch.empty(515 * C, device=dev), sums)
            _exact(sums, want, f"{entry} sums")
            wdg, wdb = eb.ref_grads(want, c, gbeta)
            _exact(dg, wdg, f"{entry} dgamma, gbeta {gbeta}")
            _exact(db, wdb, f"{entry} dbeta, gbeta {gbeta}")
            b.done()


# ------------------------------------------------------------------ backward, stage 2
def _stage2(dev, c, shape4, modes, ops=None, b=None):
    """Crafted sums k * total: exact dyadic coefficients, so dy (and dres = dz) are exact."""
    M, C = c.M, c.C
    b = b or Bench(dev)
    ops = ops or BwdOps(b, c, shape4)
    invstd, gamma = b.inp(c.invstd2, F32), b.inp(c.gamma2, F32)
    sums = b.inp(torch.cat([c.k1, c.k2]).double() * eb.TOTAL2, F64, what="sums")
    total = b.inp(torch.tensor([eb.TOTAL2], dtype=F64), F64, what="total")
    a, kb, kc = eb.ref_coef2(c)
    work = _work(M, C, dev)
    for mode in modes:
        dz = eb.ref_dz(c, mode)
        want = a * dz + kb * c.y.double() + kc
        for with_dres in (False, True):
            dg, db = b.inp(c.dg0, F32, what="dgamma"), b.inp(c.db0, F32, what="dbeta")
            dy = b.out(shape4, BF, "dy")
            dres = b.out(shape4, BF, "dres") if with_dres else None
            ops.call(mode, invstd, gamma, dg, db, 0.0, dy, dres, work, stage=2, sums=sums, total=total)
            _exact(dy, want, f"dy, mode {mode}, dres={with_dres}")
            if with_dres:
                _exact(dres, dz, f"dres, mode {mode}")
            _exact(dg, c.dg0, "dgamma untouched")
            _exact(db, c.db0, "dbeta untouched")
            b.done()


@pytest.mark.parametrize("shape", eb.APPLY_SHAPES, ids=ids)
def test_bn_backward_apply_exact(dev, shape):
    """Stage "apply" of modes 0, 1, 2, 4, with and without dres, at the flat streaming kernels'
    block edges; dres against a reference of its own."""
    M, C = shape
    _stage2(dev, eb.bn_case(M, C), (1, 1, M, C), (0, 1, 2, 4))


# ------------------------------------------------------------------ mode 3
def _mode3_ops(b, c):
    N, H, W, K, S, P = c.geom
    ops = BwdOps(b, c, (N, H, W, c.C))
    ops.pdy = b.inp(c.pdy, BF, what="pdy")
    ops.pidx = b.inp(c.codes, U8, what="pidx")
    ops.ksp = (K, S, P)
    return ops


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("geom", eb.MODE3_GEOMS, ids=ids)
def test_bn_backward_mode3_exact(dev, geom, C):
    """Both stages through a max pool's gradient with a random code tensor over {0..K*K-1, 15}
    that is independent of y: the 2x2 quad kernels (even H, W, no dres), the per-pixel gather
    (odd sizes, or dres given), the K <= 2S fast path at 2/2/0 and the general loop at 3/1/1."""
    N, H, W, K, S, P = geom
    c = eb.mode3_case(geom, C)
    b = Bench(dev)
    ops = _mode3_ops(b, c)
    _stage1(dev, c, (N, H, W, C), (3,), b=b, ops=ops)
    _stage2(dev, c, (N, H, W, C), (3,), ops=ops, b=b)


# ------------------------------------------------------------------ tier B
def _whole_backward(dev, c, shape4, modes, ops_of=BwdOps):
    M, C = c.M, c.C
    b = Bench(dev)
    ops = ops_of(b, c, shape4) if ops_of is BwdOps else ops_of(b, c)
    invstd, gamma = b.inp(c.invstdB, F32), b.inp(c.gamma, F32)
    work = _work(M, C, dev)
    for mode in modes:
        dz = eb.ref_dz(c, mode)
        sums = eb.ref_bwd_sums(dz, c.y, c.mean, c.invstdB)
        ref, bound = eb.tierb_bound(*eb.ref_coef(sums, M, c.gamma, c.mean, c.invstdB), dz, c.y)
        for gbeta in (0.0, 1.0):
            dg, db = b.inp(c.dg0, F32, what="dgamma"), b.inp(c.db0, F32, what="dbeta")
            dy = b.out(shape4, BF, "dy")
            dres = b.out(shape4, BF, "dres") if mode in (1, 4) else None
            ops.call(mode, invstd, gamma, dg, db, gbeta, dy, dres, work)
            wdg, wdb = eb.ref_grads(sums, c, gbeta)
            _exact(dg, wdg, f"dgamma, mode {mode}, gbeta {gbeta}")
            _exact(db, wdb, f"dbeta, mode {mode}, gbeta {gbeta}")
            worst = eb.assert_within(dy, ref, bound, f"dy, mode {mode}")
            print(f"mode {mode} gbeta {gbeta}: worst |dy - ref| / bound = {worst:.4f}")
            if dres is not None:
                _exact(dres, dz, f"dres, mode {mode}")
            b.done()


@pytest.mark.parametrize("shape", eb.TIERB_SHAPES, ids=ids)
def test_bn_backward_whole_bounded(dev, shape):
    """Stage 0 with an inexact 1/M and gamma: dgamma and dbeta exactly (gbeta 0 and 1 in the
    whole backward), dy within ulp_bf16(ref)/2 + 8 * 2^-24 * (|a*dz| + |b*y| + |c|) of the
    float64 reference built from the stored fp32 gamma, mean and invstd.  y keeps
    |y| >= 3|mean| (exact_bn_pool.tierb_of says why the bound needs it)."""
    M, C = shape
    _whole_backward(dev, eb.tierb_of(eb.bn_case(M, C)), (1, 1, M, C), (0, 1, 2, 4))


@pytest.mark.parametrize("geom", eb.TIERB_MODE3, ids=ids)
def test_bn_backward_whole_bounded_mode3(dev, geom):
    N, H, W, K, S, P = geom
    _whole_backward(dev, eb.tierb_of(eb.mode3_case(geom, 64)), (N, H, W, 64), (3,), ops_of=_mode3_ops)


# ------------------------------------------------------------------ the bindings' guards
def _bf(dev, *shape):
    return torch.zeros(*shape, device=dev, dtype=BF)


@pytest.mark.parametrize("C", [24, 80])
def test_bn_apply_refuses_channel_counts_it_cannot_index(dev, C):
    """The kernel takes a chunk's channel as i & (C/8 - 1): C/8 must be a power of two."""
    y, v = _bf(dev, 1, 1, 4, C), torch.ones(C, device=dev)
    with pytest.raises(RuntimeError, match="power of two"):
        lib().bn_apply(y, None, v, v, torch.empty_like(y), True)


def test_bn_backward_refuses_a_dres_of_another_shape(dev):
    M, C = 4, 64
    y, v = _bf(dev, 1, 1, M, C), torch.ones(C, device=dev)
    with pytest.raises(RuntimeError, match="dres"):
        lib().bn_backward(y, None, y, v, v, v, v.clone(), v.clone(), 0.0, 0, None, None, None, None, 3, 2, 1,
                          torch.empty_like(y), _bf(dev, 1, 1, 2 * M, C), _work(M, C, dev))


def test_maxpool_guards(dev):
    """idx dtype and size, N and C, the pooled extent, K*K <= 255.  Every refused tensor is at
    least as large as the one the kernel would have used."""
    L = lib()
    x, y = _bf(dev, 2, 5, 4, 8), _bf(dev, 2, 3, 2, 8)
    idx = torch.zeros(2, 3, 2, 8, device=dev, dtype=U8)
    L.maxpool_fwd(x, y, idx, 3, 2, 1)  # the accepted call
    L.maxpool_bwd(y, idx, torch.empty_like(x), 3, 2, 1)
    for fn in (lambda *a: L.maxpool_fwd(x, *a), lambda y_, i_, *a: L.maxpool_bwd(y_, i_, torch.empty_like(x), *a)):
        with pytest.raises(RuntimeError, match="idx"):
            fn(y, idx.int(), 3, 2, 1)
        with pytest.raises(RuntimeError, match="idx"):
            fn(y, torch.zeros(2 * idx.numel(), device=dev, dtype=U8), 3, 2, 1)
        with pytest.raises(RuntimeError, match="idx"):
            fn(y, torch.zeros(2, 3, 2, 16, device=dev, dtype=U8)[..., ::2], 3, 2, 1)
        with pytest.raises(RuntimeError, match="N and C"):
            fn(_bf(dev, 3, 3, 2, 8), torch.zeros(3, 3, 2, 8, device=dev, dtype=U8), 3, 2, 1)
        with pytest.raises(RuntimeError, match="N and C"):
            fn(_bf(dev, 2, 3, 2, 16), torch.zeros(2, 3, 2, 16, device=dev, dtype=U8), 3, 2, 1)
        with pytest.raises(RuntimeError, match="extent"):
            fn(_bf(dev, 2, 4, 2, 8), torch.zeros(2, 4, 2, 8, device=dev, dtype=U8), 3, 2, 1)
        with pytest.raises(RuntimeError, match="extent"):
            fn(_bf(dev, 2, 3, 3, 8), torch.zeros(2, 3, 3, 8, device=dev, dtype=U8), 3, 2, 1)
    x16 = _bf(dev, 1, 16, 16, 8)
    y1, i1 = _bf(dev, 1, 1, 1, 8), torch.zeros(1, 1, 1, 8, device=dev, dtype=U8)
    with pytest.raises(RuntimeError, match="255"):
        L.maxpool_fwd(x16, y1, i1, 16, 1, 0)
    with pytest.raises(RuntimeError, match="255"):
        L.maxpool_bwd(y1, i1, torch.empty_like(x16), 16, 1, 0)


def test_avgpool_guards(dev):
    """y (forward) must be contiguous: a strided view of the right size and dtype is refused.
    (The device checks are not exercised: a tensor on another device is host memory here, which
    an unguarded kernel could not have touched safely.)"""
    x = _bf(dev, 3, 1, 7, 8)
    lib().avgpool_fwd(x, _bf(dev, 3, 8))
    with pytest.raises(RuntimeError, match="contiguous"):
        lib().avgpool_fwd(x, _bf(dev, 3, 16)[:, ::2])
    lib().avgpool_bwd(_bf(dev, 3, 8), torch.empty_like(x))
    with pytest.raises(RuntimeError):
        lib().avgpool_bwd(_bf(dev, 3, 16)[:, ::2], torch.empty_like(x))


def test_bn_eval_coeffs_guards(dev):
    C = 24
    v = lambda n=C, dt=F32: torch.ones(n, device=dev, dtype=dt)
    lib().bn_eval_coeffs(v(), v(), v(), v(), 1e-5, v(), v())
    for pos in range(1, 6):  # each vector after gamma with C + 8 elements
        args = [v() for _ in range(6)]
        args[pos] = v(C + 8)
        with pytest.raises(RuntimeError, match="C elements"):
            lib().bn_eval_coeffs(*args[:4], 1e-5, *args[4:])
    with pytest.raises(RuntimeError, match="C elements"):
        lib().bn_eval_coeffs(v(C + 8), v(), v(), v(), 1e-5, v(C + 8), v(C + 8))  # gamma sets C
    for pos in range(6):
        args = [v() for _ in range(6)]
        args[pos] = v(C, F64)
        with pytest.raises(RuntimeError, match="fp32"):
            lib().bn_eval_coeffs(*args[:4], 1e-5, *args[4:])
