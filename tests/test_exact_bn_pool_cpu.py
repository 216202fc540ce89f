"""CPU side of the element-exact BatchNorm / pooling suite (tests/exact_bn_pool.py): the
exactness preconditions of every case the GPU file runs, each reference against an independent
float64 route (F.batch_norm with autograd, F.max_pool2d / F.avg_pool2d on tie-free data), the
tie rule, and the tier-B bound against fp32 emulations of the kernels' formulas."""
import pytest
import torch
import torch.nn.functional as F

import exact_bn_pool as eb

ids = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _nchw(a):
    return a.permute(0, 3, 1, 2).contiguous()


def _nhwc(a):
    return a.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("shape", eb.APPLY_SHAPES, ids=ids)
def test_apply_preconditions(shape):
    """bn_apply's outputs and the crafted stage-2 dy / dres are bf16 numbers; exact zeros and
    negative pre-ReLU values occur."""
    c = eb.bn_case(*shape)
    seen = eb.apply_preconditions(c)
    assert 0 < seen["out"] <= 28
    seen = eb.apply2_preconditions(c)
    assert max(seen.values()) <= 30


@pytest.mark.parametrize("shape", eb.SUMS_SHAPES, ids=ids)
def test_sums_preconditions(shape):
    """(The (32785, 2048) case asserts the same on the device, where its operands live.)"""
    seen = eb.sums_preconditions(eb.bn_case(*shape))
    assert set(seen) == {0, 1, 2, 4}


@pytest.mark.parametrize("shape", eb.TIERB_SHAPES, ids=ids)
def test_tierb_sums_preconditions(shape):
    c = eb.tierb_of(eb.bn_case(*shape))
    assert (c.y.abs() >= 3 * c.mean.abs()).all() and (c.y == 0).any() and (c.y < 0).any()
    eb.sums_preconditions(c, invstd=c.invstdB)


@pytest.mark.parametrize("geom", eb.MAXPOOL_GEOMS + eb.FUSED_GEOMS, ids=ids)
def test_pool_preconditions(geom):
    seen = eb.pool_preconditions(eb.pool_case(geom))
    if geom[1] * geom[2] > 1:
        assert seen["ties"] > 0  # the tie rule is exercised
    if geom[1] * geom[2] >= 9:
        assert seen["code15"] > 0  # windows that pass no gradient occur


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("geom", eb.MODE3_GEOMS, ids=ids)
def test_mode3_preconditions(geom, C):
    c = eb.mode3_case(geom, C)
    eb.sums_preconditions(c, modes=(3,))
    eb.apply2_preconditions(c, modes=(3,))
    assert set(c.codes.unique().tolist()) <= set(range(geom[3] ** 2)) | {15}


def test_other_preconditions():
    for T in eb.STAT_T:
        for C in eb.STAT_C:
            assert eb.stat_preconditions(eb.stat_case(T, C)) <= 64 * T
    for HW in eb.AVG_HW:
        for C in eb.AVG_C:
            assert eb.avg_preconditions(eb.avg_case(HW, C)) <= 8 * HW


def test_preconditions_fail_when_a_range_is_widened():
    c = eb.bn_case(129, 64)
    wide = type(c)(**vars(c))
    wide.y = c.y * 16  # |y * scale| up to 256 at granularity 1/2: more than 8 significand bits
    with pytest.raises(AssertionError, match="bf16"):
        eb.apply_preconditions(wide)
    big = type(c)(**vars(c))
    big.dout = c.dout * 2.0 ** 20
    with pytest.raises(AssertionError, match="2\\^24"):
        eb.sums_preconditions(big)


def test_cases_are_deterministic():
    a = eb.bn_case(37, 64)
    eb.bn_case.cache_clear()
    b = eb.bn_case(37, 64)
    for n in ("y", "res", "dout", "scale", "shift", "mean", "invstd", "gamma"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert set(a.y.unique().tolist()) <= set(float(i) for i in range(-8, 9))
    assert set(a.scale.unique().tolist()) <= set(eb.SCALES)


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
def test_bn_references_against_autograd(relu, res):
    """ref_finalize / ref_apply / ref_bwd_sums / ref_coef against F.batch_norm in double."""
    M, C = 53, 16
    g = torch.Generator().manual_seed(1)
    y = torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + 0.5
    r = torch.randn(M, C, generator=g, dtype=torch.float64)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    dout = torch.randn(M, C, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, dtype=torch.float64, generator=g), torch.rand(C, dtype=torch.float64, generator=g) + 0.5
    yr, g_, b_ = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_t, rv_t = rm.clone(), rv.clone()
    z = F.batch_norm(yr.t().unsqueeze(0), rm_t, rv_t, g_, b_, True, eb.f32(eb.MOMENTUM), eb.f32(eb.EPS)).squeeze(0).t()
    z.retain_grad()
    t = z + r if res else z
    out = F.relu(t) if relu else t
    out.backward(dout)
    fin = eb.ref_finalize(y.sum(0), (y * y).sum(0), float(M), gamma, beta, rm, rv)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-12)
    close(fin.rmean, rm_t)
    close(fin.rvar, rv_t)
    mine = eb.ref_apply(y, fin.scale, fin.shift, res=r if res else None, relu=relu)
    close(mine, out.detach())
    dz = dout * (mine > 0) if relu else dout
    close(dz, z.grad)
    sums = eb.ref_bwd_sums(dz, y, fin.mean, fin.invstd)
    close(sums[0], b_.grad)
    close(sums[1], g_.grad)
    a, b, cc = eb.ref_coef(sums, M, gamma, fin.mean, fin.invstd)
    close(a * dz + b * y + cc, yr.grad)
    ref, bound = eb.tierb_bound(a, b, cc, dz, y)
    close(ref, yr.grad)
    assert (bound >= 0).all()


def test_finalize_count_one_and_sync_merge():
    S, Q = torch.tensor([3.0]).double(), torch.tensor([11.0]).double()
    one = torch.ones(1)
    fin = eb.ref_finalize(S, Q, 1.0, one, one, one, one)
    assert fin.var.item() == 2.0  # 11 - 9, and no division by count - 1
    assert abs(fin.rvar.item() - (0.9 + 0.1 * 2.0)) < 1e-7
    # three ranks of unequal counts merge to the statistics of the concatenation
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(n, 5, generator=g, dtype=torch.float64) + i for i, n in enumerate((1, 7, 40))]
    rows = torch.stack([eb.ref_sync_row(x.sum(0), (x * x).sum(0), float(len(x))) for x in xs])
    mean, var, N = eb.ref_sync_merge(rows)
    allx = torch.cat(xs)
    assert N == 48.0
    torch.testing.assert_close(mean, allx.mean(0), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(var, allx.var(0, unbiased=False), rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("geom", [(2, 7, 9, 8, 3, 2, 1), (1, 6, 6, 8, 2, 2, 0), (2, 5, 5, 8, 3, 1, 1)], ids=ids)
def test_pool_references_against_torch_on_tie_free_data(geom):
    N, H, W, C, K, S, P = geom
    g = torch.Generator().manual_seed(3)
    x = (torch.randperm(N * H * W * C, generator=g).double() + 1).view(N, H, W, C)  # distinct, > 0
    xr = _nchw(x).requires_grad_(True)
    want, ind = F.max_pool2d(xr, K, S, P, return_indices=True)
    best, code = eb.ref_maxpool_fwd(x, K, S, P)
    assert torch.equal(best, _nhwc(want.detach()))
    OH, OW = eb.pool_out(H, W, K, S, P)
    oh = torch.arange(OH).view(1, 1, OH, 1)
    ow = torch.arange(OW).view(1, 1, 1, OW)
    assert torch.equal(code, _nhwc((ind // W - (oh * S - P)) * K + (ind % W - (ow * S - P))))
    dy = torch.randn(N, OH, OW, C, generator=g, dtype=torch.float64)
    want.backward(_nchw(dy))
    torch.testing.assert_close(eb.ref_pool_gather(dy, code, H, W, K, S, P), _nhwc(xr.grad), rtol=1e-13, atol=1e-13)
    # the fused tail on positive data: no code 15, yarg is the input at the argmax
    one, zero = torch.ones(C), torch.zeros(C)
    fb, fc, fa = eb.ref_fused_pool(x, one, zero, K, S, P)
    assert torch.equal(fb, best) and torch.equal(fc, code) and torch.equal(fa, best)
    fb, fc, fa = eb.ref_fused_pool(x, -one, zero, K, S, P)  # every BN value < 0
    assert (fb == 0).all() and (fc == 15).all()


def test_tie_rule_on_a_hand_written_window():
    """First maximum in (kh, kw) scan order wins; taps outside the image never win; a window
    maximum of 0 gives code 15 with y at the first valid tap."""
    x = torch.tensor([[1.0, 3.0, 3.0], [3.0, 0.0, 2.0], [3.0, 3.0, 1.0]]).view(1, 3, 3, 1)
    best, code = eb.ref_maxpool_fwd(x, 3, 1, 0)
    assert best.item() == 3.0 and code.item() == 1
    best, code = eb.ref_maxpool_fwd(x, 3, 2, 1)  # windows at (-1, -1), (-1, 1), (1, -1), (1, 1)
    assert best.flatten().tolist() == [3.0, 3.0, 3.0, 3.0]
    assert code.flatten().tolist() == [5, 3, 1, 3]
    # a pixel named by all four windows over it collects all four gradients
    dy = torch.tensor([1.0, 2.0, 4.0, 8.0]).view(1, 2, 2, 1)
    codes = torch.tensor([8, 6, 2, 0], dtype=torch.uint8).view(1, 2, 2, 1)  # all name pixel (1, 1)
    dx = eb.ref_pool_gather(dy, codes, 3, 3, 3, 2, 1)
    assert dx[0, 1, 1, 0].item() == 15.0 and dx.sum().item() == 15.0
    codes[:] = 0  # code 0 names the padding for every window but (1, 1): only its gradient passes
    dx = eb.ref_pool_gather(dy, codes, 3, 3, 3, 2, 1)
    assert dx.sum().item() == 8.0 and dx[0, 1, 1, 0].item() == 8.0
    y = torch.tensor([[-5.0, -1.0], [-2.0, -3.0]]).view(1, 2, 2, 1)
    fb, fc, fa = eb.ref_fused_pool(y, torch.ones(1), torch.zeros(1), 2, 2, 0)
    assert fb.item() == 0.0 and fc.item() == 15 and fa.item() == -5.0


@pytest.mark.parametrize("HW", eb.AVG_HW)
def test_avgpool_references(HW):
    c = eb.avg_case(HW, 24)
    x4 = c.x.double().view(3, HW, 1, 24)
    want = F.avg_pool2d(_nchw(x4), (HW, 1)).view(3, 24)
    got = eb.ref_avg_fwd(c.x)
    assert torch.equal(got, want.float().bfloat16().double())
    assert torch.equal(got, (c.x.sum(1) / HW).bfloat16().double())  # the fp32 division itself
    back = eb.ref_avg_bwd(c.g, HW)
    assert back.shape == (3, HW, 24)
    inv = torch.tensor(1.0) / HW
    assert torch.equal(back[:, 0], (c.g * inv).bfloat16().double())  # fp32 product, then RNE


def test_ulp_and_compare_helpers():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0, -3.0])
    assert eb.ulp(v, 24).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 0.0, 2.0 ** -22]
    assert eb.ulp(v, 8).tolist()[:3] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    w = torch.tensor([1.0, 2.0]).double()
    eb.assert_ulps(w + 2.0 ** -23, w, 1, "ok")
    with pytest.raises(AssertionError, match="1 of 2"):
        eb.assert_ulps(w + 2.0 ** -22, w, 1, "one ulp too far")
    with pytest.raises(AssertionError):
        eb.assert_ulps(torch.tensor([float("nan"), 2.0]), w, 1, "nan")
    with pytest.raises(AssertionError, match="outside the bound"):
        eb.assert_within(torch.tensor([1.0, 2.5]), w, torch.tensor([0.1, 0.1]).double(), "bound")


# ------------------------------------------------------------------ tier B
def _tierb_check(c, mode):
    dz = eb.ref_dz(c, mode)
    sums = eb.ref_bwd_sums(dz, c.y, c.mean, c.invstdB)
    a, b, cc = eb.ref_coef(sums, c.M, c.gamma, c.mean, c.invstdB)
    ref, bound = eb.tierb_bound(a, b, cc, dz, c.y)
    rne = ref.float().bfloat16().double()
    worst, differ = 0.0, 0.0
    for variant in range(4):
        got = eb.emulate_whole_backward(sums, c.M, c.gamma, c.mean, c.invstdB, dz, c.y, variant)
        worst = max(worst, eb.assert_within(got, ref, bound, f"emulation {variant}"))
        differ = max(differ, (got != rne).double().mean().item())
    return worst, differ


@pytest.mark.parametrize("shape", eb.TIERB_SHAPES, ids=ids)
def test_tierb_bound_holds_for_fp32_emulations(shape):
    """Four fp32 evaluations of the kernels' formulas (unfused and three FMA contractions) stay
    within ulp_bf16(ref)/2 + 8 * 2^-24 * (|a*dz| + |b*y| + |c|) of the float64 reference at
    every shape the GPU test uses, and almost all elements are RNE(ref) itself."""
    c = eb.tierb_of(eb.bn_case(*shape))
    for mode in (0, 1, 2, 4):
        worst, differ = _tierb_check(c, mode)
        assert worst <= 1.0 and differ < 1e-2, (mode, worst, differ)


@pytest.mark.parametrize("geom", eb.TIERB_MODE3, ids=ids)
def test_tierb_bound_holds_for_mode3(geom):
    worst, differ = _tierb_check(eb.tierb_of(eb.mode3_case(geom, 64)), 3)
    assert worst <= 1.0 and differ < 1e-2
