"""CPU side of the element-exact conv suite (tests/exact_conv.py): the exactness preconditions
of every case the GPU file runs, and self-tests of the references, the guards, the exact
compare and the mask packer."""
import pytest
import torch
import torch.nn.functional as F

import exact_conv as ec


@pytest.mark.parametrize("geom", ec.ALL_GEOMS, ids=ec.geom_id)
def test_exact_preconditions(geom):
    """The data of every GPU case keeps bf16 results integral within 256 and fp32 results
    (and the sums of their terms' magnitudes) below 2^24."""
    seen = ec.exact_preconditions(ec.int_case(geom))
    assert seen["y"] > 0 and seen["dx"] > 0 and seen["dw"] > 0


def test_int_case_recipe_and_determinism():
    geom = ec.GEOMS_CHUNKS[0]
    N, H, W, Cin, Cout, k, s, p = geom
    c = ec.int_case(geom)
    assert set(c.x.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(c.w.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert torch.equal((c.w != 0).sum((1, 2, 3)), torch.full((Cout,), min(Cin * k * k, 48)))
    assert set(c.red_invstd.unique().tolist()) <= {0.5, 1.0, 2.0}
    ec.int_case.cache_clear()
    d = ec.int_case(geom)
    for n in ("x", "w", "dy", "add_y", "add_x", "keep_add", "red_y", "red_keep", "dw_base"):
        assert torch.equal(getattr(c, n), getattr(d, n)), n
    assert not torch.equal(ec.int_case(geom, 1).x, c.x)
    one = ec.int_case((2, 5, 9, 64, 256, 1, 1, 0))  # K = 64 >= 48; the stem has K = 147
    assert torch.equal((one.w != 0).sum((1, 2, 3)), torch.full((256,), 48))


def _nchw(a):
    return a.permute(0, 3, 1, 2).contiguous()


def _nhwc(a):
    return a.permute(0, 2, 3, 1).contiguous()


# non-square, stride-2 with odd sizes, 1x1/s2, tiny, 7x7/s2/p3
REF_GEOMS = [(2, 5, 11, 8, 16, 3, 1, 1), (2, 9, 14, 8, 16, 3, 2, 1), (2, 14, 9, 8, 16, 3, 2, 1),
             (2, 9, 14, 8, 16, 1, 2, 0), (3, 2, 3, 8, 8, 3, 1, 1), (1, 1, 1, 8, 8, 3, 1, 1),
             (2, 16, 24, 3, 8, 7, 2, 3), (2, 10, 6, 8, 8, 3, 2, 1)]


@pytest.mark.parametrize("geom", REF_GEOMS, ids=ec.geom_id)
def test_refs_match_torch_float64(geom):
    """The tap-loop references equal torch's float64 convolution and its gradients (exactly:
    the operands are integers), with add, pre-BN, masked add, projection and base."""
    N, H, W, Cin, Cout, k, s, p = geom
    c = ec.int_case(geom, seed=3)
    x, w, dy = _nchw(c.x).double(), c.w.double(), _nchw(c.dy).double()
    assert torch.equal(ec.ref_fwd(geom, c.x, c.w), _nhwc(F.conv2d(x, w, None, s, p)))
    assert torch.equal(ec.ref_fwd(geom, c.x, c.w, add=c.add_y),
                       _nhwc(F.conv2d(x, w, None, s, p)) + c.add_y.double())
    a = torch.relu(c.x.double() * c.pre_scale.double() + c.pre_shift.double())
    pre = (c.pre_scale, c.pre_shift)
    assert torch.equal(ec.ref_fwd(geom, c.x, c.w, pre=pre), _nhwc(F.conv2d(_nchw(a), w, None, s, p)))
    dx = _nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), w, dy, s, p))
    assert torch.equal(ec.ref_dgrad(geom, c.dy, c.w), dx)
    assert torch.equal(ec.ref_dgrad(geom, c.dy, c.w, add=c.add_x), dx + c.add_x.double())
    assert torch.equal(ec.ref_dgrad(geom, c.dy, c.w, add=c.add_x, keep=c.keep_add),
                       dx + c.add_x.double() * c.keep_add)
    if ec.has_projection(geom):
        dx2 = _nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), c.w2.double(), _nchw(c.dy2).double(), 2, 0))
        assert torch.equal(ec.ref_dgrad(geom, c.dy, c.w, dy2=c.dy2, w2=c.w2), dx + dx2)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, s, p)
    assert torch.equal(ec.ref_wgrad(geom, c.x, c.dy), dw)
    assert torch.equal(ec.ref_wgrad(geom, c.x, c.dy, base=c.dw_base), dw + c.dw_base.double())
    assert torch.equal(ec.ref_wgrad(geom, c.x, c.dy, pre=pre),
                       torch.nn.grad.conv2d_weight(_nchw(a), w.shape, dy, s, p))
    assert (ec.ref_wgrad(geom, c.x, c.dy, absolute=True) >= dw.abs()).all()


def test_ref_stats_and_bn_reduce():
    c = ec.int_case(REF_GEOMS[0], seed=3)
    y = ec.ref_fwd(c.geom, c.x, c.w)
    st = ec.ref_stats(y)
    flat = y.reshape(-1, y.shape[-1])
    assert torch.equal(st[0], flat.sum(0)) and torch.equal(st[1], (flat * flat).sum(0))
    dx = ec.ref_dgrad(c.geom, c.dy, c.w)
    keep = ec.relu_keep(c)
    assert torch.equal(keep, torch.relu(c.red_y * c.red_scale + c.red_shift) > 0)
    got = ec.ref_bn_reduce(dx, keep, c.red_y, c.red_mean, c.red_invstd)
    dz = torch.where(keep, dx, torch.zeros((), dtype=torch.float64))
    xhat = (c.red_y.double() - c.red_mean.double()) * c.red_invstd.double()
    assert torch.equal(got[0], dz.sum((0, 1, 2)))
    assert torch.equal(got[1], (dz * xhat).sum((0, 1, 2)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8])
@pytest.mark.parametrize("fill", ["out", "in"])
def test_guarded_flags_writes_on_either_side(dtype, fill):
    shape = (3, 5, 7, 8)  # 840 elements: a bf16 body that is not a multiple of 16 bytes + 8
    cpu = torch.device("cpu")
    t, check = ec.guarded(shape, dtype, cpu, fill)
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and t.data_ptr() % 16 == 0
    if dtype != torch.uint8:
        assert torch.isnan(t).all()  # outputs start as NaN; inputs are overwritten by the caller
    t.copy_(torch.ones(shape).to(dtype))  # writing the whole tensor leaves the guards alone
    check("whole")
    flat = t.view(-1)
    base = flat.storage_offset() if dtype == torch.uint8 else None
    for off, side in ((-1, "below"), (flat.numel(), "above"), (-ec.GUARD, "below"),
                      (flat.numel() + ec.GUARD - 1, "above")):
        t2, check2 = ec.guarded(shape, dtype, cpu, fill)
        f2 = t2.view(-1)
        # a one-element write just outside the view, through a wider window on the same storage
        wide = torch.as_strided(f2, (f2.numel() + 2 * ec.GUARD,), (1,), f2.storage_offset() - ec.GUARD)
        wide[off + ec.GUARD] = 3
        with pytest.raises(AssertionError, match=side):
            check2("one element")
    assert base is None or base >= ec.GUARD


def test_guarded_inputs_poison_with_nan():
    t, _ = ec.guarded((4, 8), torch.bfloat16, torch.device("cpu"), "in")
    f = t.view(-1)
    wide = torch.as_strided(f, (f.numel() + 2,), (1,), f.storage_offset() - 1)
    t.zero_()
    assert torch.isnan(wide[0]) and torch.isnan(wide[-1]) and not torch.isnan(wide[1:-1]).any()
    m, _ = ec.guarded((16,), torch.uint8, torch.device("cpu"), "in")
    wm = torch.as_strided(m, (18,), (1,), m.storage_offset() - 1)
    m.zero_()
    assert int(wm[0]) == 0xFF and int(wm[-1]) == 0xFF


def test_assert_exact_reports_the_element():
    want = torch.arange(2 * 3 * 4 * 8, dtype=torch.float64).view(2, 3, 4, 8)
    ec.assert_exact(want.bfloat16(), want, "same")  # integers below 256 survive bf16
    got = want.clone()
    got[1, 2, 3, 5] += 1
    with pytest.raises(AssertionError) as e:
        ec.assert_exact(got, want, "one element")
    msg = str(e.value)
    assert "1 of 192 elements differ" in msg and "n=1, y=2, x=3, c=5" in msg
    assert "got 190.0 want 189.0" in msg and "affected x (1 of 4): [3]" in msg
    got = want.clone()
    got[0, 1, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"1 NaN[\s\S]*n=0, y=1, x=0, c=0"):
        ec.assert_exact(got, want, "unwritten")
    dw = torch.zeros(4, 3, 3, 3)
    bad = dw.clone()
    bad[2, 1, 0, 2] = 1
    with pytest.raises(AssertionError, match="co=2, ci=1, kh=0, kw=2"):
        ec.assert_exact(bad, dw, "dw", layout="oikk")
    with pytest.raises(AssertionError, match="shape"):
        ec.assert_exact(dw[:3], dw, "shape")


def test_pack_bits_matches_existing_tests():
    import test_native_resnet_kernels as tk
    import test_round6_gpu as t6

    keep = torch.rand(3, 5, 7, 64, generator=torch.Generator().manual_seed(5)) > 0.4
    got = ec.pack_bits(keep)
    assert torch.equal(got, tk._bits(keep)) and torch.equal(got, t6._bits(keep))
    flat = keep.reshape(-1)
    for i in (0, 1, 77, flat.numel() // 8 - 1):
        assert int(got[i]) == sum(int(flat[8 * i + j]) << j for j in range(8))
