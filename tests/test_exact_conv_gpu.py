"""Element-exact tests of the ResNet conv kernel family (conv_igemm / conv_halo / conv_pipe /
conv_res64 / conv_stem / wgrad_halo / wgrad_res64) on small-integer operands.

Every product and partial sum is exactly representable (tests/test_exact_conv_cpu.py asserts
the preconditions for each case here), so every result must equal the float64 tap-loop
reference of tests/exact_conv.py bit for bit, element by element, in any accumulation order.
Outputs are NaN-prefilled views between guard regions (a missed element or a write past the
tensor shows); inputs sit between NaN guards (a read past an operand that reaches a MAC
poisons the result).  Where a cfg does not take a shape and the dispatcher falls back the
result must still be exact; where the binding refuses the shape it must raise.  Which kernel
runs is asserted too (conv_route_info / wgrad_route_info against the limits restated below):
the specialised family where the shape fits, the documented fallback tile where it does not,
so a silent fallback fails."""
import functools

import pytest
import torch

import exact_conv as ec
from dmlab.ops._native import lib
from dmlab.ops.convbn import _cpad

pytestmark = pytest.mark.gpu

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
FWD_CFGS = list(range(9, 18)) + [39, 41, 42, 80, 90, 91, 92, 93]
HALO_CFGS = [39, 41, 42]
PIPE_BN = {90: 256, 91: 128, 92: 128, 93: 64}  # column tile of the pipelined cfgs
S2_CFGS = list(range(11, 18)) + [90, 91, 92, 93]
geoms = functools.partial(pytest.mark.parametrize, ids=ec.geom_id)


def _skip_wide(cfg, ncols):
    if cfg in (9, 12, 15) and ncols % 128:
        pytest.skip("128-wide tile needs Cout % 128 == 0")


# ---- the support limits the kernels document (the contracts of csrc's *_supported predicates),
# restated here so that a predicate which drifts shows as a refusal or a computation the test
# did not expect
def _halo_ok(W, cin, k, s, p):
    """Halo-staged unit-stride tiles: 64-channel chunks, taps within +-1, and the halo of a
    128- / 256-pixel run starting at a row's last pixel within 384 / 448 LDS rows."""
    rows = lambda bm: ((W - 1 + bm - 1) // W + 3) * W
    return s == 1 and cin % 64 == 0 and (k, p) in ((3, 1), (1, 0)) and rows(128) <= 384 and rows(256) <= 448


def _res64_ok(geom):
    N, H, W, Cin, Cout, k, s, p = geom
    return (Cin, Cout, k, s, p) == (64, 64, 3, 1, 1) and W <= 63


def _pipe_ok(cfg, cin, ncols):
    return cin % 64 == 0 and cin <= 2048 and ncols % PIPE_BN[cfg] == 0


def _wgrad_halo_ok(geom):
    N, H, W, Cin, Cout, k, s, p = geom
    return (k, s, p) == (3, 1, 1) and Cin % 64 == 0 and 64 + 2 * W + 2 <= 192


def _wgrad_res64_ok(geom):
    N, H, W, Cin, Cout, k, s, p = geom
    return (Cin, Cout, k, s, p) == (64, 64, 3, 1, 1) and W <= 60


def _wgrad_s2_ok(geom):
    """Stride-2 3x3/p1 over the parity planes of an even image, output rows up to 31 wide."""
    N, H, W, Cin, Cout, k, s, p = geom
    return (k, s, p) == (3, 2, 1) and H % 2 == 0 and W % 2 == 0 and Cin % 64 == 0 and W // 2 <= 31


# ---- the kernel each launch must run on: (family, tile), or None where it must be refused
REFUSED = None
IGEMM_FALLBACK = {39: -1, 41: -1, 42: 12}  # halo cfg -> igemm tile (csrc/conv_cfg.h fallback)


def _conv_route(geom, cfg, dgrad=False, pre=False, red=False):
    """One geometry (forward, or the stride-1 data gradient, whose GEMM reads Cout channels and
    writes Cin columns).  No fallback tile takes a pre-BN operand or the reduction epilogue."""
    N, H, W, Cin, Cout, k, s, p = geom
    cin, ncols = (Cout, Cin) if dgrad else (Cin, Cout)
    special = pre or red
    if cfg == 80:
        return ("res64", 80) if _res64_ok(geom) else REFUSED
    if cfg in HALO_CFGS or (pre and cfg in PIPE_BN):  # a pre-BN launch on 90-93 runs on 41
        row = 41 if cfg in PIPE_BN else cfg
        if red and row != 42:
            return REFUSED
        if _halo_ok(W, cin, k, s, p):
            return ("halo", row)
        return REFUSED if special else ("igemm", IGEMM_FALLBACK[cfg])
    if cfg in PIPE_BN:
        if _pipe_ok(cfg, cin, ncols):
            return ("pipe", cfg)
        return REFUSED if special else ("igemm", -2 if ncols % 128 == 0 else -1)
    return REFUSED if special else ("igemm", cfg)


def _wgrad_route(geom, cfg, pre=False):
    Cout = geom[4]
    if cfg == 8:
        return ("res64", 8) if _wgrad_res64_ok(geom) else REFUSED
    fits = {4: _wgrad_halo_ok, 5: _wgrad_halo_ok, 7: _wgrad_s2_ok}.get(cfg)
    if fits is None:
        return REFUSED if pre else ("v2", cfg)
    if fits(geom) and not (pre and cfg == 7):
        return ("s2" if cfg == 7 else "halo", cfg)
    return REFUSED if pre else ("v2", 2 if Cout % 128 == 0 else 3)


def _assert_route(got, want, what):
    family, tile, ok = got
    if want is REFUSED:
        assert not ok, f"{what}: must be refused, routed to {family} {tile}"
    else:
        assert ok and (family, tile) == want, f"{what}: runs on {got}, expected {want}"


# ---- device operands of one case, each between NaN (0xFF) guards, shared by the tests
class DevCase:
    def __init__(self, dev, geom):
        N, H, W, Cin, Cout, k, s, p = geom
        self.dev, self.geom = dev, geom
        self.c, self.r = ec.int_case(geom), ec.case_refs(geom)
        self._checks = []
        c, cp = self.c, _cpad(Cin)
        assert cp == Cin
        self.xn = self._in((N, H, W, cp), BF, "xn")
        lib().pack_input(c.x.permute(0, 3, 1, 2).contiguous().to(dev), self.xn)
        self.wf = self._in((Cout, k, k, cp), BF, "wf")
        self.wd = self._in((Cin, k, k, Cout), BF, "wd")
        lib().pack_weights(c.w.to(dev), self.wf, self.wd, cp)
        ec.assert_exact(self.xn, c.x, "pack_input")
        ec.assert_exact(self.wf, c.w.permute(0, 2, 3, 1), "pack_weights wf", layout="")
        ec.assert_exact(self.wd, c.w.permute(1, 2, 3, 0), "pack_weights wd", layout="")
        for n in ("dy", "add_y", "add_x", "red_y"):
            setattr(self, n, self._in(None, BF, n, getattr(c, n)))
        for n in ("pre_scale", "pre_shift", "red_scale", "red_shift", "red_mean", "red_invstd"):
            setattr(self, n, self._in(None, F32, n, getattr(c, n)))
        self.keep_add = self._in(None, U8, "keep_add", ec.pack_bits(c.keep_add))
        self.red_keep = self._in(None, U8, "red_keep", ec.pack_bits(c.red_keep))
        if ec.has_projection(geom):
            self.dy2 = self._in(None, BF, "dy2", c.dy2)
            self.wd2 = self._in((Cin, 1, 1, Cout), BF, "wd2")
            lib().pack_weights(c.w2.to(dev), torch.empty(Cout, 1, 1, cp, device=dev, dtype=BF),
                               self.wd2, cp)
            ec.assert_exact(self.wd2, c.w2.permute(1, 2, 3, 0), "pack_weights wd2", layout="")
        self.check_inputs()

    def _in(self, shape, dtype, name, src=None):
        v, chk = ec.guarded(tuple(src.shape) if src is not None else shape, dtype, self.dev, "in")
        if src is not None:
            v.copy_(src.to(self.dev))
        self._checks.append((name, chk))
        return v

    def check_inputs(self):
        for name, chk in self._checks:
            chk(f"input {name}")

    def out(self, shape, dtype=BF):
        return ec.guarded(tuple(shape), dtype, self.dev, "out")


@functools.lru_cache(maxsize=None)
def _case(dev, geom):
    return DevCase(dev, geom)


def _stats_sum(buf, rows, C):
    """Sum over the per-tile rows of a [rows][2][C] fp32 slab, in float64 (a row that was not
    written is NaN and poisons the sum)."""
    return buf.view(rows, 2, C).double().sum(0)


# ------------------------------------------------------------------ forward
def _fwd(d, cfg, add, pre, supported):
    N, H, W, Cin, Cout, k, s, p = d.geom
    want = _conv_route(d.geom, cfg, pre=pre)
    assert supported == (want is not REFUSED)
    _assert_route(lib().conv_route_info(N, H, W, Cin, Cout, k, s, p, cfg, add=add, pre=pre), want,
                  f"fwd cfg {cfg} add={add} pre={pre}")
    OH, OW = ec.out_hw(d.geom)
    M = N * OH * OW
    y, ychk = d.out((N, OH, OW, Cout))
    T = lib().conv_stats_rows(M, cfg, Cout)
    stats, schk = d.out((T * 2 * Cout,), F32)
    kw = dict(pre_scale=d.pre_scale, pre_shift=d.pre_shift) if pre else {}
    call = lambda: lib().conv_fwd(d.xn, d.wf, y, stats, d.add_y if add else None, k, k, s, p, cfg, **kw)
    if not supported:
        with pytest.raises(RuntimeError):
            call()
        return
    call()
    what = f"fwd cfg {cfg} add={add} pre={pre}"
    ychk(f"{what}: y")
    schk(f"{what}: stats")
    d.check_inputs()
    want = getattr(d.r, "y" + ("_pre" if pre else "") + ("_add" if add else ""))
    ec.assert_exact(y, want, f"{what}: y")
    # Σy and Σy² are those of the conv itself (the fp32 tile before the add)
    ec.assert_exact(_stats_sum(stats, T, Cout), d.r.stats_pre if pre else d.r.stats,
                    f"{what}: Σy, Σy² [2][Cout]")


@geoms("geom", ec.GEOMS)
@pytest.mark.parametrize("cfg", FWD_CFGS)
@pytest.mark.parametrize("add", [False, True])
def test_fwd_exact(dev, geom, cfg, add):
    """y (+ add) and the summed statistics rows; cfg 80 refuses what it does not take."""
    _skip_wide(cfg, geom[4])
    _fwd(_case(dev, geom), cfg, add, False, cfg != 80 or _res64_ok(geom))


@geoms("geom", ec.GEOMS)
@pytest.mark.parametrize("cfg", HALO_CFGS + [80, 90, 91, 92, 93])
@pytest.mark.parametrize("add", [False, True])
def test_fwd_prebn_exact(dev, geom, cfg, add):
    """Fused relu(x*scale + shift) staging (halo cfgs and cfg 80; 90-93 are routed to 41):
    y, Σy and Σy² exact; shapes the halo kernels do not take are refused."""
    N, H, W, Cin, Cout, k, s, p = geom
    ok = _res64_ok(geom) if cfg == 80 else _halo_ok(W, Cin, k, s, p)
    _fwd(_case(dev, geom), cfg, add, True, ok)


# ------------------------------------------------------------------ data gradient
UNCHECKED = object()  # a refusal that is the binding's operand check, not a route


def _dgrad(d, cfg, mode, supported=True, red=None, route=UNCHECKED):
    """mode: plain | acc (in place) | masked (add + 1-bit add_mask) | merged (dy2 / wd2).
    red: None, "y" (mask from red_y*scale + shift > 0) or "bits" (1-bit red_mask).
    route: the (family, tile) the launch must run on, REFUSED, or UNCHECKED."""
    N, H, W, Cin, Cout, k, s, p = d.geom
    dx, xchk = d.out((N, H, W, Cin))
    add, kw = None, {}
    if mode == "acc":
        dx.copy_(d.add_x)
        add = dx
    elif mode == "masked":
        add, kw["add_mask"] = d.add_x, d.keep_add
    elif mode == "merged":
        # (a geometry without a projection passes well-formed stand-ins: it must be refused)
        kw.update(dy2=getattr(d, "dy2", d.dy), wd2=getattr(d, "wd2", d.wd))
    part = None
    if red:
        rows = (lib().conv_stats_rows(N * H * W, cfg, Cin) if s == 1
                else lib().dgrad_s2_red_rows(N, H, W, cfg))
        part, pchk = d.out((rows * 2 * Cin,), F32)
        kw.update(red_y=d.red_y, red_scale=d.red_scale, red_shift=d.red_shift, red_mean=d.red_mean,
                  red_invstd=d.red_invstd, red_part=part)
        if red == "bits":
            kw["red_mask"] = d.red_keep
    if route is not UNCHECKED:
        assert supported == (route is not REFUSED)
        _assert_route(lib().conv_route_info(N, H, W, Cin, Cout, k, s, p, cfg, add=add is not None,
                                            red=bool(red), dgrad=True, merged=mode == "merged"),
                      route, f"dgrad cfg {cfg} {mode} red={red}")
    call = lambda: lib().conv_dgrad(d.dy, d.wd, dx, k, k, s, p, add, cfg, **kw)
    if not supported:
        with pytest.raises(RuntimeError):
            call()
        return
    call()
    what = f"dgrad cfg {cfg} {mode} red={red}"
    xchk(f"{what}: dx")
    d.check_inputs()
    name = {"plain": "dx", "acc": "dx_acc", "masked": "dx_masked", "merged": "dx_merged"}[mode]
    ec.assert_exact(dx, getattr(d.r, name), f"{what}: dx")
    if red:
        pchk(f"{what}: red_part")
        ec.assert_exact(_stats_sum(part, rows, Cin), d.r.red[(name, red)],
                        f"{what}: Σdz, Σdz·x̂ [2][Cin]")


@geoms("geom", ec.GEOMS_S1)
@pytest.mark.parametrize("cfg", FWD_CFGS)
@pytest.mark.parametrize("mode", ["plain", "acc"])
def test_dgrad_s1_exact(dev, geom, cfg, mode):
    _skip_wide(cfg, geom[3])
    _dgrad(_case(dev, geom), cfg, mode, cfg != 80 or _res64_ok(geom),
           route=_conv_route(geom, cfg, dgrad=True))


@geoms("geom", ec.GEOMS_S1)
@pytest.mark.parametrize("cfg", [80, 42, 39, 90, 13])
def test_dgrad_s1_masked_add_exact(dev, geom, cfg):
    """Fused identity skip: dx = dgrad(dy) + add where the 1-bit mask is set."""
    _dgrad(_case(dev, geom), cfg, "masked", cfg != 80 or _res64_ok(geom),
           route=_conv_route(geom, cfg, dgrad=True))


@geoms("geom", ec.GEOMS_STRIDE2)
@pytest.mark.parametrize("cfg", S2_CFGS)
@pytest.mark.parametrize("mode", ["plain", "acc", "merged"])
def test_dgrad_s2_exact(dev, geom, cfg, mode):
    """The parity classes of a stride-2 data gradient (1x1/s2: the empty classes are
    zero-filled), in place, and with the 1x1/s2 projection merged into class (0,0)."""
    N, H, W, Cin, Cout, k, s, p = geom
    _skip_wide(cfg, Cin)
    # the classes' one launch: the igemm tiles always; a pipelined tile where it fits, else one
    # launch per class (tile 0), which takes no merged segment
    ok, route = True, ("igemm", cfg)
    if cfg in PIPE_BN:
        route = ("pipe", cfg if _pipe_ok(cfg, Cout, Cin) else 0)
    if mode == "merged":
        if not ec.has_projection(geom):
            ok, route = False, UNCHECKED  # only a 3x3/s2/p1 data gradient merges: refused
        elif route == ("pipe", 0):
            ok, route = False, REFUSED  # a pipelined tile that does not fit is refused
    _dgrad(_case(dev, geom), cfg, mode, ok, route=route)


@geoms("geom", ec.GEOMS_S1)
@pytest.mark.parametrize("cfg", [80, 42, 90, 91, 92, 93])
@pytest.mark.parametrize("masked", [False, True])
def test_dgrad_s1_bn_reduce_exact(dev, geom, cfg, masked):
    """The consumer BN's backward reduction in the dgrad epilogue: mask from y*scale + shift,
    or the 1-bit red_mask together with the fused masked add; dx and the summed rows exact."""
    N, H, W, Cin, Cout, k, s, p = geom
    ok = (_res64_ok(geom) if cfg == 80 else _halo_ok(W, Cout, k, s, p) if cfg == 42
          else _pipe_ok(cfg, Cout, Cin))
    _dgrad(_case(dev, geom), cfg, "masked" if masked else "plain", ok, "bits" if masked else "y",
           route=_conv_route(geom, cfg, dgrad=True, red=True))


@geoms("geom", ec.GEOMS_STRIDE2)
@pytest.mark.parametrize("cfg", [13, 93])
@pytest.mark.parametrize("src", ["y", "bits"])
@pytest.mark.parametrize("mode", ["plain", "merged"])
def test_dgrad_s2_bn_reduce_exact(dev, geom, cfg, src, mode):
    """Stride 2 on an igemm and a pipelined tile, alone and with the merged projection; a
    data gradient with empty parity classes (1x1/s2) has no complete dx to reduce: refused."""
    _dgrad(_case(dev, geom), cfg, mode, ec.has_projection(geom), src)


# ------------------------------------------------------------------ weight gradient
def _wgrad(d, cfg, S, beta, pre, supported=True):
    N, H, W, Cin, Cout, k, s, p = d.geom
    want = _wgrad_route(d.geom, cfg, pre)
    # (cfg 8 also refuses a slab count past the image rows: the route exists, the launcher's
    # own guard raises)
    assert supported == (want is not REFUSED) or (cfg == 8 and not supported)
    _assert_route(lib().wgrad_route_info(N, H, W, Cin, Cout, k, s, p, cfg, pre=pre), want,
                  f"wgrad cfg {cfg} pre={pre}")
    K = k * k * _cpad(Cin)
    dw, wchk = d.out((Cout, Cin, k, k), F32)
    slab, schk = d.out((S * Cout * K,), F32)
    if beta:
        dw.copy_(d.c.dw_base)
    kw = dict(pre_scale=d.pre_scale, pre_shift=d.pre_shift) if pre else {}
    call = lambda: lib().conv_wgrad(d.xn, d.dy, dw, slab, Cin, k, k, s, p, float(beta), S, cfg,
                                    False, **kw)
    if not supported:
        with pytest.raises(RuntimeError):
            call()
        return
    call()
    what = f"wgrad cfg {cfg} S={S} beta={beta} pre={pre}"
    wchk(f"{what}: dw")
    schk(f"{what}: slab")
    d.check_inputs()
    want = getattr(d.r, "dw" + ("_pre" if pre else "") + ("_base" if beta else ""))
    ec.assert_exact(dw, want, f"{what}: dw", layout="oikk")


@geoms("geom", ec.GEOMS)
@pytest.mark.parametrize("cfg", [2, 3, 6, 4, 5])
def test_wgrad_exact(dev, geom, cfg):
    """The igemm tiles (2, 3, 6) and the halo tiles (4, 5; other shapes fall back) with
    split-m slabs ending mid-row and mid-image, beta 0 and 1 onto an integer base."""
    if cfg == 2 and geom[4] % 128:
        pytest.skip("128-wide tile needs Cout % 128 == 0")
    d = _case(dev, geom)
    for S in (1, 3, 7):
        for beta in (0, 1):
            _wgrad(d, cfg, S, beta, False)


@geoms("geom", ec.GEOMS)
@pytest.mark.parametrize("cfg", [4, 5])
def test_wgrad_prebn_exact(dev, geom, cfg):
    d = _case(dev, geom)
    for S, beta in ((1, 0), (3, 1)):
        _wgrad(d, cfg, S, beta, True, _wgrad_halo_ok(geom))


@geoms("geom", ec.GEOMS_STRIDE2 + ec.GEOMS_WGRAD_S2)
def test_wgrad_s2_exact(dev, geom):
    """wgrad cfg 7 over the input parity planes: even non-square images up to Wg = 31; odd
    sizes, 1x1 taps and Wg = 32 fall back."""
    d = _case(dev, geom)
    for S in (1, 3, 7):
        for beta in (0, 1):
            _wgrad(d, 7, S, beta, False)


@geoms("geom", ec.GEOMS_S1)
@pytest.mark.parametrize("pre", [False, True])
def test_wgrad_res64_exact(dev, geom, pre):
    """Row-streaming cfg 8: one workgroup, a prime count, one workgroup per image row; more
    slabs than rows and shapes past W = 60 are refused."""
    N, H, W, Cin, Cout, k, s, p = geom
    d = _case(dev, geom)
    ok = _wgrad_res64_ok(geom)
    for S in sorted({1, min(5, N * H), N * H}):
        for beta in (0, 1):
            _wgrad(d, 8, S, beta, pre, ok)
    _wgrad(d, 8, N * H + 1, 0, pre, False)


# ------------------------------------------------------------------ stem (space-to-depth)
@pytest.mark.parametrize("cfg", [16, 60])
def test_stem_s2d_exact(dev, cfg):
    """7x7/s2/p3 stem == 4x4/s1 conv over the space-to-depth packed input: y, statistics and
    the weight gradient through the s2d reduce."""
    geom = ec.STEM_GEOM
    N, H, W, C, Co, k, s, p = geom
    c, r = ec.int_case(geom), ec.case_refs(geom)
    xs, xchk = ec.guarded((N, H // 2, W // 2, 16), BF, dev, "in")
    lib().pack_input_s2d(c.x.permute(0, 3, 1, 2).contiguous().to(dev), xs)
    wf, fchk = ec.guarded((Co, 4, 4, 16), BF, dev, "in")
    lib().pack_weights_s2d(c.w.to(dev), wf)
    dy, dchk = ec.guarded(tuple(c.dy.shape), BF, dev, "in")
    dy.copy_(c.dy.to(dev))
    want_xs = torch.zeros(N, H // 2, W // 2, 16, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            want_xs[..., (a * 2 + b) * 3:(a * 2 + b) * 3 + 3] = c.x[:, a::2, b::2, :]
    ec.assert_exact(xs, want_xs, "pack_input_s2d")
    y, ychk = ec.guarded((N, H // 2, W // 2, Co), BF, dev, "out")
    M = N * (H // 2) * (W // 2)
    T = lib().conv_stats_rows(M, cfg, Co)
    stats, schk = ec.guarded((T * 2 * Co,), F32, dev, "out")
    lib().conv_fwd(xs, wf, y, stats, None, 4, 4, 1, 2, cfg)
    for chk, n in ((ychk, "y"), (schk, "stats"), (xchk, "xs"), (fchk, "wf")):
        chk(f"stem cfg {cfg}: {n}")
    ec.assert_exact(y, r.y, f"stem cfg {cfg}: y")
    ec.assert_exact(_stats_sum(stats, T, Co), r.stats, f"stem cfg {cfg}: Σy, Σy²")
    for wcfg in (3, 6):
        for S in (1, 4):
            for beta in (0, 1):
                dw, wchk = ec.guarded((Co, C, 7, 7), F32, dev, "out")
                slab, lchk = ec.guarded((S * Co * 256,), F32, dev, "out")
                if beta:
                    dw.copy_(c.dw_base)
                lib().conv_wgrad(xs, dy, dw, slab, C, 4, 4, 1, 2, float(beta), S, wcfg, True)
                what = f"stem wgrad cfg {wcfg} S={S} beta={beta}"
                for chk, n in ((wchk, "dw"), (lchk, "slab"), (xchk, "xs"), (dchk, "dy")):
                    chk(f"{what}: {n}")
                ec.assert_exact(dw, r.dw_base if beta else r.dw, f"{what}: dw", layout="oikk")
