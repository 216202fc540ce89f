"""Element-exact tests of the Linear GEMM family (csrc/gemm.hip) and the thin-conv family
(csrc/conv_small.hip).

Tier A: small-integer operands make every partial sum an exact fp32 number
(tests/test_exact_linear_cpu.py asserts the preconditions of each case here), so every result
must equal the float64 reference of tests/exact_linear.py bit for bit, whatever the MFMA order,
the split-K chunking, the batch slicing or the FMA contraction.  Tier B: Gaussian operands and
the bound (K + 4) * 2^-23 * sum|a||b| + half an ulp of the output type.  Every output is a
NaN-prefilled view between guard regions (an element that was not written, a beta = 0 that
multiplied instead of overwriting, or a write past the tensor shows); every input sits between
NaN guards.  The bindings' refusals are checked with arguments that even an unguarded kernel
would have kept inside its allocations."""
import pytest
import torch

import exact_conv as ec
import exact_linear as el
from dmlab.ops._native import lib

pytestmark = pytest.mark.gpu

BF, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
NAN = float("nan")


class Bench:
    """Guarded device tensors of one test; done() checks every guard."""

    def __init__(self, dev):
        self.dev, self.checks, self.inputs = dev, [], []

    def inp(self, t, dtype=None, what="operand"):
        v, chk = ec.guarded(tuple(t.shape), dtype or t.dtype, self.dev, "in")
        v.copy_(t.to(self.dev))
        self.inputs.append((chk, what))
        return v

    def out(self, shape, dtype, what="output", prior=None):
        v, chk = ec.guarded(tuple(shape), dtype, self.dev, "out")
        if prior is not None:
            v.copy_(prior.to(self.dev))
        self.checks.append((chk, what))
        return v

    def done(self):
        for chk, what in self.checks + self.inputs:
            chk(what)
        self.checks = []


def _exact(got, want, what):
    ec.assert_exact(got.reshape(want.shape), want, what, layout="")


def _exact_nan(got, want, what):
    """Exact where the reference is a number, NaN exactly where it is NaN."""
    g = got.detach().double().cpu().reshape(want.shape)
    gn, wn = torch.isnan(g), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN at {int(gn.sum())} elements, expected at {int(wn.sum())}; " \
                                f"first unexpected {(gn & ~wn).nonzero()[:4].tolist()}, first missing {(wn & ~gn).nonzero()[:4].tolist()}"
    zero = torch.zeros_like(g)
    ec.assert_exact(torch.where(gn, zero, g), torch.where(wn, zero, want), what, layout="")


def _all_ones_bits(t):
    """True when every byte of t is 0xFF (the NaN prefill, bit for bit)."""
    return bool((t.contiguous().view(U8) == 0xFF).all()) if t.numel() else True


# ------------------------------------------------------------------ GEMM
def run_gemm(dev, case, poison=None):
    M, N, K = case.M, case.N, case.K
    o, b = el.gemm_operands(case), Bench(dev)
    sam, sak, sbk, sbn, scm = el.strides_of(case)
    A, B = b.inp(o.A, what="A"), b.inp(o.B, what="B")
    if poison:
        (A if poison == "A" else B).view(-1)[0] = NAN
    mask = b.inp(o.Amask, what="Amask") if case.mask else None
    bias = b.inp(o.bias, what="bias") if case.bias else None
    C = b.out((M, scm), el.DT[case.tc], "C") if case.out in ("C", "both") else None
    C32 = b.out((M, scm), F32, "C32") if case.out in ("C32", "both") else None
    if case.beta != 0.0:  # the prior contents; with beta == 0 the NaN prefill must be overwritten
        src = C32 if C32 is not None else C
        src[:, :N] = o.prior.to(src.dtype).to(dev)
    lib().gemm(A, mask, B, C, C32, bias, M, N, K, sam, sak, sbk, sbn, scm, case.alpha, case.beta, case.relu,
               lowp=case.lowp)
    ref = el.gemm_ref_poisoned(case, poison) if poison else el.gemm_ref(case)
    what = el.gemm_id(case) + (f" poison {poison}" if poison else "")
    for name, t in (("C", C), ("C32", C32)):
        if t is None:
            continue
        (_exact_nan if poison else _exact)(t[:, :N], el.round_to(ref, t.dtype), f"{name} of {what}")
        assert _all_ones_bits(t[:, N:]), f"{name} of {what}: the gap between rows (scm > N) was written"
    b.done()


def _run_all(dev, cases):
    for case in dict.fromkeys(cases):
        run_gemm(dev, case)


def test_gemm_plan_binding_matches_the_table_and_the_mirror():
    """The split-K decision for the named shapes: a retune cannot silently move a case off the
    path it was written for.  (Host only, but it needs the extension.)"""
    for key, want in el.EXPECTED_PLANS.items():
        assert tuple(lib().gemm_plan(*key[:3], bool(key[3]), bool(key[4]))) == want, key
    for c in dict.fromkeys(el.all_gemm_cases()):
        assert tuple(lib().gemm_plan(c.M, c.N, c.K, c.ta == "b", c.lowp)) == el.case_plan(c), c


@pytest.mark.parametrize("kernel", ["f32mfma", "bf16mfma"])
@pytest.mark.parametrize("mn", el.MN_EDGE, ids=lambda v: "%dx%d" % v)
def test_gemm_edges_exact(dev, mn, kernel):
    """K in {1, 3, 31, 32, 33, 63, 64, 65, 129} x all four layouts at one (M, N): tile edges in m, n
    and k, the epilogue (alpha, beta, bias, relu, C / C32 / both, scm = N + 5) walking along."""
    _run_all(dev, el.edge_cases(*mn, kernel == "bf16mfma"))


@pytest.mark.parametrize("kernel", ["f32mfma", "bf16mfma"])
def test_gemm_splitk_exact(dev, kernel):
    """Chunk boundaries: fp32 K = 256 (4 full chunks), 257 (last chunk 1 wide), 400 (last 16 wide,
    LeNet fc1) and several tiles; bf16 K = 128, 130 (96 + 34), 272 (the last chunk is empty and
    must contribute zeros) and several tiles.  Every layout, the epilogue in the reduce."""
    cases = el.split_cases(kernel == "bf16mfma")
    assert all(el.case_plan(c)[0] > 1 for c in cases)
    _run_all(dev, cases)


def test_gemm_every_dtype_instantiation_exact(dev):
    """The 8 instantiations of the fp32 kernel and the 4 of the bf16 kernel, each at an edge
    shape and through split-K, writing C alone and C with C32; lowp with an fp32 B that needs
    rounding to bf16 (ties included), which also puts the bf16 output rounding to work."""
    _run_all(dev, el.dtype_cases())


def test_gemm_epilogue_exact(dev):
    """bias x relu; beta in {0, 0.5, 1} reading an fp32 C32 or a bf16 C; C and C32 together;
    scm = N + 5 (the gaps keep their NaN fill); each also through the split-K reduce.  beta = 0
    runs on NaN-prefilled outputs: it must overwrite."""
    cases = el.epilogue_cases()
    assert any(c.beta == 0.0 and el.case_plan(c)[0] > 1 for c in cases)
    _run_all(dev, cases)


def test_gemm_masked_a_exact(dev):
    """Amask over {2, 0, -0.0, -1, NaN} with NaN / Inf in the masked-out entries of A: kept where
    Amask > 0 by selection, so the result is finite and exact.  Both kernels, dgrad and wgrad
    layouts, an edge shape and split-K."""
    _run_all(dev, el.mask_cases())


@pytest.mark.parametrize("which", ["A", "B"])
def test_gemm_element0_poison(dev, which):
    """Out-of-range staging loads read element 0 and are zeroed by a select: with A[0] (B[0]) =
    NaN, row (column) 0 of C is NaN and every other element is exact."""
    for case in el.poison_cases():
        run_gemm(dev, case, poison=which)


@pytest.mark.parametrize("shape", el.TIERB_SHAPES, ids=lambda s: "%dx%dx%d%s" % (s[0], s[1], s[2], "_lowp" if s[3] else ""))
def test_gemm_tierb_bounded(dev, shape):
    """Gaussian operands: |C - ref| <= (K + 4) * 2^-23 * sum_k |a||b| + ulp_out(ref) / 2, per element,
    for an fp32 C32 and (lowp) a bf16 C written by the same call."""
    M, N, K, lowp = shape
    c, b = el.tierb_case(*shape), Bench(dev)
    A, B = b.inp(c.A, what="A"), b.inp(c.B, what="B")
    C = b.out((M, N), BF, "C") if lowp else None
    C32 = b.out((M, N), F32, "C32")
    lib().gemm(A, None, B, C, C32, None, M, N, K, K, 1, 1, K, N, 1.0, 0.0, False, lowp=lowp)
    for t in (C, C32):
        if t is not None:
            worst = el.assert_within(t, c.ref, c.bound + el.half_ulp(c.ref, t.dtype), f"tier B {shape} {t.dtype}")
            print(f"tier B {shape} {t.dtype}: worst |C - ref| / bound = {worst:.4f}")
    b.done()


# ------------------------------------------------------------------ colsum / bias_act
@pytest.mark.parametrize("M", el.COLSUM_M)
def test_colsum_exact(dev, M):
    """fp32 and bf16, with and without the mask (NaN / Inf behind it), beta in {0, 0.5, 1}; beta = 0
    on a NaN-prefilled out must overwrite."""
    for N in el.COLSUM_N:
        c, b = el.colsum_case(M, N), Bench(dev)
        for dt in (F32, BF):
            a, am, mk = b.inp(c.a, dt, "A"), b.inp(c.a_masked, dt, "A"), b.inp(c.maskv, dt, "Amask")
            for masked in (False, True):
                for beta in el.BETAS:
                    out = b.out((N,), F32, "out", prior=c.prior if beta else None)
                    lib().colsum(am if masked else a, mk if masked else None, out, beta)
                    _exact(out, el.ref_colsum(c, masked, beta), f"colsum {M}x{N} {dt} mask={masked} beta={beta}")
                    b.done()


@pytest.mark.parametrize("M", el.BIAS_ACT_M)
def test_bias_act_exact(dev, M):
    for N in el.COLSUM_N:
        c, b = el.bias_act_case(M, N), Bench(dev)
        y, bias = b.inp(c.y, what="y"), b.inp(c.bias, what="bias")
        for use_bias in (False, True):
            for relu in (False, True):
                for dt in (F32, BF):
                    out = b.out((M, N), dt, "out")
                    lib().bias_act(y, bias if use_bias else None, out, relu)
                    _exact(out, el.round_to(el.ref_bias_act(c, use_bias, relu), dt),
                           f"bias_act {M}x{N} bias={use_bias} relu={relu} {dt}")
                    b.done()


# ------------------------------------------------------------------ thin conv
VARIANTS = [(dt, relu, bias) for dt in (F32, BF) for relu in (False, True) for bias in (False, True)]


@pytest.mark.parametrize("geom", el.CONV_GEOMS, ids=str)
def test_conv_small_fwd_exact(dev, geom):
    """y and the uint8 argmax code at every element: the first strict maximum of the pre-bias
    accumulators in (dy, dx) row-major order wins (integer accumulators tie in many windows)."""
    B, Cin, H, W, Cout, K, pad, pool = geom
    OH, OW, PH, PW = el.conv_dims(geom)
    c, b = el.conv_case(geom), Bench(dev)
    w, bias = b.inp(c.w, what="w"), b.inp(c.bias, what="bias")
    for dt, relu, use_bias in VARIANTS:
        r = el.conv_refs(geom, relu, use_bias)
        x = b.inp(c.x, dt, "x")
        y = b.out((B, Cout, PH, PW), dt, "y")
        mask = b.out((B, Cout, PH, PW), U8, "mask") if pool == 2 else None
        lib().conv_small_fwd(x, w, bias if use_bias else None, y, mask, pad, pool, relu)
        _exact(y, r.y, f"y {dt} relu={relu} bias={use_bias}")
        if pool == 2:
            _exact(mask, r.code, f"mask {dt} relu={relu} bias={use_bias}")
        b.done()


def _run_conv_bwd(dev, geom, bs, variants, betas=(0.0, 1.0), outs=((True, True), (False, True), (True, False))):
    B, Cin, H, W, Cout, K, pad, pool = geom
    c, b = el.conv_case(geom), Bench(dev)
    nwork = lib().conv_small_workspace(B, Cin, H, W, Cout, K, pad, bs)
    assert nwork == el.conv_workspace(geom, bs)
    w = b.inp(c.w, what="w")
    for dt, relu, use_bias in variants:
        r = el.conv_refs(geom, relu, use_bias)
        x, dp, yp = b.inp(c.x, dt, "x"), b.inp(c.dp, dt, "dp"), b.inp(r.y, dt, "yp")
        mask = b.inp(r.code, U8, "mask") if pool == 2 else None
        for beta in betas:
            for with_dx, with_db in outs:
                dx = b.out(c.x.shape, dt, "dx") if with_dx else None
                dw = b.out(c.w.shape, F32, "dw", prior=c.dw0 if beta else None)
                db = b.out((Cout,), F32, "db", prior=c.db0 if beta else None) if with_db else None
                work = b.out((nwork,), F32, "work")  # sized exactly: a write past it hits the guard
                lib().conv_small_bwd(x, w, dp, yp, mask, dx, dw, db, work, pad, pool, relu, beta, bs)
                what = f"{dt} relu={relu} bias={use_bias} beta={beta} bs={bs}"
                if with_dx:
                    _exact(dx, r.dx, f"dx {what}")
                _exact(dw, beta * c.dw0.double() + r.dw, f"dw {what}")
                if with_db:
                    _exact(db, beta * c.db0.double() + r.db, f"db {what}")
                b.done()


@pytest.mark.parametrize("geom", el.CONV_GEOMS, ids=str)
def test_conv_small_bwd_exact(dev, geom):
    """dx, dw and db from the reference's pooled output and codes; beta = 0 on NaN-prefilled dw /
    db (it must overwrite) and beta = 1 over integer prior contents; dx = None and db = None; the
    workspace sized exactly inside a guarded tensor.  Batch slices of B - 1 images (two slabs, the
    last partial for B = 3).  With an odd conv output under pool 2 the last row and column of the
    dense gradient are zero."""
    _run_conv_bwd(dev, geom, max(1, geom[0] - 1), VARIANTS)


@pytest.mark.parametrize("bs", el.CONV_BS)
def test_conv_small_bwd_batch_slices(dev, bs):
    """B = 5 with bs = 1 (five slabs), 2 (a partial last slice), 5 (one slice) and 8 (bs > B)."""
    _run_conv_bwd(dev, el.CONV_SLICE_GEOM, bs, [(F32, True, True), (BF, False, False)], outs=((True, True),))


# ------------------------------------------------------------------ the bindings' refusals
# Only refusals whose rejected argument is a valid device tensor (at least as large as what an
# unguarded kernel would have touched) or a scalar are exercised.  Not exercised, because the
# rejected tensor would be host memory or need a second device: every "same device" check (gemm:
# B, Amask, C, C32, bias; colsum: Amask, out; conv_small_fwd / conv_small_bwd: w, bias, y, mask,
# dp, yp, dx, dw, db, work).
def _gemm_args(dev, M=8, N=8, K=8, dt=F32):
    z = lambda *s, d=dt: torch.zeros(*s, device=dev, dtype=d)
    return dict(A=z(M, K), Amask=None, B=z(N, K), C=z(M, N), C32=None, bias=None, M=M, N=N, K=K, sam=K, sak=1,
                sbk=1, sbn=K, scm=N, alpha=1.0, beta=0.0, relu=False, lowp=False)


def test_gemm_guards(dev):
    L = lib()
    L.gemm(**_gemm_args(dev))  # the accepted call
    half = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float16)
    for name, shape in (("A", (8, 16)), ("B", (8, 16)), ("C", (8, 16))):  # twice the bytes an fp32 read needs
        with pytest.raises(RuntimeError, match=f"{name} must be fp32 or bf16"):
            L.gemm(**{**_gemm_args(dev), name: half(*shape).view(-1)})
    with pytest.raises(RuntimeError, match="C32 must be float32"):
        L.gemm(**{**_gemm_args(dev), "C": None, "C32": torch.zeros(8, 8, device=dev, dtype=F64)})
    with pytest.raises(RuntimeError, match="Amask must have A's dtype"):
        L.gemm(**{**_gemm_args(dev), "Amask": torch.ones(8, 16, device=dev, dtype=BF)})
    with pytest.raises(RuntimeError, match="Amask must have at least"):
        L.gemm(**{**_gemm_args(dev), "A": torch.zeros(8, 16, device=dev), "Amask": torch.ones(8, 8, device=dev)})
    for k, v, msg in (("K", 0, "K must be >= 1"), ("M", -1, "M and N"), ("N", -1, "M and N"),
                      ("sam", -8, "non-negative"), ("sak", -1, "non-negative"), ("sbk", -1, "non-negative"),
                      ("sbn", -8, "non-negative"), ("scm", -8, "non-negative")):
        with pytest.raises(RuntimeError, match=msg):
            L.gemm(**{**_gemm_args(dev), k: v})
    with pytest.raises(RuntimeError, match="gemm_plan"):
        L.gemm_plan(8, 8, 0, False, False)
    # M * N == 0 returns before any launch and leaves the outputs alone
    for k in ("M", "N"):
        C, chk = ec.guarded((8, 8), F32, dev, "out")
        L.gemm(**{**_gemm_args(dev), "C": C, k: 0})
        torch.cuda.synchronize()
        assert _all_ones_bits(C)
        chk("C")


def test_colsum_guards(dev):
    L = lib()
    A, out = torch.zeros(4, 8, device=dev), torch.zeros(8, device=dev)
    L.colsum(A, torch.ones(4, 8, device=dev), out, 0.0)
    with pytest.raises(RuntimeError, match="A must be fp32 or bf16"):
        L.colsum(torch.zeros(4, 8, device=dev, dtype=F64), None, out, 0.0)
    with pytest.raises(RuntimeError, match="Amask must have A's dtype"):
        L.colsum(A, torch.ones(4, 8, device=dev, dtype=F64), out, 0.0)
    with pytest.raises(RuntimeError, match="A's shape"):
        L.colsum(A, torch.ones(8, 8, device=dev), out, 0.0)
    with pytest.raises(RuntimeError, match="A's shape"):
        L.colsum(A, torch.ones(4, 16, device=dev)[:, ::2], out, 0.0)
    with pytest.raises(RuntimeError, match="out must be"):
        L.colsum(A, None, torch.zeros(16, device=dev), 0.0)
    with pytest.raises(RuntimeError, match="out must be"):
        L.colsum(A, None, torch.zeros(8, device=dev, dtype=F64), 0.0)


def _conv_args(dev, B=2, Cin=2, H=9, W=7, Cout=3, K=3, pad=0, pool=2, bs=2):
    OH, OW = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    PH, PW = OH // pool, OW // pool
    z = lambda *s, d=F32: torch.zeros(*s, device=dev, dtype=d)
    nwork = (B * Cout * OH * OW + 63) // 64 * 64 + -(-B // max(bs, 1)) * (Cout * Cin * K * K + Cout)
    fwd = dict(x=z(B, Cin, H, W), w=z(Cout, Cin, K, K), bias=z(Cout), y=z(B, Cout, PH, PW),
               mask=z(B, Cout, PH, PW, d=U8), pad=pad, pool=pool, relu=True)
    bwd = dict(x=fwd["x"], w=fwd["w"], dp=z(B, Cout, PH, PW), yp=z(B, Cout, PH, PW), mask=fwd["mask"],
               dx=z(B, Cin, H, W), dw=z(Cout, Cin, K, K), db=z(Cout), work=z(2 * nwork), pad=pad, pool=pool,
               relu=True, beta=0.0, bs=bs)
    return fwd, bwd


def test_conv_small_guards(dev):
    """Every refusal raises before any launch: the mask's dtype, size and contiguity, K, pool, pad,
    bs, the shapes of w / y / dp / yp / dx / dw / db / bias, the workspace."""
    L = lib()
    fwd, bwd = _conv_args(dev)
    call = {"fwd": lambda a: L.conv_small_fwd(*a.values()), "bwd": lambda a: L.conv_small_bwd(*a.values())}
    call["fwd"](fwd)  # the accepted calls
    call["bwd"](bwd)
    z = lambda *s, d=F32: torch.zeros(*s, device=dev, dtype=d)
    both = [("mask", z(2, 3, 3, 2, d=torch.int32), "uint8"), ("mask", z(2, 3, 3, 4, d=U8), "uint8"),
            ("mask", z(2, 3, 3, 4, d=U8)[..., ::2], "uint8"), ("mask", None, "mask required"),
            ("w", z(3, 2, 4, 4), "K in"), ("w", z(3, 2, 7, 7), "K in"), ("w", z(3, 4, 3, 3), "x's Cin"),
            ("w", z(3, 2, 3, 5), "x's Cin"), ("w", z(3, 2, 3, 3, d=F64), "float32"),
            ("pool", 3, "pool must be"), ("pool", 0, "pool must be"), ("pad", -1, "pad must be")]
    only = {"fwd": [("y", z(2, 3, 4, 2), "y shape"), ("y", z(2, 4, 3, 2), "y shape"), ("y", z(2, 3, 3, 2, d=BF), "dtype"),
                    ("bias", z(4), "bias must be"), ("bias", z(3, d=F64), "bias must be")],
            "bwd": [("bs", 0, "bs must be"), ("bs", -1, "bs must be"),
                    ("dp", z(2, 3, 4, 2), "dp shape"), ("yp", z(2, 3, 3, 3), "yp shape"), ("dp", z(2, 3, 3, 2, d=BF), "dp must have"),
                    ("dx", z(2, 2, 9, 8), "dx shape"), ("dx", z(2, 2, 9, 7, d=BF), "dx must have"),
                    ("dw", z(3, 2, 3, 4), "dw shape"), ("dw", z(3, 2, 3, 3, d=F64), "float32"),
                    ("db", z(4), "db must be"), ("db", z(6)[::2], "db must be"),
                    ("work", z(8), "workspace too small"), ("work", z(4096, d=F64), "float32")]}
    for which, base in (("fwd", fwd), ("bwd", bwd)):
        for key, bad, msg in both + only[which]:
            with pytest.raises(RuntimeError, match=msg):
                call[which]({**base, key: bad})
    with pytest.raises(RuntimeError, match="too small for K"):
        f2, _ = _conv_args(dev, H=3, W=7, K=3)  # conv output 1 x 5 under pool 2
        f2["y"], f2["mask"] = z(2, 3, 1, 2), z(2, 3, 1, 2, d=U8)
        call["fwd"](f2)
    with pytest.raises(RuntimeError, match="bs must be"):
        L.conv_small_workspace(2, 2, 9, 7, 3, 3, 0, 0)


def test_conv_small_bwd_refuses_an_image_its_lds_cannot_hold(dev):
    """Backward-data stages Cout * (OH + 2K - 2) * (OW + 2K - 2) floats of one image in LDS: at
    64 x 64 with Cout = 16, K = 5 that is 333 KB.  The binding refuses (naming the image size)
    instead of a launch that fails and leaves dx unwritten; without dx the same call runs."""
    _, bwd = _conv_args(dev, B=1, Cin=1, H=64, W=64, Cout=16, K=5, pad=2, pool=2, bs=1)
    with pytest.raises(RuntimeError, match="64 x 64.*bytes of LDS"):
        lib().conv_small_bwd(*bwd.values())
    lib().conv_small_bwd(*{**bwd, "dx": None}.values())
    torch.cuda.synchronize()
