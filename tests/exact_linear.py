"""Element-exact references for the Linear GEMM family (csrc/gemm.hip) and the thin-conv family
(csrc/conv_small.hip).

Tier A: every operand is a small integer held in fp32 (A in [-2, 2], B with at most 48 entries
of +-1 along k per output column, bias and prior contents in [-4, 4]), so |sum| <= 96, every
partial sum is an exact fp32 number in any order (MFMA order, split-K chunks, the ordered
reduce, the thin conv's tap order, batch slices) and alpha * sum + beta * C + bias is exact in
fp32 for alpha in {1, 2, 0.125}, beta in {0, 1, 0.5}.  The float64 references below are built
from the strided definitions and explicit tap loops (never a library matmul / convolution on
the operands); a bf16 output is the float64 value rounded once with torch's RNE.
exact_preconditions / conv_preconditions assert, per case, the conditions under which this
holds.  Tier B: Gaussian operands and a per-element bound derived from the formats.

This module never calls the code under test.  guarded / assert_exact / the limits come from
tests/exact_conv.py."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import torch

from exact_bn_pool import assert_within, ulp  # noqa: F401  (re-exported)
from exact_conv import LIM_BF16, LIM_FP32, assert_exact, guarded  # noqa: F401  (re-exported)

F32, BF, F64, U8 = torch.float32, torch.bfloat16, torch.float64, torch.uint8
DT = {"f": F32, "b": BF}
NAN, INF = float("nan"), float("inf")
MASK_VALUES = [2.0, 0.0, -0.0, -1.0, NAN]  # kept where > 0: only the 2 keeps
B_FRACTIONS = [2.0 ** -8, 3 * 2.0 ** -9, 3 * 2.0 ** -8]  # tie to even (down), above the tie, tie (up)
NZ_PER_COLUMN = 48

# ------------------------------------------------------------------ GEMM: the cases
# la: "k" = A stored [M, K] (sak == 1), "m" = A stored [K, M] (sam == 1)
# lb: "k" = B stored [N, K] (sbk == 1), "n" = B stored [K, N] (sbn == 1)
# out: "C" (dtype tc), "C32" (fp32 only) or "both"; beta reads C32 when there is one, else C
# pad: scm = N + pad; mask: Amask given; bfrac: lowp with an fp32 B that is not bf16-representable
_FIELDS = "M N K la lb ta tb tc lowp alpha beta bias relu out pad mask bfrac seed"
_DEFAULTS = ("k", "k", "f", "f", "f", False, 1.0, 0.0, False, False, "C", 0, False, False, 0)
GemmCase = namedtuple("GemmCase", _FIELDS, defaults=_DEFAULTS)
FWD, DGRAD, WGRAD, FOURTH = ("k", "k"), ("k", "n"), ("m", "n"), ("m", "k")  # the callers' three + one
LAYOUTS = [FWD, DGRAD, WGRAD, FOURTH]

MN_EDGE = [(1, 1), (63, 65), (64, 64), (65, 63), (130, 70)]
K_NOSPLIT = [1, 3, 31, 32, 33, 63, 64, 65, 129]
# fp32 split-K: one output tile, K = 256 / 257 / 400; LeNet fc1 itself; several tiles
SPLIT_F32 = [(64, 64, 256), (63, 61, 257), (64, 64, 400), (32, 120, 400), (130, 70, 300)]
# bf16 split-K: S = 2; chunks 96 + 34; S = 4 with an empty last chunk; several tiles
SPLIT_BF16 = [(64, 64, 128), (63, 65, 130), (64, 64, 272), (130, 70, 272)]
# the 8 instantiations of the fp32 kernel and the 4 of the bf16 kernel: (ta, tb, tc, lowp)
DTYPES_F32 = [(a, b, c, False) for a in "fb" for b in "fb" for c in "fb"]
DTYPES_BF16 = [("b", b, c, True) for b in "fb" for c in "fb"]
ALPHAS, BETAS = [1.0, 2.0, 0.125], [0.0, 1.0, 0.5]

# (M, N, K, a_bf16, lowp) -> (S, kchunk, chunks): what gemm() must decide for the named shapes.
# chunks is the number of k-blocks launched; the bf16 kernel launches all S (the last may be empty).
EXPECTED_PLANS = {
    (64, 64, 256, 0, 0): (8, 64, 4),
    (63, 61, 257, 0, 0): (8, 64, 5),
    (64, 64, 400, 0, 0): (8, 64, 7),
    (32, 120, 400, 0, 0): (8, 64, 7),  # LeNet fc1: 7 chunks, the last 16 wide
    (130, 70, 300, 0, 0): (8, 64, 5),
    (130, 70, 300, 1, 0): (8, 64, 5),  # bf16 A without lowp stays on the fp32 kernel
    (130, 70, 129, 0, 0): (1, 129, 1),
    (65, 63, 255, 0, 0): (1, 255, 1),  # below 4 stages: no split
    (64, 64, 128, 1, 1): (2, 64, 2),
    (63, 65, 130, 1, 1): (2, 96, 2),  # 96 + 34
    (64, 64, 272, 1, 1): (4, 96, 4),  # 96 + 96 + 80 + an empty chunk
    (130, 70, 272, 1, 1): (4, 96, 4),
    (130, 70, 129, 1, 1): (2, 96, 2),  # K = 129 already splits on the bf16 kernel
    (65, 63, 65, 1, 1): (1, 65, 1),
    (64, 64, 127, 1, 1): (1, 127, 1),
    (256, 1000, 512, 1, 1): (4, 128, 4),  # the ResNet head
}


def plan_mirror(M, N, K, a_bf16, lowp):
    """The split-K heuristic of csrc/gemm.hip, restated (tests compare it with EXPECTED_PLANS and
    with the gemm_plan binding)."""
    tiles = -(-M // 64) * -(-N // 64)
    S = 1
    if lowp and a_bf16:
        while S < 16 and tiles * S < 256 and K // (S * 2) >= 64:
            S *= 2
        return (1, K, 1) if S == 1 else (S, (-(-K // S) + 31) // 32 * 32, S)
    if K >= 256:
        while S < 16 and tiles * S < 256 and K // (S * 2) >= 32:
            S *= 2
    if S == 1:
        return (1, K, 1)
    kchunk = (-(-K // S) + 63) // 64 * 64
    return (S, kchunk, -(-K // kchunk))


def uses_bf16_kernel(case):
    return bool(case.lowp and case.ta == "b")


def case_plan(case):
    return plan_mirror(case.M, case.N, case.K, int(case.ta == "b"), int(case.lowp))


def _cycle(i, seq):
    return seq[i % len(seq)]


def _epilogue(i):
    """A deterministic walk over alpha x beta x bias x relu x output, one per case index."""
    return dict(alpha=_cycle(i, ALPHAS), beta=_cycle(i // 3, BETAS), bias=bool(i & 1), relu=bool((i >> 1) & 1),
                out=_cycle(i // 2, ["C", "C32", "both"]), pad=_cycle(i // 5, [0, 5]))


def edge_cases(M, N, bf16_kernel):
    """Every K without split x all four layouts at one (M, N), epilogue walking with the index."""
    dt = dict(ta="b", tb="b", tc="b", lowp=True) if bf16_kernel else {}
    return [GemmCase(M, N, K, la, lb, **dt, **_epilogue(i * 4 + j))
            for i, K in enumerate(K_NOSPLIT) for j, (la, lb) in enumerate(LAYOUTS)]


def split_cases(bf16_kernel):
    dt = dict(ta="b", tb="b", tc="b", lowp=True) if bf16_kernel else {}
    shapes = SPLIT_BF16 if bf16_kernel else SPLIT_F32
    return [GemmCase(M, N, K, la, lb, **dt, **_epilogue(i * 4 + j + 1))
            for i, (M, N, K) in enumerate(shapes) for j, (la, lb) in enumerate(LAYOUTS)]


def dtype_cases():
    """Each instantiation at an edge shape and through split-K, outputs "C" and "both"; the lowp
    ones with an fp32 B also with a B that needs rounding."""
    out = []
    for i, (ta, tb, tc, lowp) in enumerate(DTYPES_F32 + DTYPES_BF16):
        shapes = [(65, 63, 33), (130, 70, 272) if lowp else (130, 70, 300)]
        for j, (M, N, K) in enumerate(shapes):
            la, lb = _cycle(i + j, LAYOUTS[:3])
            for o in ("C", "both"):
                e = dict(_epilogue(i + 3 * j), out=o)
                out.append(GemmCase(M, N, K, la, lb, ta, tb, tc, lowp, **e))
                if lowp and tb == "f":
                    out.append(GemmCase(M, N, K, la, lb, ta, tb, tc, lowp, bfrac=True, **e))
    return out


def epilogue_cases():
    """bias x relu; beta in {0, 0.5, 1} reading an fp32 C32 and reading a bf16 C; C and C32
    together; scm = N + 5: each without split and through the split-K reduce, on both kernels."""
    out = []
    for kern, shapes in ((False, [(65, 63, 65), (63, 61, 257)]), (True, [(65, 63, 65), (63, 65, 130)])):
        ta = tb = "b" if kern else "f"
        for M, N, K in shapes:
            base = dict(M=M, N=N, K=K, ta=ta, tb=tb, lowp=kern)
            for bias in (False, True):
                for relu in (False, True):
                    out.append(GemmCase(**base, tc="f", bias=bias, relu=relu, alpha=2.0))
            for beta in BETAS:
                for pad in (0, 5):
                    out.append(GemmCase(**base, tc="f", out="C32", beta=beta, pad=pad, bias=True))
                    out.append(GemmCase(**base, tc="b", out="C", beta=beta, pad=pad, alpha=0.125))
                    out.append(GemmCase(**base, tc="b", out="both", beta=beta, pad=pad, relu=True))
    return out


def mask_cases():
    """Masked A on both kernels in the dgrad and wgrad layouts, at an edge shape and through
    split-K (the masked-out entries of A hold NaN and Inf)."""
    out = []
    for kern, shapes in ((False, [(65, 63, 33), (130, 70, 300)]), (True, [(65, 63, 33), (130, 70, 272)])):
        t = "b" if kern else "f"
        for M, N, K in shapes:
            for la, lb in (DGRAD, WGRAD):
                for beta in (0.0, 1.0):
                    out.append(GemmCase(M, N, K, la, lb, t, "f", "f", kern, mask=True, beta=beta,
                                        out="C32" if beta else "C"))
    return out


def poison_cases():
    """K no multiple of the k stage, partial tiles, and split-K with a partial last chunk: every
    staging loop has out-of-range elements, which read element 0."""
    out = []
    for kern, shapes in ((False, [(63, 65, 33), (63, 61, 257)]), (True, [(63, 65, 33), (63, 65, 130)])):
        t = "b" if kern else "f"
        for M, N, K in shapes:
            for la, lb in LAYOUTS[:3]:
                out.append(GemmCase(M, N, K, la, lb, t, t, "f", kern))
    return out


def all_gemm_cases():
    cases = dtype_cases() + epilogue_cases() + mask_cases() + poison_cases()
    for kern in (False, True):
        cases += split_cases(kern)
        for M, N in MN_EDGE:
            cases += edge_cases(M, N, kern)
    return cases


def gemm_id(c):
    return (f"{c.M}x{c.N}x{c.K}_{c.la}{c.lb}_{c.ta}{c.tb}{c.tc}{'_lowp' if c.lowp else ''}"
            f"_a{c.alpha}_b{c.beta}{'_bias' if c.bias else ''}{'_relu' if c.relu else ''}_{c.out}"
            f"{'_pad' if c.pad else ''}{'_mask' if c.mask else ''}{'_bfrac' if c.bfrac else ''}")


# ------------------------------------------------------------------ GEMM: operands
def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _choice(g, values, shape):
    v = torch.tensor(values, dtype=F32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def sparse_b(g, K, N):
    """[K, N] with exactly min(K, 48) entries of +-1 along k in every column, zeros elsewhere."""
    nz = min(K, NZ_PER_COLUMN)
    pos = torch.rand(N, K, generator=g).argsort(1)[:, :nz]
    b = torch.zeros(N, K)
    b.scatter_(1, pos, _choice(g, [-1.0, 1.0], (N, nz)))
    return b.t().contiguous()


@functools.lru_cache(maxsize=None)
def gemm_draw(M, N, K, seed=0):
    """The logical operands of one shape (shared: do not modify)."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * M + 17 * N + K)
    d = SimpleNamespace()
    d.a = _randint(g, -2, 2, (M, K))
    d.b = sparse_b(g, K, N)
    d.bias = _randint(g, -4, 4, (N,))
    d.prior = _randint(g, -4, 4, (M, N))
    d.maskv = _choice(g, MASK_VALUES, (M, K))
    d.junk = _choice(g, [NAN, INF, -INF], (M, K))
    d.frac = _choice(g, B_FRACTIONS, (K, N))
    return d


def strides_of(case):
    M, N, K = case.M, case.N, case.K
    sam, sak = (K, 1) if case.la == "k" else (1, M)
    sbk, sbn = (1, K) if case.lb == "k" else (N, 1)
    return sam, sak, sbk, sbn, N + case.pad


@functools.lru_cache(maxsize=None)
def gemm_operands(case):
    """The operands as the kernel gets them: storage order and dtype applied (CPU tensors)."""
    d = gemm_draw(case.M, case.N, case.K, case.seed)
    o = SimpleNamespace(bias=d.bias if case.bias else None, prior=d.prior)
    a = d.a
    if case.mask:
        a = torch.where(d.maskv > 0, d.a, d.junk)
    b = d.b * (1 + d.frac) if case.bfrac else d.b
    store = lambda t, rowmajor: (t if rowmajor else t.t()).contiguous()
    o.A = store(a, case.la == "k").to(DT[case.ta])
    o.Amask = store(d.maskv, case.la == "k").to(DT[case.ta]) if case.mask else None
    o.B = store(b, case.lb == "n").to(DT[case.tb])
    o.prior_dtype = F32 if case.out in ("C32", "both") else DT[case.tc]
    return o


def strided(flat, rows, cols, sr, sc):
    """The [rows, cols] matrix t(r, c) = flat[r * sr + c * sc]."""
    idx = torch.arange(rows).view(-1, 1) * sr + torch.arange(cols).view(1, -1) * sc
    return flat[idx]


def gemm_terms(case, A=None, B=None):
    """a(m, k) after the mask selection and b(k, n) after the lowp rounding, float64."""
    o = gemm_operands(case)
    sam, sak, sbk, sbn, _ = strides_of(case)
    A = o.A if A is None else A
    B = o.B if B is None else B
    a = strided(A.double().flatten(), case.M, case.K, sam, sak)
    if case.mask:
        keep = strided(o.Amask.double().flatten(), case.M, case.K, sam, sak) > 0
        a = torch.where(keep, a, torch.zeros_like(a))  # by selection: NaN / Inf do not leak
    if uses_bf16_kernel(case) and B.dtype == F32:
        B = B.bfloat16()  # rounded to bf16 while it is staged
    b = strided(B.double().flatten(), case.K, case.N, sbk, sbn)
    return a, b


def gemm_epilogue(case, acc):
    """alpha * acc + beta * C + bias, ReLU: float64, before the output rounding."""
    o = gemm_operands(case)
    v = case.alpha * acc
    if case.beta != 0.0:
        v = v + case.beta * o.prior.to(o.prior_dtype).double()
    if case.bias:
        v = v + o.bias.double()
    return torch.relu(v) if case.relu else v


def round_to(v, dtype):
    """One RNE rounding of float64 values that are exact fp32 numbers."""
    return v.float().to(dtype).double()


@functools.lru_cache(maxsize=None)
def gemm_ref(case):
    """The float64 reference before the output rounding (shared: do not modify)."""
    a, b = gemm_terms(case)
    return gemm_epilogue(case, torch.einsum("mk,kn->mn", a, b))


@functools.lru_cache(maxsize=None)
def gemm_ref_poisoned(case, which):
    """gemm_ref with storage element 0 of A (or B) set to NaN: row (column) 0 is NaN, and nothing
    else is, because an out-of-range staging load of element 0 is discarded by selection."""
    o = gemm_operands(case)
    A, B = o.A.clone(), o.B.clone()
    (A if which == "A" else B).view(-1)[0] = NAN
    a, b = gemm_terms(case, A=A, B=B)
    ref = gemm_epilogue(case, torch.einsum("mk,kn->mn", a, b))
    bad = torch.isnan(ref)
    assert bad[0].all() if which == "A" else bad[:, 0].all()
    assert int(bad.sum()) == (case.N if which == "A" else case.M)
    return ref


def exact_preconditions(case):
    """The conditions under which the kernel's result is independent of its accumulation order
    and equal to gemm_ref (rounded once where the output is bf16).  Returns the maxima found."""
    o = gemm_operands(case)
    d = gemm_draw(case.M, case.N, case.K, case.seed)
    a, b = gemm_terms(case)
    assert torch.isfinite(a).all() and torch.isfinite(b).all(), "operands after selection are finite"
    assert torch.equal(a, a.round()) and float(a.abs().max()) <= 2, "A: integers in [-2, 2]"
    if not case.mask:  # stored as drawn: the storage dtype holds the integers exactly
        assert torch.equal(o.A.double().flatten().sort().values, d.a.double().flatten().sort().values)
    nz = int((b != 0).sum(0).max())
    assert nz <= NZ_PER_COLUMN, f"B: {nz} non-zeros in a column"
    gran = 2.0 ** -7 if case.bfrac else 1.0  # the products are multiples of gran
    if case.bfrac:
        raw = strided(o.B.double().flatten(), case.K, case.N, *strides_of(case)[2:4])
        assert (raw[raw != 0] != raw[raw != 0].float().bfloat16().double()).all(), "B needs rounding"
        assert set(b.abs().unique().tolist()) <= {0.0, 1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6}
    else:
        assert set(b.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert torch.equal(b / gran, (b / gran).round())  # integer a: every product is a multiple of gran
    abs_sum = torch.einsum("mk,kn->mn", a.abs(), b.abs())
    seen = {"abs_sum": float(abs_sum.max())}
    assert seen["abs_sum"] <= 2 * NZ_PER_COLUMN * (1 + 2.0 ** -6), "|sum| <= 96 (x the rounded fraction)"
    assert seen["abs_sum"] / gran < LIM_FP32, "every partial sum is exact in fp32"
    acc = torch.einsum("mk,kn->mn", a, b)
    stages = [acc, case.alpha * acc, gemm_ref(case)]
    if case.beta != 0.0:
        stages.append(case.alpha * acc + case.beta * o.prior.double())
    for s in stages:  # every intermediate of the epilogue is an fp32 number: no rounding before the last
        assert torch.equal(s.float().double(), s), "epilogue intermediate not exact in fp32"
    assert case.alpha in ALPHAS and case.beta in BETAS
    assert float(o.prior.abs().max()) <= 4 and torch.equal(o.prior.to(o.prior_dtype).float(), o.prior)
    ref = gemm_ref(case)
    seen["out"] = float(ref.abs().max())
    if case.tc == "b" and case.out != "C32" and case.alpha >= 1 and not case.bfrac:
        assert seen["out"] <= LIM_BF16, "bf16 output magnitude"
        if case.beta != 0.5:
            assert torch.equal(round_to(ref, BF), ref), "integers up to 256 are bf16 numbers"
    return seen


# ------------------------------------------------------------------ GEMM: tier B
TIERB_SHAPES = [(65, 63, 129, False), (32, 120, 400, False), (130, 70, 300, False),
                (65, 63, 129, True), (64, 64, 272, True), (130, 70, 512, True)]
ULP32 = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def tierb_case(M, N, K, lowp):
    """Gaussian operands in the forward layout (bf16 for lowp), the float64 reference and the
    bound (K + 4) * ulp32 * sum_k |a||b| (one ulp per accumulate covers round-to-nearest and
    truncation in any order); the caller adds half an ulp of the output type."""
    g = torch.Generator().manual_seed(101 * M + 7 * N + K + int(lowp))
    dt = BF if lowp else F32
    c = SimpleNamespace(M=M, N=N, K=K, lowp=lowp)
    c.A = torch.randn(M, K, generator=g).to(dt)
    c.B = torch.randn(N, K, generator=g).to(dt)  # stored [N, K]: sbk = 1, sbn = K
    a, b = c.A.double(), c.B.double().t()
    c.ref = torch.einsum("mk,kn->mn", a, b)
    c.bound = (K + 4) * ULP32 * torch.einsum("mk,kn->mn", a.abs(), b.abs())
    return c


def half_ulp(ref, dtype):
    return ulp(ref, 8 if dtype == BF else 24) / 2


# ------------------------------------------------------------------ colsum / bias_act
COLSUM_M, COLSUM_N = [1, 3, 4, 5, 257], [1, 63, 64, 65, 130]
BIAS_ACT_M = [1, 5]


@functools.lru_cache(maxsize=None)
def colsum_case(M, N):
    g = torch.Generator().manual_seed(1009 * M + N)
    c = SimpleNamespace(M=M, N=N)
    c.a = _randint(g, -2, 2, (M, N))
    c.maskv = _choice(g, MASK_VALUES, (M, N))
    c.a_masked = torch.where(c.maskv > 0, c.a, _choice(g, [NAN, INF, -INF], (M, N)))
    c.prior = _randint(g, -4, 4, (N,))
    return c


def ref_colsum(c, masked, beta):
    """out[n] = beta * prior[n] + sum_m (A(m, n) where mask(m, n) > 0), float64."""
    a = c.a.double()
    if masked:
        a = torch.where(c.maskv > 0, c.a_masked.double(), torch.zeros_like(a))
    s = torch.zeros(c.N, dtype=F64)
    for m in range(c.M):
        s += a[m]
    return s if beta == 0.0 else beta * c.prior.double() + s


def colsum_preconditions(c):
    assert float(c.a.abs().sum(0).max()) + 4 < LIM_FP32
    for masked in (False, True):
        for beta in BETAS:
            r = ref_colsum(c, masked, beta)
            assert torch.isfinite(r).all() and torch.equal(r.float().double(), r)
    return float(c.a.abs().sum(0).max())


@functools.lru_cache(maxsize=None)
def bias_act_case(M, N):
    """y in eighths up to 256: y + bias is exact in fp32 and needs rounding (ties included) in bf16."""
    g = torch.Generator().manual_seed(2003 * M + N)
    c = SimpleNamespace(M=M, N=N)
    c.y = _randint(g, -2048, 2048, (M, N)) / 8
    c.bias = _randint(g, -4, 4, (N,))
    return c


def ref_bias_act(c, bias, relu):
    v = c.y.double() + (c.bias.double() if bias else 0.0)
    return torch.relu(v) if relu else v


# ------------------------------------------------------------------ thin conv
# (B, Cin, H, W, Cout, K, pad, pool)
CONV_GEOMS = [
    (2, 1, 28, 28, 6, 5, 2, 2),   # LeNet conv1: 196 pooled pixels, 784 input pixels (4 x-blocks in backward-data)
    (2, 6, 14, 14, 16, 5, 0, 2),  # LeNet conv2
    (3, 2, 13, 9, 3, 3, 0, 2),    # conv output 11 x 7 under pool 2: the last row and column are unpooled
    (2, 3, 7, 5, 4, 3, 1, 1),
    (1, 1, 28, 28, 2, 5, 2, 1),   # 784 outputs: 4 forward x-blocks
]
CONV_SLICE_GEOM = (5, 2, 13, 9, 3, 3, 0, 2)  # B = 5 for the batch-slice sizes
CONV_BS = [1, 2, 5, 8]  # single images, a partial last slice, one slice, bs > B


def conv_dims(geom):
    B, Cin, H, W, Cout, K, pad, pool = geom
    OH, OW = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    return OH, OW, OH // pool, OW // pool


def conv_workspace(geom, bs):
    """The documented workspace size in floats: dyc rounded up to 64, then S slabs."""
    B, Cin, H, W, Cout, K, pad, pool = geom
    OH, OW, _, _ = conv_dims(geom)
    total = B * Cout * OH * OW
    return (total + 63) // 64 * 64 + -(-B // bs) * (Cout * Cin * K * K + Cout)


@functools.lru_cache(maxsize=None)
def conv_case(geom, seed=0):
    """Integer operands of one thin-conv geometry, NCHW (shared: do not modify)."""
    B, Cin, H, W, Cout, K, pad, pool = geom
    OH, OW, PH, PW = conv_dims(geom)
    g = torch.Generator().manual_seed(4001 * seed + 13 * H + 7 * W + Cout)
    c = SimpleNamespace(geom=geom, seed=seed)
    c.x = _randint(g, -2, 2, (B, Cin, H, W))
    c.w = sparse_b(g, Cin * K * K, Cout).t().contiguous().view(Cout, Cin, K, K)
    c.bias = _randint(g, -4, 4, (Cout,))
    c.dp = _randint(g, -2, 2, (B, Cout, PH, PW))
    c.dw0 = _randint(g, -4, 4, (Cout, Cin, K, K))
    c.db0 = _randint(g, -4, 4, (Cout,))
    return c


def _pad_nchw(x, p):
    return torch.nn.functional.pad(x, (p, p, p, p))


def ref_conv_acc(x, w, pad):
    """acc[b, co, oh, ow] = sum_{ci, kh, kw} x[b, ci, oh - pad + kh, ow - pad + kw] * w[co, ci, kh, kw]."""
    Cout, Cin, K, _ = w.shape
    xp, wd = _pad_nchw(x.double(), pad), w.double()
    OH, OW = xp.shape[2] - K + 1, xp.shape[3] - K + 1
    acc = torch.zeros(x.shape[0], Cout, OH, OW, dtype=F64)
    for kh in range(K):
        for kw in range(K):
            for ci in range(Cin):
                acc += xp[:, ci:ci + 1, kh:kh + OH, kw:kw + OW] * wd[:, ci, kh, kw].view(1, Cout, 1, 1)
    return acc


def ref_pool_first_max(acc, pool):
    """Over the 2 x 2 window in (dy, dx) row-major order the first strict maximum wins; the code
    is its position 0..3.  Returns (best, code, ties): ties marks windows whose maximum occurs
    more than once.  pool == 1: the accumulators themselves, code 0."""
    if pool == 1:
        z = torch.zeros(acc.shape, dtype=torch.bool)
        return acc, z.to(U8), z
    PH, PW = acc.shape[2] // 2, acc.shape[3] // 2
    win = [acc[:, :, dy:2 * PH:2, dx:2 * PW:2] for dy in (0, 1) for dx in (0, 1)]
    best, code = win[0].clone(), torch.zeros(win[0].shape, dtype=U8)
    for i in (1, 2, 3):
        better = win[i] > best
        best = torch.where(better, win[i], best)
        code = torch.where(better, torch.full_like(code, i), code)
    ties = sum((w_ == best).long() for w_ in win) > 1
    return best, code, ties


def ref_conv_fwd(x, w, bias, pad, pool, relu):
    """(y, code, ties): the pooled maximum of the pre-bias accumulators + bias, ReLU."""
    best, code, ties = ref_pool_first_max(ref_conv_acc(x, w, pad), pool)
    y = best if bias is None else best + bias.double().view(1, -1, 1, 1)
    return (torch.relu(y) if relu else y), code, ties


def ref_unpool(dp, yp, code, OH, OW, pool, relu):
    """The dense conv-output gradient: dp at the window's coded position where the pooled output
    is live (yp > 0 under ReLU); zero elsewhere, the unpooled last row / column included."""
    g = dp.double()
    if relu:
        g = torch.where(yp.double() > 0, g, torch.zeros_like(g))
    if pool == 1:
        return g
    B, C, PH, PW = g.shape
    dyc = torch.zeros(B, C, OH, OW, dtype=F64)
    for i, (dy, dx) in enumerate((a, b) for a in (0, 1) for b in (0, 1)):
        dyc[:, :, dy:2 * PH:2, dx:2 * PW:2] = torch.where(code == i, g, torch.zeros_like(g))
    return dyc


def ref_conv_bwd(x, w, dyc, pad, absolute=False):
    """(dx, dw, db) of the dense gradient by tap loops; absolute: sums of |terms| instead."""
    Cout, Cin, K, _ = w.shape
    xd, wd, d = x.double(), w.double(), dyc
    if absolute:
        xd, wd, d = xd.abs(), wd.abs(), d.abs()
    B, _, H, W = x.shape
    OH, OW = d.shape[2:]
    xp = _pad_nchw(xd, pad)
    dxp = torch.zeros_like(xp)
    dw = torch.zeros(Cout, Cin, K, K, dtype=F64)
    for kh in range(K):
        for kw in range(K):
            for ci in range(Cin):
                xs = xp[:, ci:ci + 1, kh:kh + OH, kw:kw + OW]
                dw[:, ci, kh, kw] = (d * xs).sum((0, 2, 3))
                dxp[:, ci, kh:kh + OH, kw:kw + OW] += (d * wd[:, ci, kh, kw].view(1, Cout, 1, 1)).sum(1)
    return dxp[:, :, pad:pad + H, pad:pad + W].contiguous(), dw, d.sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def conv_refs(geom, relu, bias, seed=0):
    """Every float64 reference of one (geometry, relu, bias): computed once, shared."""
    B, Cin, H, W, Cout, K, pad, pool = geom
    OH, OW, PH, PW = conv_dims(geom)
    c = conv_case(geom, seed)
    r = SimpleNamespace()
    r.y, r.code, r.ties = ref_conv_fwd(c.x, c.w, c.bias if bias else None, pad, pool, relu)
    r.dyc = ref_unpool(c.dp, r.y, r.code, OH, OW, pool, relu)
    r.dx, r.dw, r.db = ref_conv_bwd(c.x, c.w, r.dyc, pad)
    return r


def conv_preconditions(geom, relu, bias, seed=0):
    """y and dx are integers of magnitude <= 256 (exact in bf16), every sum of |terms| stays
    below 2^24 (exact in fp32 in any order, any batch slicing), dw0 + dw likewise."""
    B, Cin, H, W, Cout, K, pad, pool = geom
    c, r = conv_case(geom, seed), conv_refs(geom, relu, bias, seed)
    assert int((c.w != 0).flatten(1).sum(1).max()) <= NZ_PER_COLUMN
    seen = {}
    for n in ("y", "dx"):
        v = getattr(r, n)
        assert torch.equal(v, v.round()), f"{n}: integers"
        seen[n] = float(v.abs().max())
        assert seen[n] <= LIM_BF16, f"{n}: max {seen[n]} > 256 is not exact in bf16"
    assert float(ref_conv_acc(c.x.abs(), c.w.abs(), pad).max()) + 4 < LIM_FP32
    ax, aw, ab = ref_conv_bwd(c.x, c.w, r.dyc, pad, absolute=True)
    assert float(ax.max()) < LIM_FP32 and float(aw.max()) + 4 < LIM_FP32 and float(ab.max()) + 4 < LIM_FP32
    seen["dw"], seen["db"] = float(r.dw.abs().max()), float(r.db.abs().max())
    seen["ties"] = float(r.ties.double().mean())
    if pool == 2 and (conv_dims(geom)[0] % 2 or conv_dims(geom)[1] % 2):
        OH, OW, PH, PW = conv_dims(geom)
        assert (r.dyc[:, :, 2 * PH:, :] == 0).all() and (r.dyc[:, :, :, 2 * PW:] == 0).all()
    return seen
