"""CPU side of the element-exact Linear / thin-conv suite (tests/exact_linear.py): every
reference against float64 torch on the same operands (matmul; conv2d + max_pool2d + autograd),
the exactness preconditions of every case the GPU file runs, the tie rule, and the split-K plan
mirror against the table of expected plans."""
import pytest
import torch
import torch.nn.functional as F

import exact_linear as el

F64 = torch.float64


# ------------------------------------------------------------------ GEMM
def test_case_lists_cover_what_they_claim():
    cases = el.all_gemm_cases()
    f32 = {(c.ta, c.tb, c.tc if c.out != "C32" else "f") for c in cases if not el.uses_bf16_kernel(c)}
    b16 = {(c.tb, c.tc if c.out != "C32" else "f") for c in cases if el.uses_bf16_kernel(c)}
    assert len(f32) == 8 and len(b16) == 4  # every instantiation of the dispatch
    for kern in (False, True):
        mine = [c for c in cases if el.uses_bf16_kernel(c) == kern]
        assert {(c.la, c.lb) for c in mine} == set(el.LAYOUTS)
        for split in (False, True):
            sub = [c for c in mine if (el.case_plan(c)[0] > 1) == split]
            assert {c.beta for c in sub} == set(el.BETAS) and {c.alpha for c in sub} == set(el.ALPHAS)
            assert {c.out for c in sub} == {"C", "C32", "both"} and {c.pad for c in sub} == {0, 5}
            assert {(c.bias, c.relu) for c in sub} == {(a, b) for a in (False, True) for b in (False, True)}
            assert any(c.mask for c in sub)
            assert any(c.beta != 0 and c.out == "C" and c.tc == "b" for c in sub)  # beta reads a bf16 C
    for M, N in el.MN_EDGE:
        assert {c.K for c in el.edge_cases(M, N, False)} == set(el.K_NOSPLIT)
        assert all(el.case_plan(c)[0] == 1 for c in el.edge_cases(M, N, False))
    assert all(el.case_plan(c)[0] > 1 for kern in (False, True) for c in el.split_cases(kern))
    assert all(c.K % (32 if el.uses_bf16_kernel(c) else 64) for c in el.poison_cases())


def test_gemm_preconditions_hold_for_every_case():
    seen = [el.exact_preconditions(c) for c in dict.fromkeys(el.all_gemm_cases())]
    assert max(s["abs_sum"] for s in seen) <= 96 * (1 + 2.0 ** -6)
    assert max(s["abs_sum"] for s in seen) >= 48  # the sparse columns are not trivially short


def test_gemm_preconditions_bite(monkeypatch):
    """The same cases against a tighter sparsity limit, and a B column of 96 non-zeros, are refused."""
    c = el.GemmCase(130, 70, 300)
    el.exact_preconditions(c)
    monkeypatch.setattr(el, "NZ_PER_COLUMN", 47)
    with pytest.raises(AssertionError, match="non-zeros in a column"):
        el.exact_preconditions(c)
    monkeypatch.undo()
    monkeypatch.setattr(el, "sparse_b", lambda g_, K, N: torch.ones(K, N))
    dense = el.GemmCase(8, 8, 96, seed=99)  # a draw of its own: the shared ones stay as they are
    with pytest.raises(AssertionError, match="non-zeros in a column"):
        el.exact_preconditions(dense)


@pytest.mark.parametrize("case", [
    el.GemmCase(65, 63, 33), el.GemmCase(63, 65, 129, "m", "n", beta=0.5, bias=True, relu=True, alpha=0.125),
    el.GemmCase(130, 70, 300, "k", "n", "b", "f", "b", True, mask=True, beta=1.0, out="both", pad=5),
    el.GemmCase(64, 64, 272, "m", "k", "b", "f", "f", True, bfrac=True, alpha=2.0),
    el.GemmCase(1, 1, 1, "m", "n"), el.GemmCase(32, 120, 400, "m", "n", mask=True)], ids=el.gemm_id)
def test_gemm_reference_against_float64_matmul(case):
    """The strided, selected, rounded reference against torch.matmul in float64 on the logical
    operands (transposed back from their storage order by torch, not by index arithmetic)."""
    o, d = el.gemm_operands(case), el.gemm_draw(case.M, case.N, case.K, case.seed)
    A = (o.A if case.la == "k" else o.A.t()).double()
    if case.mask:
        A = A.masked_fill(~(d.maskv > 0), 0.0)
    B = o.B.bfloat16() if el.uses_bf16_kernel(case) else o.B
    B = (B if case.lb == "n" else B.t()).double()
    want = case.alpha * torch.matmul(A, B)
    if case.beta:
        want = want + case.beta * d.prior.double()
    if case.bias:
        want = want + d.bias.double()
    if case.relu:
        want = want.clamp_min(0)
    assert torch.equal(el.gemm_ref(case), want)  # exact operands: equal whatever matmul's order


def test_lowp_b_rounding_covers_the_ties():
    c = el.GemmCase(64, 64, 272, "k", "k", "b", "f", "f", True, bfrac=True)
    raw = el.gemm_operands(c).B.double()
    _, b = el.gemm_terms(c)
    assert set(b.abs().unique().tolist()) == {0.0, 1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6}
    r = raw[raw != 0].abs()
    assert {float(v) for v in r.unique()} == {1 + f for f in el.B_FRACTIONS}
    # 1 + 2^-8 and 1 + 3 * 2^-8 are halfway cases: to even, i.e. down and up
    assert el.round_to(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=F64), el.BF).tolist() == \
        [1.0, 1 + 2.0 ** -6]


def test_bf16_output_rounding_is_exercised_with_halfway_cases():
    """alpha = 0.125 on |sum| <= 96 gives eighths below 16: seven significand bits, a bf16 number
    as it stands.  The output rounding (f2bf) is exercised by the lowp cases whose B needed
    rounding: multiples of 2^-7 up to ~100, thousands of them halfway between two bf16 numbers."""
    c = el.GemmCase(65, 63, 65, ta="b", tb="b", tc="b", lowp=True, alpha=0.125, beta=0.5)
    assert torch.equal(el.round_to(el.gemm_ref(c), el.BF), el.gemm_ref(c))
    inexact = halfway = 0
    for c in dict.fromkeys(el.dtype_cases()):
        if c.tc == "b" and c.out != "C32" and c.bfrac:
            ref = el.gemm_ref(c)
            r = el.round_to(ref, el.BF)
            inexact += int((r != ref).sum())
            halfway += int(((r != ref) & ((ref - r).abs() == el.ulp(ref, 8) / 2)).sum())
    assert inexact > 1000 and halfway > 100


def test_plan_mirror_matches_the_table():
    for key, want in el.EXPECTED_PLANS.items():
        assert el.plan_mirror(*key) == want, key
    # the properties the split cases were written for
    S, kc, ch = el.plan_mirror(32, 120, 400, 0, 0)
    assert 400 - (ch - 1) * kc == 16  # LeNet fc1: the last chunk is 16 wide
    S, kc, ch = el.plan_mirror(63, 61, 257, 0, 0)
    assert 257 - (ch - 1) * kc == 1
    S, kc, ch = el.plan_mirror(64, 64, 272, 1, 1)
    assert (ch - 1) * kc >= 272  # the last launched chunk is empty
    S, kc, ch = el.plan_mirror(63, 65, 130, 1, 1)
    assert (kc, 130 - kc) == (96, 34)
    for c in el.all_gemm_cases():
        S, kc, ch = el.case_plan(c)
        assert ch <= S and (S == 1 or kc * ch >= c.K)
        # a chunk is a whole number of k stages: the staging bound gk < ke only ever cuts at K
        assert S == 1 or kc % (32 if el.uses_bf16_kernel(c) else 64) == 0


def test_tierb_reference_and_bound():
    for M, N, K, lowp in el.TIERB_SHAPES:
        c = el.tierb_case(M, N, K, lowp)
        want = torch.matmul(c.A.double(), c.B.double().t())
        torch.testing.assert_close(c.ref, want, rtol=1e-12, atol=1e-12)
        # an fp32 evaluation in k order (one rounding per accumulate) stays inside the bound
        acc = torch.zeros(M, N)
        a32, b32 = c.A.float(), c.B.float().t()
        for k in range(K):
            acc = acc + a32[:, k:k + 1] * b32[k:k + 1, :]
        err = (acc.double() - c.ref).abs()
        assert (err <= c.bound + el.half_ulp(c.ref, el.F32)).all()
        assert float((err / c.bound).max()) < 0.25  # and is far from its edge


# ------------------------------------------------------------------ colsum / bias_act
def test_colsum_and_bias_act_references():
    for M in el.COLSUM_M:
        for N in el.COLSUM_N:
            c = el.colsum_case(M, N)
            assert el.colsum_preconditions(c) <= 2 * M
            assert torch.equal(el.ref_colsum(c, False, 0.0), c.a.double().sum(0))
            kept = c.a.double() * (c.maskv > 0)
            assert torch.equal(el.ref_colsum(c, True, 0.5), 0.5 * c.prior.double() + kept.sum(0))
            assert not torch.isfinite(c.a_masked[~(c.maskv > 0)]).any()
    c = el.bias_act_case(5, 65)
    v = el.ref_bias_act(c, True, True)
    assert torch.equal(v, F.relu(c.y.double() + c.bias.double()))
    assert torch.equal(v.float().double(), v) and (el.round_to(v, el.BF) != v).any()


# ------------------------------------------------------------------ thin conv
TIE_CAP = 0.2  # share of 2x2 windows whose maximum is not unique (5-13 % with these integer draws)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("geom", el.CONV_GEOMS + [el.CONV_SLICE_GEOM], ids=str)
def test_conv_references_against_torch(geom, relu, bias):
    """y, dx, dw, db against conv2d + max_pool2d + autograd in float64.  torch's pooling has a
    tie rule of its own, so the backward is taken through torch's argmax (ref_unpool is given
    torch's codes), and the codes themselves are compared where the window has no tie."""
    B, Cin, H, W, Cout, K, pad, pool = geom
    OH, OW, PH, PW = el.conv_dims(geom)
    c, r = el.conv_case(geom), el.conv_refs(geom, relu, bias)
    seen = el.conv_preconditions(geom, relu, bias)
    x = c.x.double().requires_grad_(True)
    w = c.w.double().requires_grad_(True)
    b = c.bias.double().requires_grad_(True)
    acc = F.conv2d(x, w, None, 1, pad)
    if pool == 2:
        pooled, ind = F.max_pool2d(acc, 2, 2, return_indices=True)
        oh, ow = ind // OW, ind % OW
        code = ((oh - 2 * torch.arange(PH).view(1, 1, PH, 1)) * 2 + (ow - 2 * torch.arange(PW).view(1, 1, 1, PW)))
        code = code.to(torch.uint8)
    else:
        pooled, code = acc, torch.zeros(acc.shape, dtype=torch.uint8)
    y = pooled + b.view(1, -1, 1, 1) if bias else pooled
    y = F.relu(y) if relu else y
    assert torch.equal(r.y, y.detach())
    y.backward(c.dp.double())
    assert seen["ties"] < TIE_CAP, seen
    if pool == 2:
        assert seen["ties"] > 0  # the tie rule is exercised on the GPU
        assert torch.equal(r.code[~r.ties], code[~r.ties])
    # torch passes relu's gradient where y > 0, as the kernel's "live" rule does
    dyc = el.ref_unpool(c.dp, r.y, code, OH, OW, pool, relu)
    dx, dw, db = el.ref_conv_bwd(c.x, c.w, dyc, pad)
    assert torch.equal(dx, x.grad) and torch.equal(dw, w.grad)
    assert torch.equal(db, b.grad if bias else dyc.sum((0, 2, 3)))


def test_conv_codes_against_torch_on_tie_free_data():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 11, 9, generator=g, dtype=F64)
    w = torch.randn(4, 3, 3, 3, generator=g, dtype=F64)
    y, code, ties = el.ref_conv_fwd(x, w, None, 1, 2, False)
    assert not ties.any()
    want, ind = F.max_pool2d(F.conv2d(x, w, None, 1, 1), 2, 2, return_indices=True)
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)
    PH, PW = code.shape[2:]
    oh, ow = ind // 9, ind % 9
    assert torch.equal(code.long(), (oh - 2 * torch.arange(PH).view(-1, 1)) * 2 + ow - 2 * torch.arange(PW))


def test_pool_tie_rule_on_hand_written_windows():
    """First strict maximum in (dy, dx) row-major order; the bias and ReLU come after the choice."""
    acc = torch.tensor([[3.0, 3.0, 1.0, 5.0], [3.0, 3.0, 5.0, 5.0]]).view(1, 1, 2, 4)
    best, code, ties = el.ref_pool_first_max(acc, 2)
    assert best.flatten().tolist() == [3.0, 5.0] and code.flatten().tolist() == [0, 1] and ties.all()
    acc = torch.tensor([[-4.0, -2.0], [-2.0, -3.0]]).view(1, 1, 2, 2)
    y, code, ties = el.ref_conv_fwd(torch.ones(1, 1, 1, 1), torch.ones(1, 1, 1, 1), None, 0, 1, True)
    assert y.item() == 1.0 and code.item() == 0
    best, code, ties = el.ref_pool_first_max(acc, 2)
    assert best.item() == -2.0 and code.item() == 1  # all windows negative: still the first maximum
    # an odd conv output: the last row and column belong to no window and get no gradient
    dyc = el.ref_unpool(torch.ones(1, 1, 1, 1), torch.ones(1, 1, 1, 1), torch.full((1, 1, 1, 1), 3, dtype=torch.uint8),
                        3, 3, 2, True)
    assert dyc.flatten().tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]


def test_conv_workspace_formula():
    assert el.conv_workspace((2, 1, 28, 28, 6, 5, 2, 2), 1) == 2 * 6 * 784 + 2 * (150 + 6)
    assert el.conv_workspace(el.CONV_SLICE_GEOM, 2) == (5 * 3 * 77 + 63) // 64 * 64 + 3 * (54 + 3)
    assert el.conv_workspace(el.CONV_SLICE_GEOM, 8) == (5 * 3 * 77 + 63) // 64 * 64 + (54 + 3)
