"""Preconditions and reference self-checks of the exact LeNet / optimiser suite
(tests/exact_lenet.py), no GPU.

tests/test_exact_lenet_gpu.py compares the fused LeNet step and the flat optimiser kernels
with float64 references bit for bit.  That is only sound if every intermediate the kernels form
is exactly representable in any accumulation order; this file asserts that for every case the
GPU file draws (both take their cases from exact_lenet.py), that the pool ties, the zero
pre-activations, the zero seeds and the planted logit ties the comparison lives on are there,
that the odd-batch bound separates a dropped or doubled sample from rounding, and that the
references agree with float64 torch autograd and torch.optim.SGD."""
import math

import pytest
import torch
import torch.nn.functional as F

import exact_lenet as el

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
LIM = el.LIM_FP32
ALL_ROWS = el.POW2_B + el.ODD_B + (el.CURSOR_ROWS,)


def _step(n):
    c = el.case(n)
    return c, el.ref_step(c.x, c.labels, c.W)


def _batches():
    """(id, x, labels, W) of every batch a power-of-two GPU test runs."""
    out = [(f"B{n}", el.case(n).x, el.case(n).labels, el.case(n).W) for n in el.POW2_B]
    lc = el.label_case()
    out.append(("labels", lc.x, lc.labels, lc.W))
    cc = el.case(el.CURSOR_ROWS)
    for k in range(3):
        rows = el.clamped_rows(k)
        out.append((f"cursor{k}", cc.x[rows], cc.labels[rows], cc.W))
    return out


BATCHES = _batches()


def _is_int(v):
    return torch.equal(v, v.round())


def _fp32(name, v):
    assert torch.equal(el.fp32_roundtrip(v), v), f"{name}: not representable in fp32"


def _sum_ok(name, v, abs_terms, unit):
    """v and its terms are multiples of `unit`, and the sum of the terms' absolute values is
    below 2^24 units: every partial sum in any order is exact in fp32."""
    assert _is_int(v / unit), f"{name}: not a multiple of {unit}"
    assert (v.abs() <= abs_terms).all(), name
    m = float(abs_terms.max() / unit)
    assert m < LIM, f"{name}: sum of |terms| = {m} units >= 2^24"
    _fp32(name, v)


def _tie_share(a):
    """Share of the 2x2 windows whose maximum is positive and held by more than one element,
    and of those whose maximum is <= 0."""
    win = torch.stack([a[:, :, (k >> 1)::2, (k & 1)::2] for k in range(4)], -1)
    mx = win.max(-1).values
    tied = ((win == mx[..., None]).sum(-1) > 1) & (mx > 0)
    return tied.double().mean().item(), (mx <= 0).double().mean().item()


# ------------------------------------------------------------------ layout and operands
def test_flat_layout():
    off, total = el.flat_layout()
    assert off[2] % 4 == 0, "fc1.w is read as float4"
    assert any(o % 4 for o in off), "some segment starts off a 16-byte boundary"
    spans = sorted((o, o + n) for o, n in zip(off, el.SEG_N))
    assert spans[0][0] > 0 and spans[-1][1] < total
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 < b0, "a gap between every two segments"
    assert sorted(off) != off and sorted(off, reverse=True) != off, "permuted order"
    assert int(el.gap_mask().sum()) == total - sum(el.SEG_N)
    f = el.flat_of([torch.full((n,), float(i)) for i, n in enumerate(el.SEG_N)])
    assert torch.isnan(f[el.gap_mask()]).all() and not torch.isnan(f[~el.gap_mask()]).any()
    assert f[off[6]] == 6 and f[off[6] + 149] == 6
    assert el.REC_USED == 400 + 120 + 120 + 10 and el.CS == 2400 + 16 + 150 + 6
    assert len(el.CURSOR_SIDX) == 3 * el.CURSOR_B


@pytest.mark.parametrize("n", ALL_ROWS)
def test_operands(n):
    c = el.case(n)
    W = c.W
    assert _is_int(c.x) and c.x.abs().max() == 2 and tuple(c.x.shape) == (n, 1, 28, 28)
    assert torch.equal(c.x.to(BF).float(), c.x), "the images are exact in bf16"
    assert set(W.c1w.unique().tolist()) == {-1.0, 0.0, 1.0}
    for k, keep in (("c2w", el.KEEP2), ("f1w", el.KEEP_F1)):
        w = getattr(W, k)
        assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert abs((w != 0).float().mean().item() - keep) < 0.01
    for k, lim in (("c1b", 2), ("c2b", 2), ("f1b", 8)):
        b = getattr(W, k)
        assert _is_int(b) and b.abs().max() <= lim
    assert set(W.f2w.unique().tolist()) == {-128.0, 0.0, 128.0}
    assert _is_int(W.f2b / 128) and W.f2b.abs().max() <= 256
    dup = sum(1 for i in range(10) for j in range(i) if torch.equal(W.f2w[i], W.f2w[j]) and W.f2b[i] == W.f2b[j])
    assert dup >= 1, "planted duplicate fc2 rows"
    assert c.labels.dtype == torch.long and c.labels.min() >= 0 and c.labels.max() < 10


def test_cursor_case():
    s, n, B = el.CURSOR_SIDX, el.CURSOR_ROWS, el.CURSOR_B
    assert -3 in s and n + 5 in s
    inside = [r for r in s if 0 <= r < n]
    assert len(set(inside)) == len(inside) - 1, "one repeated row"
    assert set(inside) | {0, n - 1} == set(range(n)), "a permutation otherwise"
    rows = [el.clamped_rows(k) for k in range(3)]
    assert any(0 in r and -3 in s[k * B:(k + 1) * B] for k, r in enumerate(rows))
    assert any(n - 1 in r and n + 5 in s[k * B:(k + 1) * B] for k, r in enumerate(rows))
    # labels read at the clamped row: they differ from the labels at the batch position and
    # the clamped rows' records differ from every other row's
    lab = el.case(n).labels
    for k, r in enumerate(rows):
        assert lab[r].tolist() != lab[:B].tolist()
    f = el.ref_forward(el.case(n).x, el.case(n).W)
    for a in range(n):
        for b in range(a):
            assert not torch.equal(f.h0[a], f.h0[b])


def test_label_case():
    lc = el.label_case()
    assert sorted(lc.labels[list(lc.invalid)].tolist()) == sorted(el.INVALID_LABELS)
    r = el.ref_step(lc.x, lc.labels, lc.W)
    ok = [b for b in range(8) if b not in lc.invalid]
    assert r.valid.tolist() == [b in ok for b in range(8)]
    for b in lc.invalid:
        assert r.rowloss[b] == 0 and not r.dl[b].any() and not r.dh1[b].any() and not r.cslab[b].any()
    for b in ok:
        assert r.dl[b].any() and r.cslab[b].any() and r.rowloss[b] > 0
    full = el.ref_step(el.case(8).x, el.case(8).labels, el.case(8).W)
    assert torch.equal(r.dl[ok], full.dl[ok]), "valid rows keep their seed: the mean divides by B"
    assert r.loss == r.rowloss[ok].sum() / 8
    # the same as dropping the rows from the sums, not from the divisor
    g, _ = el.reduce_records(full.rec, full.cslab, keep=ok)
    for a, b in zip(r.grads, g):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ references against autograd
@pytest.mark.parametrize("n", ALL_ROWS)
def test_reference_against_float64_autograd(n):
    """F.conv2d, F.relu, F.max_pool2d (first maximum, as the kernels), F.linear and the exact
    seed in float64: every forward tensor, the gradients at a1, a2, z1, the batch gradients
    and, one sample at a time, the per-sample conv partials.  All quantities are dyadic and
    short, so float64 is exact in either formulation: compared with torch.equal."""
    c, r = _step(n)
    P = {k: getattr(c.W, k).double().requires_grad_(True) for k in el.W_KEYS}
    a1 = F.conv2d(c.x.double(), P["c1w"], P["c1b"], padding=2)
    p1 = F.max_pool2d(F.relu(a1), 2)
    a2 = F.conv2d(p1, P["c2w"], P["c2b"])
    h0 = F.max_pool2d(F.relu(a2), 2).flatten(1)
    z1 = F.linear(h0, P["f1w"], P["f1b"])
    h1 = F.relu(z1)
    lg = F.linear(h1, P["f2w"], P["f2b"])
    for t in (a1, a2, z1):
        t.retain_grad()
    for got, want in ((r.a1, a1), (r.p1, p1), (r.a2, a2), (r.h0, h0), (r.z1, z1), (r.h1, h1), (r.lg, lg)):
        assert torch.equal(got, want.detach())
    # the seed: softmax - onehot over B, the softmax in float64 (exact zeros below -128)
    assert torch.exp(torch.tensor(-128.0, dtype=F32)) == 0 and torch.exp(torch.tensor(0.0, dtype=F32)) == 1
    assert (torch.softmax(lg.detach(), 1) - r.softmax).abs().max() < 1e-50
    assert torch.equal((r.softmax - F.one_hot(c.labels, 10)) * r.inv_b, r.dl)
    lg.backward(r.dl, retain_graph=True)
    assert torch.equal(r.da1, a1.grad) and torch.equal(r.dc2, a2.grad) and torch.equal(r.dh1, z1.grad)
    for k, g in zip(el.SEG_KEYS, r.grads):
        assert torch.equal(g, P[k].grad.flatten()), k
    lossf = F.cross_entropy(lg.detach(), c.labels, reduction="none")
    assert (lossf - r.rowloss).abs().max() <= 1e-9 * r.rowloss.abs().max()
    for b in range(n):
        for p in P.values():
            p.grad = None
        one = torch.zeros_like(r.dl)
        one[b] = r.dl[b]
        lg.backward(one, retain_graph=True)
        want = torch.cat([P[k].grad.flatten() for k in ("c2w", "c2b", "c1w", "c1b")])
        assert torch.equal(r.cslab[b], want), f"sample {b}"


# ------------------------------------------------------------------ Tier A preconditions
@pytest.mark.parametrize("name,x,labels,W", BATCHES, ids=[b[0] for b in BATCHES])
def test_exactness_preconditions(name, x, labels, W):
    r = el.ref_step(x, labels, W)
    B = x.shape[0]
    assert B & (B - 1) == 0 and r.inv_b == 1.0 / B
    # forward: integers, the sums of the absolute values below 2^24
    for nm, v, a in (("conv1", r.a1, r.a1_abs), ("conv2", r.a2, r.a2_abs), ("fc1", r.z1, r.z1_abs),
                     ("fc2", r.lg, r.lg_abs)):
        _sum_ok(nm, v, a, 1.0)
    for nm in ("p1", "p2", "h1"):
        _fp32(nm, getattr(r, nm))
    # logits: multiples of 128, so two of a row are equal or at least 128 apart
    assert _is_int(r.lg / 128)
    gaps = (r.lg[:, :, None] - r.lg[:, None, :]).abs()
    assert ((gaps == 0) | (gaps >= 128)).all()
    assert set(r.ntie.tolist()) <= {1, 2, 4}
    assert set((r.dl * B * 4).unique().tolist()) <= {-4.0, -2.0, -1.0, 0.0, 1.0, 2.0, 4.0}
    untied = r.valid & (r.ntie == 1)
    assert _is_int(r.rowloss[untied]) and r.rowloss.abs().max() < LIM
    assert (r.rowloss_bound[untied] == 0).all() and (r.rowloss_bound[r.valid & (r.ntie > 1)] > 0).all()
    assert float(r.rowloss_bound.max()) <= 3 * 2.0 ** -4, "|logit| < 2^20: three ulps of 2^-4"
    # backward: multiples of 1 / (4 B)
    u = 1.0 / (4 * B)
    _fp32("dl", r.dl)
    _sum_ok("dh1", r.dh1_pre, r.dh1_abs, u)
    _sum_ok("g2", r.dh0, r.dh0_abs, u)
    _sum_ok("g1", r.dp1, r.dp1_abs, u)
    _sum_ok("slab", r.cslab, r.cslab_abs, u)
    for nm, g, a in zip(el.SEG_NAMES, r.grads, r.grads_abs_whole):
        _sum_ok(f"grad {nm}", g, a, u)
    # the update: d, the buffer and p of both calls, every intermediate
    for momentum, nesterov in el.SGD_VARIANTS:
        mom = {}
        for first in (True, False):  # the second call: the weights put back, the buffer kept
            for nm, g, p in zip(el.SEG_NAMES, r.grads, el.segs_of(W)):
                pn, bv, t = el.ref_sgd(p.double().flatten(), g, mom.get(nm), first, momentum, nesterov)
                for v in t:
                    _fp32(f"update {nm} m={momentum} nesterov={nesterov} first={first}", v)
                assert (bv is None) == (momentum == 0)
                mom[nm] = bv


@pytest.mark.parametrize("n", ALL_ROWS)
def test_coverage_conditions(n):
    """What the exact comparison needs to bite, asserted on the reference."""
    c, r = _step(n)
    t1, z1 = _tie_share(r.a1)
    t2, z2 = _tie_share(r.a2)
    assert t1 >= 0.05, f"pool 1: only {t1:.3f} of the windows tie for a positive maximum"
    assert t2 >= 0.01, f"pool 2: only {t2:.3f} of the windows tie for a positive maximum"
    assert z1 > 0 and z2 > 0 and (r.code1 == -1).any() and (r.code2 == -1).any()
    for code in (r.code1, r.code2):
        assert set(code.unique().tolist()) == {-1, 0, 1, 2, 3}
    assert (r.z1 == 0).any(), "some fc1 pre-activation is exactly 0"
    assert (r.z1 < 0).any() and (r.z1 > 0).any()
    if n >= 2:
        zero_seed = (r.ntie == 1) & (c.labels == r.am)
        assert zero_seed.any() and not r.dl[zero_seed].any()
        assert (r.softmax.gather(1, c.labels[:, None])[:, 0] == 0).any(), "label != argmax"
        assert (r.ntie > 1).any(), "a planted tie"
    if n >= 4:
        assert (r.ntie == 2).any() and (r.ntie == 4).any()
        assert (r.dl / r.inv_b == -0.5).any(), "a tied row labelled inside its tie"
    assert r.g1.abs().max() > 0 and r.cslab[:, el.S_C1W].abs().max() > 0


def test_zero_preactivation_with_a_gradient():
    """At z1 == 0 the h1 > 0 mask decides only where the unmasked gradient is not zero: some
    power-of-two case has such an element (a >= in the kernel would pass it on)."""
    hit = [n for n in el.POW2_B if (_step(n)[1].dh1_pre[_step(n)[1].z1 == 0] != 0).any()]
    assert hit, "no case has a non-zero gradient arriving at a zero pre-activation"


# ------------------------------------------------------------------ Tier B
@pytest.mark.parametrize("B", el.ODD_B)
def test_odd_batch_forward_is_exact_and_bound_separates(B):
    c, r = _step(B)
    assert r.inv_b != 1.0 / B and r.inv_b == float(torch.tensor(1.0 / B, dtype=F32))
    for nm, v, a in (("conv1", r.a1, r.a1_abs), ("conv2", r.a2, r.a2_abs), ("fc1", r.z1, r.z1_abs),
                     ("fc2", r.lg, r.lg_abs)):
        _sum_ok(nm, v, a, 1.0)
    # dl: a power-of-two multiple of fl(1 / B), exact in fp32
    q = r.dl / r.inv_b
    assert set(q.unique().tolist()) <= {-1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0}
    _fp32("dl", r.dl)
    # a dropped or doubled sample against the bound of the gradient kernel's sum
    g, a = el.reduce_records(r.rec, r.cslab)
    mid = B >> 1
    assert r.dl[mid].any(), "the sample between the two lanes' halves has a seed"
    for b in range(B):
        if not r.dl[b].any():
            continue
        for keep in ([i for i in range(B) if i != b], list(range(B)) + [b]):
            gd, _ = el.reduce_records(r.rec, r.cslab, keep=keep)
            for j, (nm, x, y, t) in enumerate(zip(el.SEG_NAMES, g, gd, a)):
                # a row labelled inside its 2-way tie has dh1 = (row - its duplicate) / 2B = 0
                # and reaches fc2 only; every other seeded row, the middle one among them,
                # reaches every segment
                if j >= 2 and not r.dh1[b].any() and b != mid:
                    assert torch.equal(x, y)
                    continue
                bound = el.odd_batch_bound(B, t)
                ratio = ((x - y).abs() / bound.clamp_min(1e-300)).max().item()
                assert ratio > 1e4, f"{nm}: sample {b} changes the sum by only {ratio:.3g} bounds"
    # the sample kernel's bound: above zero wherever the slab is, and small against it
    bd, bs = el.chain_bound(r)
    assert (bs >= 0).all() and (bs[r.cslab != 0] > 0).all() and (bd[r.dh1 != 0] > 0).all()
    assert (r.chain_cslab >= r.cslab.abs()).all() and (r.chain_dh1 >= r.dh1.abs()).all()
    assert bs.max() < 1e-3 * r.cslab.abs().max()


# ------------------------------------------------------------------ the optimiser cases
def test_bf16_ties():
    for v, want in el.BF16_TIES:
        t = torch.tensor([v], dtype=F32)
        assert t.double().item() == v, "exact in fp32"
        r = t.to(BF).double().item()
        assert r == want, (v, r, want)
        other = 2 * v - want  # the bf16 neighbour on the far side: v is exactly halfway
        assert other != want and torch.tensor([other], dtype=F32).to(BF).double().item() == other
        step = 2.0 ** (math.floor(math.log2(min(abs(want), abs(other)))) - 7)
        assert abs(want - other) == step, "adjacent bf16 numbers"
        even = lambda z: torch.tensor([z], dtype=F32).to(BF).view(torch.int16).item() & 1 == 0
        assert even(want) and not even(other), "to nearest even"
    ups = [abs(r) > abs(v) for v, r in el.BF16_TIES]
    assert any(ups) and not all(ups), "ties rounding up and down"


def test_planted_positions():
    assert el.planted(1) == [] and el.planted(3) == [1, 2] and el.planted(4) == [1, 3]
    assert el.planted(7) == [1, 5, 6] and el.planted(1029)[-1] == 1028


@pytest.mark.parametrize("n", el.OPT_N)
@pytest.mark.parametrize("momentum,nesterov", el.SGD_VARIANTS)
def test_sgd_case_is_exact(n, momentum, nesterov):
    c = el.sgd_case(n)
    idx = el.planted(n)
    for k, (pn, mom, t) in enumerate(el.sgd_refs(n, momentum, nesterov)):
        for v in t:
            _fp32(f"launch {k}", v)
        if idx:
            assert torch.equal(pn[idx], c.p[k][idx].double()), "a planted p stays on its tie"
            assert (pn[idx].to(F32).to(BF).double() != pn[idx]).all()
        rounds = pn.to(F32).to(BF).double() != pn
        assert rounds.sum() >= max(1, n // 2) or n == 1, "the bf16 shadow must round"
        assert (mom is None) == (momentum == 0)


@pytest.mark.parametrize("nesterov", [False, True])
def test_ref_sgd_against_torch_optim(nesterov):
    """torch.optim.SGD in float64 over three chained steps (torch refuses nesterov with
    dampening: that variant is compared at dampening 0)."""
    h = dict(el.HYPER, dampening=0.0 if nesterov else el.HYPER["dampening"])
    g = torch.Generator().manual_seed(3)
    p = torch.randn(50, generator=g, dtype=F64)
    q = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([q], lr=h["lr"], momentum=h["momentum"], dampening=h["dampening"],
                          weight_decay=h["wd"], nesterov=nesterov)
    mom = None
    for k in range(3):
        gr = torch.randn(50, generator=g, dtype=F64)
        p, mom, _ = el.ref_sgd(p, gr, mom, k == 0, h["momentum"], nesterov, h)
        q.grad = gr * h["gscale"]
        opt.step()
        assert (p - q.detach()).abs().max() < 1e-14


def test_rows_and_cast_cases():
    for rows in el.ROWS:
        for n in el.OPT_N:
            x, scale = el.rows_case(rows, n)
            assert _is_int(x) and x.abs().sum(0).max() < LIM and scale in (0.25, 0.125)
    for n in el.OPT_N:
        x = el.cast_case(n)
        assert (x.to(BF).float() != x).any() or n == 1
    x = el.cast_case(7)
    assert x[2] == 0 and x[3] == 0 and x.view(torch.int32)[3] != x.view(torch.int32)[2]


@pytest.mark.parametrize("n", el.ADAM_N)
@pytest.mark.parametrize("bias_correction", [False, True])
def test_ref_adam(n, bias_correction):
    """The float64 expression against the textbook Adam with decoupled-free weight decay, and
    the bound: positive, and a few ulps of the quantities involved."""
    c, h = el.adam_case(n), el.ADAM
    bc1, bc2 = el.adam_bias_corrections(2, bias_correction)
    (p, m, v), (Ep, Em, Ev) = el.ref_adam(c.p, c.g[0], c.m, c.v, bc1, bc2)
    gg = c.g[0].double() * h["gscale"] + h["wd"] * c.p.double()
    m2 = h["b1"] * c.m.double() + (1 - h["b1"]) * gg
    v2 = h["b2"] * c.v.double() + (1 - h["b2"]) * gg * gg
    p2 = c.p.double() - h["lr"] * (m2 * bc1) / ((v2 * bc2).sqrt() + h["eps"])
    for a, b in ((p, p2), (m, m2), (v, v2)):
        assert (a - b).abs().max() <= 1e-6 * b.abs().max()  # the hyperparameters' fp32 rounding
    assert (Ep > 0).all() and (Em > 0).all() and (Ev > 0).all()
    assert (Em <= 8 * 2.0 ** -23 * (m.abs() + c.m.abs().double() + gg.abs())).all()
    assert (Ep <= 64 * 2.0 ** -23 * (p.abs() + 1)).all(), "no element near a singular denominator"
