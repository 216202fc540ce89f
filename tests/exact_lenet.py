"""Element-exact references for the fused LeNet step (csrc/lenet_fused.hip) and the flat
optimiser kernels (csrc/optim.hip).

Integer images in [-2, 2], integer conv1 weights, sparse +-1 conv2 / fc1 weights, small integer
biases and fc2 weights in {0, +-128} with biases that are multiples of 128 make every forward
quantity an integer far below 2^24 and every logit a multiple of 128: two logits of a row are
equal or at least 128 apart, exp(0) = 1 and exp(d <= -128) = 0 in fp32, so the softmax is exactly
the indicator of the maximum (1/2 or 1/4 under a planted tie of duplicated fc2 rows).  At a batch
that is a power of two the seed is in {0, +-1, +-1/2, +-1/4} / B, every backward quantity a dyadic
rational with few bits, and with lr = 1/8, momentum = 1/2, dampening = 1/4, wd = 1/16,
gscale = 1/2 so are the update's d, buffer and p: the whole step is independent of the order
of any sum and must equal the float64 references here bit for bit.

This module draws the cases (case, label_case, cursor_case, the optimiser cases), computes the
float64 references from explicit tap and window loops (ref_step; never a library convolution
or pooling, never the code under test), and holds the bounds of what is not exact (tied
rows' loss, odd batches, Adam).  tests/test_exact_lenet_cpu.py proves the references and every
case's preconditions; tests/test_exact_lenet_gpu.py compares the kernels."""
import functools
import math
from types import SimpleNamespace

import torch

F32, F64 = torch.float32, torch.float64
LIM_FP32 = 1 << 24

# ------------------------------------------------------------------ layouts of the kernels
REC, REC_USED = 656, 650  # per-sample record: h0 (400) | h1 (120) | dh1 (120) | dl (10) | pad (6)
R_H0, R_H1, R_DH1, R_DL = slice(0, 400), slice(400, 520), slice(520, 640), slice(640, 650)
CS = 2572  # per-sample conv partials: conv2 w (2400) | conv2 b (16) | conv1 w (150) | conv1 b (6)
S_C2W, S_C2B, S_C1W, S_C1B = slice(0, 2400), slice(2400, 2416), slice(2416, 2566), slice(2566, 2572)
# flat segments in the order of the `off` argument
SEG_NAMES = ("fc2.w", "fc2.b", "fc1.w", "fc1.b", "conv2.w", "conv2.b", "conv1.w", "conv1.b")
SEG_N = (1200, 10, 48000, 120, 2400, 16, 150, 6)
SEG_KEYS = ("f2w", "f2b", "f1w", "f1b", "c2w", "c2b", "c1w", "c1b")
W_KEYS = ("c1w", "c1b", "c2w", "c2b", "f1w", "f1b", "f2w", "f2b")  # order of the `w` argument
# the segments' positions in the test's flat buffer: permuted, with gaps (NaN) before, between
# and after; fc1.w starts on a multiple of 4 floats (the sample kernel reads it as float4)
FLAT_ORDER = (7, 2, 1, 4, 3, 6, 0, 5)
FLAT_GAPS = (5, 3, 7, 2, 9, 1, 6, 4, 8)

HYPER = dict(lr=2.0 ** -3, momentum=0.5, dampening=0.25, wd=2.0 ** -4, gscale=0.5)
SGD_VARIANTS = ((0.0, False), (0.5, False), (0.5, True))  # (momentum, nesterov)
POW2_B, ODD_B = (1, 2, 4, 8), (3, 7)
INVALID_LABELS = (-1, -100, 10, 63, 67, (1 << 40) + 3)
KEEP2, KEEP_F1, KEEP_F2 = 0.12, 0.1, 0.3  # densities of conv2, fc1, fc2
SEEDS = {1: 11, 2: 41, 4: 16, 8: 14, 3: 16, 7: 11, 11: 11}  # per row count; tuned for coverage


def flat_layout():
    """(offsets by segment, total length) of the test's flat buffer."""
    off, pos = [0] * 8, FLAT_GAPS[0]
    for i, s in enumerate(FLAT_ORDER):
        if s == 2:
            pos = -(-pos // 4) * 4
        off[s] = pos
        pos += SEG_N[s] + FLAT_GAPS[i + 1]
    return off, pos


def flat_of(segs, fill=float("nan"), dtype=F64):
    """The flat buffer holding the eight segments (in `off` order) with `fill` in the gaps."""
    off, total = flat_layout()
    out = torch.full((total,), fill, dtype=dtype)
    for o, n, s in zip(off, SEG_N, segs):
        assert s.numel() == n
        out[o:o + n] = s.reshape(-1).to(dtype)
    return out


def gap_mask():
    off, total = flat_layout()
    m = torch.ones(total, dtype=torch.bool)
    for o, n in zip(off, SEG_N):
        m[o:o + n] = False
    return m


def ulp32(v):
    """The fp32 unit in the last place at |v| (float64 tensor or number; 2^-149 at 0)."""
    v = torch.as_tensor(v, dtype=F64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 23)


def fp32_roundtrip(v):
    return v.to(F32).to(F64)


# ------------------------------------------------------------------ operands
def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _sparse(g, shape, keep, scale=1.0):
    w = torch.zeros(math.prod(shape))
    idx = torch.randperm(w.numel(), generator=g)[:int(w.numel() * keep)]
    w[idx] = (torch.randint(0, 2, (idx.numel(),), generator=g).float() * 2 - 1) * scale
    return w.view(shape)


def _first_argmax(row):
    return int((row == row.max()).nonzero()[0])


def _plant_ties(W, h1):
    """Duplicate fc2 rows so that some samples' maximum is shared: the rarest argmax class
    is copied onto one class that is no sample's argmax (a 2-way tie for the samples of that
    class) and, from 4 samples on, the next rarest onto three more (a 4-way tie).  The other
    samples keep their argmax: the copies hold one of their smaller logits.  h1 does not depend
    on fc2, so this is a pure edit."""
    am = (h1 @ W.f2w.double().t() + W.f2b.double()).argmax(1).tolist()
    by_count = sorted(set(am), key=lambda c: (am.count(c), c))
    free = [c for c in range(10) if c not in am]
    plan = [(by_count[0], free[:1])]
    if h1.shape[0] >= 4 and len(by_count) > 1:
        plan.append((by_count[1], free[1:4]))
    for src, dst in plan:
        for c in dst:
            W.f2w[c], W.f2b[c] = W.f2w[src].clone(), W.f2b[src].clone()


def _labels(lg):
    """Labels from the reference logits: an untied row takes its argmax when b % 4 == 0 (a zero
    seed) and another class otherwise; a row tied 2 ways takes the second tied class from
    row 2 on (seed +1/2, -1/2) and a class outside the tie otherwise; a row tied more ways
    always takes a class outside (the seed stays a power of two over B)."""
    out = []
    for b in range(lg.shape[0]):
        tie = (lg[b] == lg[b].max()).nonzero().flatten().tolist()
        c = (tie[0] + 1 + b) % 10
        while c in tie:
            c = (c + 1) % 10
        if len(tie) == 1:
            out.append(tie[0] if b % 4 == 0 else c)
        elif len(tie) == 2:
            out.append(tie[1] if b >= 2 else c)
        else:
            out.append(c)
    return torch.tensor(out, dtype=torch.long)


@functools.lru_cache(maxsize=None)
def case(nrows):
    """Weights, `nrows` images and their labels (shared: do not modify)."""
    g = torch.Generator().manual_seed(SEEDS[nrows])
    c = SimpleNamespace(nrows=nrows)
    c.x = _randint(g, -2, 2, (nrows, 1, 28, 28))
    for b in range(nrows):  # blank parts of most images: the samples' features and argmax differ
        if b % 4 == 1:
            c.x[b, :, 14:, :] = 0
        elif b % 4 == 2:
            c.x[b, :, :, :14] = 0
        elif b % 4 == 3:
            keep = (torch.rand(4, 4, generator=g) > 0.5).float()
            c.x[b] *= keep.repeat_interleave(7, 0).repeat_interleave(7, 1)
    W = SimpleNamespace()
    W.c1w, W.c1b = _randint(g, -1, 1, (6, 1, 5, 5)), _randint(g, -2, 2, (6,))
    W.c2w, W.c2b = _sparse(g, (16, 6, 5, 5), KEEP2), _randint(g, -2, 2, (16,))
    W.f1w, W.f1b = _sparse(g, (120, 400), KEEP_F1), _randint(g, -8, 8, (120,))
    W.f2w, W.f2b = _sparse(g, (10, 120), KEEP_F2, 128.0), _randint(g, -2, 2, (10,)) * 128
    c.W = W
    f = ref_forward(c.x, W)
    _plant_ties(W, f.h1)
    c.labels = _labels(ref_forward(c.x, W).lg)
    return c


@functools.lru_cache(maxsize=None)
def label_case():
    """The 8-row case with six labels outside [0, 10): rows 1 and 7 stay valid."""
    c = case(8)
    lab = c.labels.clone()
    rows = (0, 2, 3, 4, 5, 6)
    lab[list(rows)] = torch.tensor(INVALID_LABELS)
    return SimpleNamespace(nrows=8, x=c.x, W=c.W, labels=lab, invalid=rows)


CURSOR_B, CURSOR_ROWS = 4, 11
# three batches of 4: a permutation of the 11 rows with row 5 repeated, one entry below 0
# (clamped to row 0) and one past the end (clamped to row 10)
CURSOR_SIDX = (7, 2, 5, -3, 9, 4, CURSOR_ROWS + 5, 1, 5, 8, 3, 6)


def clamped_rows(batch):
    s = CURSOR_SIDX[batch * CURSOR_B:(batch + 1) * CURSOR_B]
    return [min(max(r, 0), CURSOR_ROWS - 1) for r in s]


# ------------------------------------------------------------------ float64 references
def _conv(xp, w, b):
    """y[n, o] = b[o] + sum_{c, kh, kw} xp[n, c, y + kh, x + kw] w[o, c, kh, kw] (valid; tap loop)."""
    k = w.shape[-1]
    OH, OW = xp.shape[2] - k + 1, xp.shape[3] - k + 1
    y = b.view(1, -1, 1, 1).expand(xp.shape[0], w.shape[0], OH, OW).clone()
    for kh in range(k):
        for kw in range(k):
            y += torch.einsum("ncyx,oc->noyx", xp[:, :, kh:kh + OH, kw:kw + OW], w[:, :, kh, kw])
    return y


def _conv_dgrad(dy, w, H, W_):
    k = w.shape[-1]
    OH, OW = dy.shape[2:]
    dx = torch.zeros(dy.shape[0], w.shape[1], H, W_, dtype=F64)
    for kh in range(k):
        for kw in range(k):
            dx[:, :, kh:kh + OH, kw:kw + OW] += torch.einsum("noyx,oc->ncyx", dy, w[:, :, kh, kw])
    return dx


def _conv_wgrad(dy, xp, k):
    """Per sample: dw[n, o, c, kh, kw] = sum_{y, x} dy[n, o, y, x] xp[n, c, y + kh, x + kw]."""
    OH, OW = dy.shape[2:]
    dw = torch.zeros(dy.shape[0], dy.shape[1], xp.shape[1], k, k, dtype=F64)
    for kh in range(k):
        for kw in range(k):
            dw[:, :, :, kh, kw] = torch.einsum("noyx,ncyx->noc", dy, xp[:, :, kh:kh + OH, kw:kw + OW])
    return dw


def _pool(a):
    """relu + 2x2 max-pool by the kernels' rule: the windows' elements in the order (0,0), (0,1),
    (1,0), (1,1), an element wins when strictly greater than the best so far, which starts at 0:
    the first maximum wins a tie, code -1 (no gradient) where the maximum is <= 0."""
    n, c, H, W_ = a.shape
    best = torch.zeros(n, c, H // 2, W_ // 2, dtype=F64)
    code = torch.full(best.shape, -1, dtype=torch.long)
    for k in range(4):
        v = a[:, :, (k >> 1)::2, (k & 1)::2]
        up = v > best
        best, code = torch.where(up, v, best), torch.where(up, k, code)
    return best, code


def _unpool(g, code):
    n, c, PH, PW = g.shape
    out = torch.zeros(n, c, 2 * PH, 2 * PW, dtype=F64)
    for k in range(4):
        out[:, :, (k >> 1)::2, (k & 1)::2] = torch.where(code == k, g, 0.0)
    return out


def _dw(W):
    return SimpleNamespace(**{k: getattr(W, k).double() for k in W_KEYS})


def _abs(W):
    return SimpleNamespace(**{k: getattr(W, k).abs() for k in W_KEYS})


def ref_forward(x, W):
    """The forward in float64, with the sums of the terms' absolute values (`*_abs`)."""
    w, f = _dw(W), SimpleNamespace()
    wa = _abs(w)
    f.xp = torch.nn.functional.pad(x.double().view(-1, 1, 28, 28), (2, 2, 2, 2))
    f.a1, f.a1_abs = _conv(f.xp, w.c1w, w.c1b), _conv(f.xp.abs(), wa.c1w, wa.c1b)
    f.p1, f.code1 = _pool(f.a1)
    f.a2, f.a2_abs = _conv(f.p1, w.c2w, w.c2b), _conv(f.p1, wa.c2w, wa.c2b)
    f.p2, f.code2 = _pool(f.a2)
    f.h0 = f.p2.flatten(1)
    f.z1, f.z1_abs = f.h0 @ w.f1w.t() + w.f1b, f.h0 @ wa.f1w.t() + wa.f1b
    f.h1 = f.z1.clamp_min(0.0)
    f.lg, f.lg_abs = f.h1 @ w.f2w.t() + w.f2b, f.h1 @ wa.f2w.t() + wa.f2b
    return f


def inv_batch(B):
    """fl(1 / B) as the launcher computes it (fp32)."""
    return float(torch.tensor(1.0, dtype=F32) / torch.tensor(float(B), dtype=F32))


def ref_step(x, labels, W, B=None):
    """Everything one fused step forms for the samples x (their count is the batch unless B is
    given), in float64: the forward, the loss, the seed, the per-sample record and conv
    partials, the batch gradients, and for every sum the sum of its terms' absolute values."""
    r = ref_forward(x, W)
    w = _dw(W)
    wa = _abs(w)
    n = x.shape[0]
    r.B = B or n
    r.inv_b = inv_batch(r.B)
    mx = r.lg.max(1).values
    tie = r.lg == mx[:, None]
    r.ntie = tie.sum(1)
    r.am = tie.double().argmax(1)  # the first maximum
    r.valid = (labels >= 0) & (labels < 10)  # csrc/loss.hip: any other label is ignored
    lab = torch.where(r.valid, labels, 0)
    onehot = torch.nn.functional.one_hot(lab, 10).double()
    r.softmax = tie.double() / r.ntie[:, None]
    r.dl = (r.softmax - onehot) * r.inv_b * r.valid[:, None]
    zl = r.lg.gather(1, lab[:, None])[:, 0]
    lse = torch.log(r.ntie.double())
    r.rowloss = torch.where(r.valid, mx + lse - zl, 0.0)
    # untied (or ignored) rows are exact; a tied row's mx + logf(se) - z_label costs one fp32
    # ulp each for logf, the add and the subtract
    r.rowloss_bound = torch.where(r.valid & (r.ntie > 1),
                                  ulp32(lse) + ulp32(mx.abs() + lse) + ulp32(r.rowloss), 0.0)
    r.loss = r.rowloss.sum() / r.B
    # the mean: exact when every row is; else the rows' bounds, one ulp per add of the wave
    # sum (at the sum of the absolute values) and one for the division
    if bool((r.rowloss_bound == 0).all()):
        r.loss_bound = 0.0
    else:
        r.loss_bound = float((r.rowloss_bound.sum() + n * ulp32(r.rowloss.abs().sum())) / r.B
                             + ulp32(r.loss))
    # ---- backward
    r.dh1_pre, r.dh1_abs = r.dl @ w.f2w, r.dl.abs() @ wa.f2w
    r.dh1 = torch.where(r.z1 > 0, r.dh1_pre, 0.0)
    r.dh0, r.dh0_abs = r.dh1 @ w.f1w, r.dh1.abs() @ wa.f1w
    r.g2 = torch.where(r.code2 >= 0, r.dh0.view(n, 16, 5, 5), 0.0)
    r.dc2 = _unpool(r.g2, r.code2)
    r.dp1, r.dp1_abs = _conv_dgrad(r.dc2, w.c2w, 14, 14), _conv_dgrad(r.dc2.abs(), wa.c2w, 14, 14)
    r.g1 = torch.where(r.code1 >= 0, r.dp1, 0.0)
    r.da1 = _unpool(r.g1, r.code1)
    cat = lambda a, b, c, d: torch.cat([a.flatten(1), b.flatten(1), c.flatten(1), d.flatten(1)], 1)
    r.cslab = cat(_conv_wgrad(r.dc2, r.p1, 5), r.dc2.sum((2, 3)),
                  _conv_wgrad(r.da1, r.xp, 5), r.da1.sum((2, 3)))
    r.cslab_abs = cat(_conv_wgrad(r.dc2.abs(), r.p1, 5), r.dc2.abs().sum((2, 3)),
                      _conv_wgrad(r.da1.abs(), r.xp.abs(), 5), r.da1.abs().sum((2, 3)))
    r.rec = cat(r.h0, r.h1, r.dh1, r.dl)
    # the absolute values carried through the whole backward chain (for the odd-batch bound
    # of the sample kernel: an error made early is amplified by at most these sums)
    c_dh1 = torch.where(r.z1 > 0, r.dh1_abs, 0.0)
    c_dc2 = _unpool(torch.where(r.code2 >= 0, (c_dh1 @ wa.f1w).view(n, 16, 5, 5), 0.0), r.code2)
    c_da1 = _unpool(torch.where(r.code1 >= 0, _conv_dgrad(c_dc2, wa.c2w, 14, 14), 0.0), r.code1)
    r.chain_dh1 = c_dh1
    r.chain_cslab = cat(_conv_wgrad(c_dc2, r.p1, 5), c_dc2.sum((2, 3)),
                        _conv_wgrad(c_da1, r.xp.abs(), 5), c_da1.sum((2, 3)))
    r.grads, r.grads_abs = reduce_records(r.rec, r.cslab)
    _, cs_abs = reduce_records(r.rec, r.cslab_abs)
    r.grads_abs_whole = r.grads_abs[:4] + cs_abs[4:]  # down to the per-sample partials' terms
    return r


def reduce_records(rec, cslab, keep=None):
    """lenet_grad_kernel in float64: the eight gradients (in `off` order) from per-sample
    records [n, >= 650] and conv partials [n, 2572], and the sums of the batch terms' absolute
    values.  keep: the sample indices to sum (a dropped or doubled sample), default all."""
    rec, cslab = rec.double(), cslab.double()
    if keep is not None:
        rec, cslab = rec[list(keep)], cslab[list(keep)]
    h0, h1, dh1, dl = rec[:, R_H0], rec[:, R_H1], rec[:, R_DH1], rec[:, R_DL]
    outer = lambda a, b: torch.einsum("bi,bj->ij", a, b).flatten()
    g = [outer(dl, h1), dl.sum(0), outer(dh1, h0), dh1.sum(0)]
    a = [outer(dl.abs(), h1.abs()), dl.abs().sum(0), outer(dh1.abs(), h0.abs()), dh1.abs().sum(0)]
    for s in (S_C2W, S_C2B, S_C1W, S_C1B):
        g.append(cslab[:, s].sum(0))
        a.append(cslab[:, s].abs().sum(0))
    return g, a


def odd_batch_bound(B, abs_terms):
    """|grad - float64 sum| at a batch that is not a power of two: each lane of a parameter's
    pair accumulates at most (B + 1) / 2 terms with one rounding per accumulate (the product
    fused into it), the combine rounds once more: at most (B + 1) / 2 + 1 <= B / 2 + 2 roundings,
    each at most 2^-24 of a partial sum that never exceeds the sum of the absolute values."""
    return (B / 2 + 2) * 2.0 ** -24 * abs_terms


# Roundings along the longest chain of fp32 operations from the seed to an output of the sample
# kernel (products fused into the accumulates): fc2 dgrad 10; fc1 dgrad 12 + 10; conv2 dW and
# db 25; conv2 dgrad 150 + 16; conv1 dW 33 + 5, db 7 + 5.  Rounded up per slab section.
CHAIN_DH1 = 10
CHAIN_CSLAB = ((S_C2W, 60), (S_C2B, 60), (S_C1W, 240), (S_C1B, 240))


def chain_bound(r):
    """|dh1 - ref| and |cslab - ref| of the sample kernel at a batch that is not a power of two:
    every rounding is at most 2^-24 of a partial sum, and a partial sum (and what an earlier
    error grows to on its way to the output) never exceeds the chain of absolute values."""
    b = torch.zeros_like(r.chain_cslab)
    for s, k in CHAIN_CSLAB:
        b[:, s] = k * 2.0 ** -24 * r.chain_cslab[:, s]
    return CHAIN_DH1 * 2.0 ** -24 * r.chain_dh1, b


def ref_sgd(p, g, mom, first, momentum, nesterov, h=HYPER):
    """torch.optim.SGD's update in float64: (p, buffer or None, every intermediate formed)."""
    t = [g * h["gscale"], h["wd"] * p]
    d = t[0] + t[1]
    t.append(d)
    bv = None
    if momentum != 0:
        if first:
            bv = d
        else:
            t += [momentum * mom, (1 - h["dampening"]) * d]
            bv = t[-2] + t[-1]
        t += [bv, momentum * bv]
        d = d + momentum * bv if nesterov else bv
        t.append(d)
    t.append(h["lr"] * d)
    pn = p - h["lr"] * d
    t.append(pn)
    return pn, bv, t


def segs_of(W):
    return [getattr(W, k) for k in SEG_KEYS]


# ------------------------------------------------------------------ csrc/optim.hip cases
OPT_N = (1, 3, 4, 7, 1029)
ROWS = (1, 3, 8)
# (value, its bf16 rounding): halfway between two bf16 numbers, to nearest-even down and up,
# in three binades, both signs; 1 + 255/256 carries into the exponent
_TIES = [(1 + 1 / 256, 1.0), (1 + 3 / 256, 1 + 1 / 64), (1 + 127 / 256, 1.5), (1 + 255 / 256, 2.0),
         (1 + 5 / 256, 1 + 1 / 64), (1 + 129 / 256, 1.5)]
BF16_TIES = [(s * e * v, s * e * r) for e in (1.0, 2.0 ** -3, 16.0) for s in (1.0, -1.0) for v, r in _TIES]


def planted(n):
    """The elements of an n-vector that hold bf16 ties: 1, 5, 9, ... and the last (n > 1), so the
    vector body, its scalar tail and the all-scalar path each round some."""
    idx = set(range(1, n, 4))
    if n > 1:
        idx.add(n - 1)
    return sorted(idx)


@functools.lru_cache(maxsize=None)
def sgd_case(n):
    """Three launches of dyadic (p, g): integers in [-8, 8]; a planted element holds a bf16 tie
    t in p and -t / 8 in g, so d = g / 2 + p / 16 = 0, its buffer stays 0 and the updated p is t
    again in every launch of every variant.  The buffer carries over; p is drawn afresh for each
    launch (the unit of p shrinks 2^7 per update: three chained ones leave fp32)."""
    g = torch.Generator().manual_seed(300 + n)
    c = SimpleNamespace(n=n, p=[], g=[])
    idx = planted(n)
    t = torch.tensor([BF16_TIES[(i + n) % len(BF16_TIES)][0] for i in range(len(idx))], dtype=F32)
    for _ in range(3):
        p, gr = _randint(g, -8, 8, (n,)), _randint(g, -8, 8, (n,))
        if idx:
            p[idx], gr[idx] = t, -t / 8
        c.p.append(p)
        c.g.append(gr)
    return c


@functools.lru_cache(maxsize=None)
def sgd_refs(n, momentum, nesterov):
    """Per launch: (p after, buffer after or None, the intermediates), float64."""
    c, out, mom = sgd_case(n), [], None
    for k in range(3):
        pn, mom, t = ref_sgd(c.p[k].double(), c.g[k].double(), mom, k == 0, momentum, nesterov)
        out.append((pn, mom, t))
    return out


@functools.lru_cache(maxsize=None)
def cast_case(n):
    """fp32 values for cast_f32_bf16: the ties, Gaussians, both zeros."""
    g = torch.Generator().manual_seed(400 + n)
    x = torch.randn(n, generator=g) * 3
    for j, i in enumerate(planted(n)):
        x[i] = BF16_TIES[(j + 2 * n) % len(BF16_TIES)][0]
    if n >= 7:
        x[2], x[3] = 0.0, -0.0
    return x


@functools.lru_cache(maxsize=None)
def rows_case(rows, n):
    """Integer rows and a power-of-two scale: out = scale * sum_r x[r] exactly."""
    g = torch.Generator().manual_seed(500 + 10 * rows + n)
    return _randint(g, -64, 64, (rows, n)), (1.0 / 8 if rows == 8 else 0.25)


ADAM = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, gscale=0.5)
ADAM_N = (7, 1029)


@functools.lru_cache(maxsize=None)
def adam_case(n):
    g = torch.Generator().manual_seed(600 + n)
    r = lambda: torch.randn(n, generator=g)
    return SimpleNamespace(n=n, p=r(), m=r() * 0.1, v=r().square() * 0.1, g=[r(), r()])


def adam_bias_corrections(t, on):
    return (1 / (1 - ADAM["b1"] ** t), 1 / (1 - ADAM["b2"] ** t)) if on else (1.0, 1.0)


def ref_adam(p, g, m, v, bc1, bc2, h=ADAM):
    """adam_kernel's expression in float64 on fp32 operands and fp32 hyperparameters (1 - b
    as the fp32 difference the kernel forms), and the per-element error bound of the fp32
    evaluation: one ulp (2^-23 relative) for each multiply, add, sqrtf and the division,
    propagated to first order.  A rounding is at most half an ulp, which leaves a factor of two
    for the second-order terms.  Returns (p, m, v), (bound_p, bound_m, bound_v)."""
    f = lambda s: float(torch.tensor(s, dtype=F32))
    lr, b1, b2, eps, wd, gs = (f(h[k]) for k in ("lr", "b1", "b2", "eps", "wd", "gscale"))
    c1 = float(torch.tensor(1.0, dtype=F32) - torch.tensor(b1, dtype=F32))
    c2 = float(torch.tensor(1.0, dtype=F32) - torch.tensor(b2, dtype=F32))
    bc1, bc2 = f(bc1), f(bc2)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    e = 2.0 ** -23
    gg = g * gs + wd * p
    E_gg = e * ((g * gs).abs() + (wd * p).abs()) + e * gg.abs()
    mn = b1 * m + c1 * gg
    E_m = e * (b1 * m).abs() + e * (c1 * gg).abs() + c1 * E_gg + e * mn.abs()
    cg = c2 * gg
    E_cg = c2 * E_gg + e * cg.abs()
    cgg = cg * gg
    E_cgg = gg.abs() * E_cg + cg.abs() * E_gg + e * cgg.abs()
    vn = b2 * v + cgg
    E_v = e * (b2 * v).abs() + E_cgg + e * vn.abs()
    mb = mn * bc1
    E_mb = bc1 * E_m + e * mb.abs()
    num = lr * mb
    E_num = lr * E_mb + e * num.abs()
    s = vn * bc2
    E_s = bc2 * E_v + e * s.abs()
    rt = s.sqrt()
    E_rt = E_s / (2 * (s - E_s).clamp_min(1e-300).sqrt()) + e * rt
    den = rt + eps
    E_den = E_rt + e * den
    den_lo = den - E_den
    q = num / den
    E_q = E_num / den_lo + num.abs() * E_den / (den_lo * den_lo) + e * q.abs()
    pn = p - q
    E_p = E_q + e * pn.abs()
    return (pn, mn, vn), (E_p, E_m, E_v)


# ------------------------------------------------------------------ the steps the GPU file runs
STEP_KEYS = ([("B", n) for n in POW2_B + ODD_B] + [("labels", 8)] + [("cursor", k) for k in range(3)])


def step_inputs(key):
    """(x, labels, W) of one step: a whole case, the invalid-label case, or the rows one batch
    of the cursor case selects."""
    kind, k = key
    if kind == "B":
        c = case(k)
        return c.x, c.labels, c.W
    if kind == "labels":
        c = label_case()
        return c.x, c.labels, c.W
    c, rows = case(CURSOR_ROWS), clamped_rows(k)
    return c.x[rows], c.labels[rows], c.W


@functools.lru_cache(maxsize=None)
def step_refs(key):
    """ref_step of one of STEP_KEYS, computed once (shared: do not modify)."""
    return ref_step(*step_inputs(key))
