"""Element-exact tests of the fused LeNet step (csrc/lenet_fused.hip) and the flat optimiser
kernels (csrc/optim.hip).

Integer images and weights, fc2 weights in {0, +-128} and dyadic hyperparameters make every
quantity of the step exactly representable at a power-of-two batch (tests/test_exact_lenet_cpu.py
asserts the preconditions of each case here), so the per-sample record, the conv partials, the
row losses, the flat gradient and the updated parameters and momentum must equal the float64
references of tests/exact_lenet.py bit for bit: both first-maximum pool rules on tied windows,
the h1 > 0 mask at zero, the argmax positions, every offset of the record, the slab and the flat
buffer.  Every output is a NaN-prefilled view between guard regions, the workspaces sized
exactly; every input sits between 0xFF guards; the flat buffers hold their segments in a
permuted order between NaN gaps that must stay NaN.

Bounded, not exact, with every bound derived in tests/exact_lenet.py: the loss of a row whose
maximum logit is tied (logf), the backward at the odd batches 3 and 7 (1 / B is not dyadic) and
Adam.  Not asserted: the 6 pad floats of a record beyond keeping their prefill, and the
backward at an odd batch beyond those bounds."""
from types import SimpleNamespace

import pytest
import torch

import exact_conv as ec
import exact_lenet as el
from dmlab.ops._native import lib

pytestmark = pytest.mark.gpu

BF, F32, F64, I64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.long, torch.int32
XDTYPES = [F32, BF]
dtid = lambda v: {F32: "f32", BF: "bf16"}.get(v, str(v))
W_SHAPES = ((6, 1, 5, 5), (6,), (16, 6, 5, 5), (16,), (120, 400), (120,), (10, 120), (10,))
RATIOS = {}  # worst error-to-bound ratios of the bounded comparisons, printed per test


class Bench:
    """Guarded device tensors of one test; done() checks every guard."""

    def __init__(self, dev):
        self.dev, self.outs, self.kept = dev, [], []

    def inp(self, t, dtype=None, what="operand"):
        v, chk = ec.guarded(tuple(t.shape), dtype or t.dtype, self.dev, "in")
        v.copy_(t.to(self.dev))
        self.kept.append((chk, what))
        return v

    def out(self, shape, dtype=F32, what="output", keep=False):
        """All NaN (0xFF bytes); keep: the guards are checked by every later done() too."""
        v, chk = ec.guarded(tuple(shape), dtype, self.dev, "out")
        (self.kept if keep else self.outs).append((chk, what))
        return v

    def done(self):
        for chk, what in self.outs + self.kept:
            chk(what)
        self.outs = []


def _exact(got, want, what):
    """Bit-equal values on the device; the element-wise report of assert_exact on a mismatch."""
    want = want.to(got.device)
    if got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want):
        return
    ec.assert_exact(got.reshape(want.shape), want, what, layout="")


def _all_nan_bits(t, what):
    """Every element still holds the 0xFF prefill (never written)."""
    bad = (t.contiguous().view(torch.uint8) != 0xFF).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} prefilled bytes were overwritten, first at byte {int(bad[0])}"


def _bf16_bits(got, want, what):
    """got (bf16, device) holds exactly the bits of want (bf16, CPU)."""
    g, w = got.cpu().view(torch.int16), want.view(torch.int16)
    bad = (g != w).nonzero().flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {g.numel()} bf16 values differ, first at {int(bad[0])}: "
                              f"got {float(got.cpu()[bad[0]])} want {float(want[bad[0]])}")


def _within(got, want, bound, what):
    """|got - want| <= bound element-wise (float64); returns the worst ratio."""
    err = (got.detach().double().cpu() - want).abs()
    assert not torch.isnan(err).any(), f"{what}: NaN (never written or poisoned)"
    bad = (err > bound).nonzero()
    ratio = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    assert bad.numel() == 0 and bool((err[bound == 0] == 0).all()), (
        f"{what}: {bad.shape[0]} of {err.numel()} elements exceed the bound, worst ratio {ratio:.3g}, "
        f"first at {bad[0].tolist() if bad.numel() else '-'}")
    return ratio


def _note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"[exact_lenet] {name}: worst error / bound = {RATIOS[name]:.4f}")


def _collect(checks):
    """Run every check; report all the failures, not only the first."""
    bad = []
    for fn in checks:
        try:
            fn()
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ one fused step
class Step:
    """The operands of one case on the device and the call itself.  The weights are views of
    the flat parameter buffer p, as in the model."""

    def __init__(self, dev, x, labels, W, xdtype, B=None, sidx=None):
        L, b = lib(), Bench(dev)
        assert L.lenet_record_floats() == el.REC and L.lenet_slab_floats() == el.CS
        self.b, self.dev, self.B = b, dev, B or x.shape[0]
        self.off, self.total = el.flat_layout()
        self.gap = el.gap_mask().to(dev)
        self.x = b.inp(x.to(xdtype), what="x")
        self.labels = b.inp(labels, I64, "labels")
        self.p = b.out((self.total,), F32, "p", keep=True)  # the gaps keep the 0xFF prefill
        self.seg_at = (~el.gap_mask()).nonzero().flatten().to(dev)
        self.seg0 = el.flat_of(el.segs_of(W), fill=0.0, dtype=F32).to(dev)[self.seg_at]
        self.restore()
        order = {k: i for i, k in enumerate(el.SEG_KEYS)}
        self.w = [self.p[self.off[order[k]]:self.off[order[k]] + el.SEG_N[order[k]]].view(s)
                  for k, s in zip(el.W_KEYS, W_SHAPES)]
        self.loss_sum = b.inp(torch.zeros(1), F32, "loss_sum")
        self.ix = {}
        if sidx is not None:
            self.sidx = b.inp(torch.tensor(sidx, dtype=I64), I64, "sidx")
            self.cursor = b.inp(torch.zeros(1, dtype=I32), I32, "cursor")
            self.ix = dict(sidx=self.sidx, cursor=self.cursor, batch=self.B)

    def restore(self):
        """Put the integer weights back into p's segments (the gaps are left alone)."""
        self.p[self.seg_at] = self.seg0

    def call(self, p=None, mom=None, momentum=0.0, nesterov=False, first=True):
        b, B, h = self.b, self.B, el.HYPER
        o = SimpleNamespace()
        o.rec = b.out((B * el.REC,), F32, "rec")
        o.cslab = b.out((B * el.CS,), F32, "cslab")
        o.rowloss, o.loss = b.out((B,), F32, "rowloss"), b.out((1,), F32, "loss")
        o.grad = b.out((self.total,), F32, "grad")
        lib().lenet_fused_step(self.x, self.labels, self.w, o.rec, o.cslab, o.rowloss, o.grad, self.off,
                               p, mom, h["lr"], momentum, h["dampening"], h["wd"], h["gscale"], nesterov,
                               first, o.loss, loss_sum=self.loss_sum, **self.ix)
        b.done()
        o.rec, o.cslab = o.rec.view(B, el.REC), o.cslab.view(B, el.CS)
        return o

    def flat_checks(self, got, segs, what):
        """The eight segments of a flat buffer exact, the gaps still prefilled."""
        out = [lambda: _all_nan_bits(got[self.gap], f"{what}: the gaps")]
        for nm, o, n, s in zip(el.SEG_NAMES, self.off, el.SEG_N, segs):
            out.append(lambda nm=nm, o=o, n=n, s=s: _exact(got[o:o + n], s.flatten(), f"{what} {nm}"))
        return out


def _step(dev, key, xdtype, **kw):
    x, labels, W = el.step_inputs(key)
    return Step(dev, x, labels, W, xdtype, **kw), el.step_refs(key)


def _forward_checks(o, r, label):
    """h0 | h1 of every record, the pad, the row losses and the mean."""
    exact = r.rowloss_bound == 0
    out = [lambda: _exact(o.rec[:, el.R_H0], r.h0, f"h0 ({label})"),
           lambda: _exact(o.rec[:, el.R_H1], r.h1, f"h1 ({label})"),
           lambda: _all_nan_bits(o.rec[:, el.REC_USED:], f"the record pad ({label})"),
           lambda: _exact(o.rowloss[exact.to(o.rowloss.device)], r.rowloss[exact], f"rowloss, untied rows ({label})"),
           lambda: _within(o.rowloss, r.rowloss, r.rowloss_bound, f"rowloss, tied rows ({label})")]
    if r.loss_bound == 0:
        out.append(lambda: _exact(o.loss, r.loss.view(1), f"loss ({label})"))
    else:
        out.append(lambda: _within(o.loss, r.loss.view(1), torch.tensor([r.loss_bound], dtype=F64), f"loss ({label})"))
    return out


def _seed_checks(o, r, label):
    return [lambda: _exact(o.rec[:, el.R_DL], r.dl, f"dl ({label})"),
            lambda: _exact(o.rec[:, el.R_DH1], r.dh1, f"dh1 ({label})")]


def _slab_checks(o, r, label):
    names = (("conv2 dW", el.S_C2W), ("conv2 db", el.S_C2B), ("conv1 dW", el.S_C1W), ("conv1 db", el.S_C1B))
    return [lambda nm=nm, s=s: _exact(o.cslab[:, s], r.cslab[:, s], f"slab {nm} ({label})") for nm, s in names]


@pytest.mark.parametrize("xdtype", XDTYPES, ids=dtid)
@pytest.mark.parametrize("B", el.POW2_B)
def test_step_forward_record_exact(dev, B, xdtype):
    """h0 (pool 2 of relu(conv2) of pool 1 of relu(conv1)) and h1 of every sample, the pad's
    prefill, rowloss (an integer mx - z_label on untied rows) and the mean loss."""
    s, r = _step(dev, ("B", B), xdtype)
    _collect(_forward_checks(s.call(), r, f"B {B}, {dtid(xdtype)}"))


@pytest.mark.parametrize("xdtype", XDTYPES, ids=dtid)
@pytest.mark.parametrize("B", el.POW2_B)
def test_step_seed_and_dh1_exact(dev, B, xdtype):
    """dl = (indicator of the maximum / its multiplicity - onehot) / B and dh1 masked by h1 > 0,
    zero pre-activations included."""
    s, r = _step(dev, ("B", B), xdtype)
    _collect(_seed_checks(s.call(), r, f"B {B}, {dtid(xdtype)}"))


@pytest.mark.parametrize("xdtype", XDTYPES, ids=dtid)
@pytest.mark.parametrize("B", el.POW2_B)
def test_step_conv_slab_exact(dev, B, xdtype):
    """The whole cslab row of every sample: conv2 dW / db through the pool-2 argmax positions,
    conv1 dW / db through the pool-1 ones; 5-30 % of the windows tie for a positive maximum, so
    the first-maximum rule decides which input pixel a gradient meets."""
    s, r = _step(dev, ("B", B), xdtype)
    _collect(_slab_checks(s.call(), r, f"B {B}, {dtid(xdtype)}"))


@pytest.mark.parametrize("xdtype", XDTYPES, ids=dtid)
@pytest.mark.parametrize("B", el.POW2_B)
def test_step_flat_grad_exact_and_grads_only_leaves_p(dev, B, xdtype):
    """flat.grad: eight segments in a permuted order, the gaps between them still NaN; the
    grads-only call (p = None) leaves no trace in the p and the momentum the test still holds;
    a second call gives the same bits and loss_sum = 2 loss."""
    s, r = _step(dev, ("B", B), xdtype)
    mom = s.b.out((s.total,), F32, "mom", keep=True)
    p0 = s.p.clone()
    o = s.call()
    label = f"B {B}, {dtid(xdtype)}"
    o2 = s.call()
    _collect(s.flat_checks(o.grad, r.grads, f"grad ({label})") + [
        lambda: _all_nan_bits(mom, "momentum not passed"),
        lambda: _exact(s.p.view(I32), p0.view(I32), "p not passed"),
        lambda: _exact(o2.grad.view(I32), o.grad.view(I32), "grad, second call"),
        lambda: _exact(o2.loss, o.loss, "loss, second call"),
        lambda: _exact(s.loss_sum, o.loss + o.loss, "loss_sum after two calls")])


@pytest.mark.parametrize("xdtype", XDTYPES, ids=dtid)
@pytest.mark.parametrize("momentum,nesterov", el.SGD_VARIANTS)
@pytest.mark.parametrize("B", el.POW2_B)
def test_step_fused_sgd_exact(dev, B, momentum, nesterov, xdtype):
    """The SGD fused into the gradient kernel, lr 1/8, momentum 1/2, dampening 1/4, wd 1/16,
    gscale 1/2: p and the buffer after first=True and after a second call with first=False (the
    integer weights put back, the buffer kept), the gaps of p, mom and grad untouched."""
    s, r = _step(dev, ("B", B), xdtype)
    mom = s.b.out((s.total,), F32, "mom", keep=True)
    label = f"B {B}, {dtid(xdtype)}, momentum {momentum}, nesterov {nesterov}"
    p0 = [w.double().flatten() for w in el.segs_of(el.step_inputs(("B", B))[2])]
    checks, bufs, losses = [], [None] * 8, []
    for first in (True, False):
        s.restore()
        o = s.call(p=s.p, mom=mom, momentum=momentum, nesterov=nesterov, first=first)
        want = [el.ref_sgd(p, g, m, first, momentum, nesterov) for p, g, m in zip(p0, r.grads, bufs)]
        bufs = [w[1] for w in want]
        tag = f"first={first} ({label})"
        checks += s.flat_checks(o.grad, r.grads, f"grad {tag}")
        checks += s.flat_checks(s.p.clone(), [w[0] for w in want], f"p {tag}")
        if momentum:
            checks += s.flat_checks(mom.clone(), bufs, f"mom {tag}")
        else:
            checks.append(lambda: _all_nan_bits(mom, f"momentum 0: mom {tag}"))
        checks += _forward_checks(o, r, tag)
        losses.append(o.loss)
    checks.append(lambda: _exact(s.loss_sum, losses[0] + losses[1], "loss_sum after two calls"))
    _collect(checks)


# ------------------------------------------------------------------ device cursor
@pytest.mark.parametrize("xdtype", XDTYPES, ids=dtid)
def test_step_device_cursor(dev, xdtype):
    """An 11-row dataset, B = 4, three batches in sidx: a permutation with a repeated row, -3
    (clamped to row 0) and nrows + 5 (clamped to row 10).  Every sample's record, slab row and
    row loss are those of the row the clamp selects, labels read at the same row; the cursor
    goes 0 -> 1 -> 2 -> 0."""
    c = el.case(el.CURSOR_ROWS)
    s = Step(dev, c.x, c.labels, c.W, xdtype, B=el.CURSOR_B, sidx=el.CURSOR_SIDX)
    checks = []
    for k in range(3):
        r = el.step_refs(("cursor", k))
        assert int(s.cursor) == k
        o = s.call()
        label = f"batch {k}, rows {el.clamped_rows(k)}, {dtid(xdtype)}"
        checks += _forward_checks(o, r, label) + _seed_checks(o, r, label) + _slab_checks(o, r, label)
        checks += s.flat_checks(o.grad, r.grads, f"grad ({label})")
    assert int(s.cursor) == 0, "the cursor wraps after the last batch"
    _collect(checks)


# ------------------------------------------------------------------ labels outside [0, 10)
@pytest.mark.parametrize("xdtype", XDTYPES, ids=dtid)
def test_step_ignores_labels_outside_the_classes(dev, xdtype):
    """Labels -1, -100, 10, 63, 67 and 2^40 + 3 among valid rows: csrc/loss.hip's contract.  Each
    such row has loss 0 and an all-zero dl and contributes nothing to any gradient, the mean
    still divides by B; the valid rows' results are those of the all-valid batch, bit for bit.
    The same batch through the layer-wise model and dmlab.nn.cross_entropy is the second
    witness: the same logits, loss and gradients."""
    lc = el.label_case()
    s, r = _step(dev, ("labels", 8), xdtype)
    o = s.call()
    label = f"invalid labels, {dtid(xdtype)}"
    bad = list(lc.invalid)
    zero = lambda t, what: (lambda: _exact(t, torch.zeros(t.shape, dtype=F64), f"{what} of the ignored rows"))
    _collect([zero(o.rowloss[bad], "rowloss"), zero(o.rec[bad][:, el.R_DL], "dl"),
              zero(o.rec[bad][:, el.R_DH1], "dh1"), zero(o.cslab[bad], "the slab rows")]
             + _forward_checks(o, r, label) + _seed_checks(o, r, label) + _slab_checks(o, r, label)
             + s.flat_checks(o.grad, r.grads, f"grad ({label})"))
    # the valid rows against the all-valid batch of the same images
    full = el.step_refs(("B", 8))
    ok = [b for b in range(8) if b not in bad]
    _exact(o.rec[ok][:, :el.REC_USED], full.rec[ok], "the valid rows' records")
    _exact(o.cslab[ok], full.cslab[ok], "the valid rows' slab rows")

    if xdtype != F32:
        return  # the layer-wise model rounds its activations to the input type
    from dmlab.models import Net
    from dmlab.nn import cross_entropy

    net = Net().to(dev)
    params = dict(c1w=net.conv1.weight, c1b=net.conv1.bias, c2w=net.conv2.weight, c2b=net.conv2.bias,
                  f1w=net.fc1.weight, f1b=net.fc1.bias, f2w=net.fc2.weight, f2b=net.fc2.bias)
    with torch.no_grad():
        for k, p in params.items():
            p.copy_(getattr(lc.W, k).to(dev))
    out = net(lc.x.to(dev))
    loss = cross_entropy(out, lc.labels.to(dev))
    loss.backward()
    _collect([lambda: _exact(out.detach().float(), r.lg, "layer-wise logits"),
              lambda: _within(loss.detach().float().view(1), r.loss.view(1),
                              torch.tensor([r.loss_bound], dtype=F64), "layer-wise loss")]
             + [lambda k=k, g=g: _exact(params[k].grad.flatten(), g, f"layer-wise gradient {k}")
                for k, g in zip(el.SEG_KEYS, r.grads)])


# ------------------------------------------------------------------ Tier B: odd batches
@pytest.mark.parametrize("xdtype", XDTYPES, ids=dtid)
@pytest.mark.parametrize("B", el.ODD_B)
def test_step_odd_batch(dev, B, xdtype):
    """B = 3 and 7: fl(1 / B) is not dyadic.  The forward record, rowloss and dl (a power-of-two
    multiple of fl(1 / B)) are still exact.  The gradient kernel is given what the sample kernel
    wrote: flat.grad against the float64 reduction of the kernel's own rec and cslab within
    (B / 2 + 2) 2^-24 sum_b |term_b| per element (the two-lane split bh = (B + 1) >> 1: a dropped
    or doubled sample misses by four orders of magnitude, asserted on the CPU).  dh1 and the slab
    against the whole-step float64 reference within the chain bound of exact_lenet.py."""
    s, r = _step(dev, ("B", B), xdtype)
    o = s.call()
    label = f"B {B}, {dtid(xdtype)}"
    _collect(_forward_checks(o, r, label) + [lambda: _exact(o.rec[:, el.R_DL], r.dl, f"dl ({label})")])
    bd, bs = el.chain_bound(r)
    _note(f"sample kernel dh1, B {B}", _within(o.rec[:, el.R_DH1], r.dh1, bd, f"dh1 ({label})"))
    _note(f"sample kernel slab, B {B}", _within(o.cslab, r.cslab, bs, f"slab ({label})"))
    g, a = el.reduce_records(o.rec.cpu(), o.cslab.cpu())
    _all_nan_bits(o.grad[s.gap], f"grad: the gaps ({label})")
    worst = 0.0
    for nm, off, n, want, terms in zip(el.SEG_NAMES, s.off, el.SEG_N, g, a):
        worst = max(worst, _within(o.grad[off:off + n], want, el.odd_batch_bound(B, terms), f"grad {nm} ({label})"))
    _note(f"gradient kernel, B {B}", worst)


# ------------------------------------------------------------------ csrc/optim.hip
def _vec(b, n, offset, what, dtype=F32):
    """An n-vector starting `offset` elements into its guarded, NaN-prefilled storage."""
    store = b.out((n + offset,), dtype, what, keep=True)
    return store, store[offset:]


@pytest.mark.parametrize("momentum,nesterov", el.SGD_VARIANTS)
@pytest.mark.parametrize("n", el.OPT_N)
def test_sgd_step_exact(dev, n, momentum, nesterov):
    """sgd_step on dyadic data with dampening, wd and gscale, three launches (first, then two
    more), with and without the bf16 shadow, on 16-byte aligned buffers (float4 body + scalar
    tail) and on views starting one element into their storage (the all-scalar n4 = 0 path): p
    and the buffer equal float64 bit for bit, pbf is the float64 p rounded once to nearest-even
    (bf16 ties planted in both directions), the element before each view keeps its prefill."""
    c, refs, h = el.sgd_case(n), el.sgd_refs(n, momentum, nesterov), el.HYPER
    checks = []
    for offset in (0, 1):
        for shadow in (False, True):
            b = Bench(dev)
            (ps, p), (gs, g), (ms, mom) = (_vec(b, n, offset, w) for w in ("p", "g", "mom"))
            pbf = b.out((n,), BF, "pbf", keep=True) if shadow else None
            assert (p.data_ptr() % 16 == 0) == (offset == 0)
            for k, (pn, bv, _) in enumerate(refs):
                p.copy_(c.p[k])
                g.copy_(c.g[k])
                lib().sgd_step(p, g, mom if momentum else None, pbf, h["lr"], momentum, h["dampening"],
                               h["wd"], h["gscale"], nesterov, k == 0)
                b.done()
                tag = f"launch {k}, n {n}, offset {offset}, shadow {shadow}"
                checks.append(lambda t=p.clone(), w=pn, tag=tag: _exact(t, w, f"p ({tag})"))
                checks.append(lambda t=g.clone(), w=c.g[k].double(), tag=tag: _exact(t, w, f"g untouched ({tag})"))
                if momentum:
                    checks.append(lambda t=mom.clone(), w=bv, tag=tag: _exact(t, w, f"mom ({tag})"))
                else:
                    checks.append(lambda t=ms.clone(), tag=tag: _all_nan_bits(t, f"momentum 0: mom ({tag})"))
                if shadow:
                    checks.append(lambda t=pbf.clone(), w=pn.to(F32).to(BF), tag=tag: _bf16_bits(t, w, f"pbf ({tag})"))
                for st, what in ((ps, "p"), (gs, "g"), (ms, "mom")):
                    checks.append(lambda t=st[:offset].clone(), what=what, tag=tag:
                                  _all_nan_bits(t, f"the element before {what} ({tag})"))
    _collect(checks)


@pytest.mark.parametrize("n", el.OPT_N)
def test_cast_f32_bf16_exact(dev, n):
    """Round to nearest-even, ties in both directions, both zeros with their signs."""
    b, x = Bench(dev), el.cast_case(n)
    xd, y = b.inp(x, F32, "x"), b.out((n,), BF, "y")
    lib().cast_f32_bf16(xd, y)
    b.done()
    _bf16_bits(y, x.to(BF), f"cast, n {n}")


@pytest.mark.parametrize("rows", el.ROWS)
def test_rows_mean_exact(dev, rows):
    """out = scale * sum_r x[r] on integer rows with a power-of-two scale, every n."""
    for n in el.OPT_N:
        b = Bench(dev)
        x, scale = el.rows_case(rows, n)
        xd, out = b.inp(x, F32, "x"), b.out((n,), F32, "out")
        lib().rows_mean(xd, out, scale)
        b.done()
        _exact(out, x.double().sum(0) * scale, f"rows_mean, rows {rows}, n {n}")


@pytest.mark.parametrize("bias_correction", [False, True])
@pytest.mark.parametrize("n", el.ADAM_N)
def test_adam_step_within_derived_bound(dev, n, bias_correction):
    """adam_step with wd, gscale and the bf16 shadow on Gaussian data, two launches: p, m and v
    against the float64 expression on the launch's own fp32 inputs within one ulp per fp32
    operation (exact_lenet.ref_adam); pbf is the nearest-even rounding of the kernel's p."""
    c, h, b = el.adam_case(n), el.ADAM, Bench(dev)
    p, m, v = (b.inp(t, F32, w) for t, w in ((c.p, "p"), (c.m, "m"), (c.v, "v")))
    pbf = b.out((n,), BF, "pbf", keep=True)
    worst = 0.0
    for t in (1, 2):
        g = b.inp(c.g[t - 1], F32, "g")
        bc1, bc2 = el.adam_bias_corrections(t, bias_correction)
        before = [x.cpu().clone() for x in (p, g, m, v)]
        lib().adam_step(p, g, m, v, pbf, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["gscale"], bc1, bc2)
        b.done()
        want, bound = el.ref_adam(*before, bc1, bc2)
        for got, w, e, nm in zip((p, m, v), want, bound, "pmv"):
            worst = max(worst, _within(got, w, e, f"adam {nm}, launch {t}, n {n}"))
        _bf16_bits(pbf, p.cpu().to(BF), f"adam pbf, launch {t}, n {n}")
        _exact(g, c.g[t - 1].double(), "g untouched")
    _note(f"adam_step, n {n}, bias correction {bias_correction}", worst)
