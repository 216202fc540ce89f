"""Element-exact references for the ResNet conv kernel family.

Small-integer operands make every bf16 x bf16 product and every fp32 partial sum exactly
representable, so the result of a convolution is independent of the accumulation order (MFMA
order, split-K slabs, fixed-order reduces) and must equal a float64 reference bit for bit.
This module draws such operands (int_case), computes the float64 references from explicit tap
loops (ref_*; never a library convolution), asserts the conditions under which exactness
holds (exact_preconditions), allocates guarded tensors (guarded) and compares element by
element (assert_exact).  It never calls the code under test."""
import functools
import math
from types import SimpleNamespace

import torch

LIM_BF16 = 256  # integers up to 2^8 are exact in bf16 (8 significand bits)
LIM_FP32 = 1 << 24  # integers up to 2^24 are exact in fp32

# ------------------------------------------------------------------ the cases
# (N, H, W, Cin, Cout, k, stride, pad)
GEOMS_SMALL = [  # non-square, less than one tile; blocks crossing images, partial last tile
    (2, 5, 11, 64, 64, 3, 1, 1),
    (2, 11, 5, 64, 64, 3, 1, 1),
    (5, 7, 6, 128, 64, 3, 1, 1),
]
# short images at the width limits: W = 56 the halo LDS limit with equality, 57 falls back;
# 60 / 61 the wgrad cfg 8 limit; 63 / 64 the cfg 80 and wgrad cfg 4/5 limits
GEOMS_WIDTH = [(2, 3, W, 64, 64, 3, 1, 1) for W in (56, 57, 60, 61, 63, 64)]
GEOMS_CHUNKS = [  # several channel chunks and column tiles
    (2, 7, 10, 128, 128, 3, 1, 1),
    (2, 6, 9, 256, 256, 3, 1, 1),
    (2, 4, 6, 512, 512, 3, 1, 1),
]
GEOMS_1X1 = [(2, 5, 9, 64, 256, 1, 1, 0), (1, 3, 5, 2048, 256, 1, 1, 0)]  # 1 and 32 K-steps
GEOMS_S2 = [  # stride 2 with mixed parity-class sizes
    (2, 9, 14, 64, 128, 3, 2, 1),
    (2, 14, 9, 64, 128, 3, 2, 1),
    (2, 9, 14, 64, 128, 1, 2, 0),
    (2, 10, 6, 128, 256, 3, 2, 1),
]
GEOMS_TINY = [  # layers 3-4 of the model at a 32-pixel input
    (4, 1, 1, 512, 512, 3, 1, 1),
    (3, 2, 2, 256, 512, 3, 2, 1),
    (3, 2, 3, 256, 256, 3, 1, 1),
]
GEOMS_S1 = GEOMS_SMALL + GEOMS_WIDTH + GEOMS_CHUNKS + GEOMS_1X1 + [GEOMS_TINY[0], GEOMS_TINY[2]]
GEOMS_STRIDE2 = GEOMS_S2 + [GEOMS_TINY[1]]
GEOMS = GEOMS_S1 + GEOMS_STRIDE2
# stride-2 weight gradient over the parity planes (wgrad cfg 7): even H and W, non-square,
# Wg = 31 the widest supported, Wg = 32 one past it (falls back)
GEOMS_WGRAD_S2 = [(1, 4, 62, 64, 128, 3, 2, 1), (1, 4, 64, 64, 128, 3, 2, 1)]
STEM_GEOM = (2, 16, 24, 3, 64, 7, 2, 3)
ALL_GEOMS = GEOMS + GEOMS_WGRAD_S2 + [STEM_GEOM]


def geom_id(g):
    return "n%d_%dx%d_c%d-%d_k%ds%dp%d" % tuple(g)


def out_hw(geom):
    N, H, W, Cin, Cout, k, s, p = geom
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def has_projection(geom):
    """The geometries that take the merged 1x1/s2 projection (a 3x3/s2/p1 conv)."""
    return geom[5:] == (3, 2, 1)


# ------------------------------------------------------------------ operands
def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _choice(g, values, shape):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _sparse_weights(g, cout, cin, k):
    """Exactly min(K, 48) entries of +-1 per output channel, zeros elsewhere."""
    K = cin * k * k
    nz = min(K, 48)
    pos = torch.rand(cout, K, generator=g).argsort(1)[:, :nz]
    sign = _choice(g, [-1.0, 1.0], (cout, nz))
    w = torch.zeros(cout, K)
    w.scatter_(1, pos, sign)
    return w.view(cout, cin, k, k)


@functools.lru_cache(maxsize=None)
def int_case(geom, seed=0):
    """Integer-valued operands of one conv geometry, drawn on the CPU (activations NHWC,
    weights OIHW, all fp32 holding small integers; the tensors are shared: do not modify)."""
    N, H, W, Cin, Cout, k, s, p = geom
    OH, OW = out_hw(geom)
    g = torch.Generator().manual_seed(1000 * seed + 17)
    c = SimpleNamespace(geom=geom, seed=seed)
    c.x = _randint(g, -2, 2, (N, H, W, Cin))
    c.w = _sparse_weights(g, Cout, Cin, k)
    c.dy = _randint(g, -2, 2, (N, OH, OW, Cout))
    c.add_y = _randint(g, -4, 4, (N, OH, OW, Cout))
    c.add_x = _randint(g, -4, 4, (N, H, W, Cin))
    c.keep_add = torch.rand(N, H, W, Cin, generator=g) > 0.4
    c.pre_scale = _choice(g, [1.0, 2.0], (Cin,))
    c.pre_shift = _randint(g, -2, 2, (Cin,))
    c.red_y = _randint(g, -3, 3, (N, H, W, Cin))
    c.red_scale = _choice(g, [1.0, 2.0], (Cin,))
    c.red_shift = _randint(g, -2, 2, (Cin,))
    c.red_mean = _randint(g, -1, 1, (Cin,))
    c.red_invstd = _choice(g, [0.5, 1.0, 2.0], (Cin,))
    c.red_keep = torch.rand(N, H, W, Cin, generator=g) > 0.5
    c.dw_base = _randint(g, -4, 4, (Cout, Cin, k, k))
    if has_projection(geom):
        c.dy2 = _randint(g, -2, 2, (N, OH, OW, Cout))
        c.w2 = _sparse_weights(g, Cout, Cin, 1)
    return c


def pack_bits(keep):
    """1-bit mask layout of the kernels: bit j of byte i = element 8i + j (NHWC order)."""
    b = keep.reshape(-1, 8).to(torch.uint8) << torch.arange(8, device=keep.device, dtype=torch.uint8)
    return b.sum(1, dtype=torch.uint8)


# ------------------------------------------------------------------ float64 references
def pre_bn(x, scale, shift):
    """relu(x * scale + shift) per channel (NHWC), float64."""
    return torch.relu(x.double() * scale.double() + shift.double())


def _pad_hw(a, p):
    return torch.nn.functional.pad(a, (0, 0, p, p, p, p))


def _taps(geom):
    N, H, W, Cin, Cout, k, s, p = geom
    OH, OW = out_hw(geom)
    for kh in range(k):
        for kw in range(k):
            yield kh, kw, slice(kh, kh + s * (OH - 1) + 1, s), slice(kw, kw + s * (OW - 1) + 1, s)


def ref_fwd(geom, x, w, add=None, pre=None):
    """y[n, oy, ox, co] = sum_{kh, kw, ci} a[n, oy*s - p + kh, ox*s - p + kw, ci] * w[co, ci, kh, kw]
    (+ add), a = x or relu(x*sc + sh); zero padding is applied after the pre-BN."""
    N, H, W, Cin, Cout, k, s, p = geom
    OH, OW = out_hw(geom)
    a = x.double() if pre is None else pre_bn(x, *pre)
    ap = _pad_hw(a, p)
    wd = w.double()
    y = torch.zeros(N, OH, OW, Cout, dtype=torch.float64)
    for kh, kw, ys, xs in _taps(geom):
        y += ap[:, ys, xs, :] @ wd[:, :, kh, kw].t()
    if add is not None:
        y = y + add.double()
    return y


def ref_dgrad(geom, dy, w, add=None, keep=None, dy2=None, w2=None):
    """dx = the transpose of ref_fwd applied to dy (+ add, or add where keep; + the 1x1/s2/p0
    projection's data gradient of dy2 through w2 at the even pixels)."""
    N, H, W, Cin, Cout, k, s, p = geom
    dxp = torch.zeros(N, H + 2 * p, W + 2 * p, Cin, dtype=torch.float64)
    d, wd = dy.double(), w.double()
    for kh, kw, ys, xs in _taps(geom):
        dxp[:, ys, xs, :] += d @ wd[:, :, kh, kw]
    dx = dxp[:, p:p + H, p:p + W, :].clone()
    if dy2 is not None:
        assert s == 2
        dx[:, ::2, ::2, :] += dy2.double() @ w2.double()[:, :, 0, 0]
    if add is not None:
        a = add.double()
        dx += a if keep is None else a * keep
    return dx


def ref_wgrad(geom, x, dy, base=None, pre=None, absolute=False):
    """dw[co, ci, kh, kw] = sum_{n, oy, ox} dy[n, oy, ox, co] * a[n, oy*s - p + kh, ox*s - p + kw, ci]
    (+ base); absolute: the sum of the terms' absolute values instead."""
    N, H, W, Cin, Cout, k, s, p = geom
    a = x.double() if pre is None else pre_bn(x, *pre)
    d = dy.double()
    if absolute:
        a, d = a.abs(), d.abs()
    ap = _pad_hw(a, p)
    dm = d.reshape(-1, Cout).t()
    dw = torch.zeros(Cout, Cin, k, k, dtype=torch.float64)
    for kh, kw, ys, xs in _taps(geom):
        dw[:, :, kh, kw] = dm @ ap[:, ys, xs, :].reshape(-1, Cin)
    if base is not None:
        dw += base.double().abs() if absolute else base.double()
    return dw


def ref_stats(y):
    """Per-channel sum and sum of squares of an NHWC tensor -> [2][C]."""
    y = y.double()
    return torch.stack([y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))])


def ref_bn_reduce(dx, keep, y, mean, invstd, absolute=False):
    """The BN-backward sums of dz = dx where keep: [sum dz, sum dz * (y - mean) * invstd]."""
    dz = dx.double() * keep
    t = dz * (y.double() - mean.double())
    if absolute:
        dz, t = dz.abs(), t.abs()
    return torch.stack([dz.sum((0, 1, 2)), t.sum((0, 1, 2)) * invstd.double()])


def relu_keep(case):
    """The ReLU mask the kernels derive from red_y: y * scale + shift > 0."""
    return case.red_y.double() * case.red_scale.double() + case.red_shift.double() > 0


@functools.lru_cache(maxsize=None)
def case_refs(geom, seed=0):
    """Every float64 reference the tests of one geometry compare against, computed once."""
    c = int_case(geom, seed)
    N, H, W, Cin, Cout, k, s, p = geom
    r = SimpleNamespace()
    pre = (c.pre_scale, c.pre_shift)
    r.y = ref_fwd(geom, c.x, c.w)
    r.y_add = r.y + c.add_y.double()
    r.y_pre = ref_fwd(geom, c.x, c.w, pre=pre)
    r.y_pre_add = r.y_pre + c.add_y.double()
    r.stats = ref_stats(r.y)  # the kernels' statistics are those of the conv, before the add
    r.stats_pre = ref_stats(r.y_pre)
    r.dx = ref_dgrad(geom, c.dy, c.w)
    r.dx_acc = ref_dgrad(geom, c.dy, c.w, add=c.add_x)
    r.dx_masked = ref_dgrad(geom, c.dy, c.w, add=c.add_x, keep=c.keep_add)
    r.dw = ref_wgrad(geom, c.x, c.dy)
    r.dw_base = ref_wgrad(geom, c.x, c.dy, base=c.dw_base)
    r.dw_pre = ref_wgrad(geom, c.x, c.dy, pre=pre)
    r.dw_pre_base = ref_wgrad(geom, c.x, c.dy, base=c.dw_base, pre=pre)
    ry = relu_keep(c)
    red = lambda dx, keep, **kw: ref_bn_reduce(dx, keep, c.red_y, c.red_mean, c.red_invstd, **kw)
    r.red = {("dx", "y"): red(r.dx, ry), ("dx", "bits"): red(r.dx, c.red_keep),
             ("dx_masked", "y"): red(r.dx_masked, ry), ("dx_masked", "bits"): red(r.dx_masked, c.red_keep)}
    if has_projection(geom):
        r.dx_merged = ref_dgrad(geom, c.dy, c.w, dy2=c.dy2, w2=c.w2)
        r.red[("dx_merged", "y")] = red(r.dx_merged, ry)
        r.red[("dx_merged", "bits")] = red(r.dx_merged, c.red_keep)
    return r


# ------------------------------------------------------------------ preconditions
def _need_bf16_exact(name, v):
    assert torch.equal(v, v.round()), f"{name}: not integer-valued"
    m = float(v.abs().max())
    assert m <= LIM_BF16, f"{name}: max |v| = {m} > {LIM_BF16} is not exact in bf16"
    return m


def _need_fp32_exact(name, v, abs_terms):
    assert torch.equal(v * 2, (v * 2).round()), f"{name}: not a multiple of 1/2"
    m, a = float(v.abs().max()), float(abs_terms.max())
    assert m < LIM_FP32, f"{name}: max |v| = {m} >= 2^24"
    assert a < LIM_FP32, f"{name}: sum of |terms| = {a} >= 2^24"
    assert a >= m
    return a


def exact_preconditions(case):
    """Conditions (on the float64 references) under which every kernel result is exact in any
    accumulation order: bf16 results are integers of magnitude <= 256, fp32 results and the
    sums of their terms' absolute values stay below 2^24.  Returns the maxima found."""
    c, geom = case, case.geom
    r = case_refs(geom, case.seed)
    pre = (c.pre_scale, c.pre_shift)
    seen = {}
    # the operands themselves are stored as bf16
    for n in ("x", "w", "dy", "add_y", "add_x", "red_y", "dw_base"):
        _need_bf16_exact(n, getattr(c, n))
    _need_bf16_exact("pre-BN operand", pre_bn(c.x, *pre))
    # bf16 outputs; their fp32 accumulators hold partial sums bounded by the sum of |terms|
    for n in ("y", "y_add", "y_pre", "y_pre_add"):
        seen[n] = _need_bf16_exact(n, getattr(r, n))
    a = ref_fwd(geom, c.x.abs(), c.w.abs(), add=c.add_y.abs(), pre=None)
    ap = ref_fwd(geom, pre_bn(c.x, *pre), c.w.abs(), add=c.add_y.abs())
    assert float(a.max()) < LIM_FP32 and float(ap.max()) < LIM_FP32
    names = ["dx", "dx_acc", "dx_masked"] + (["dx_merged"] if has_projection(geom) else [])
    for n in names:
        seen[n] = _need_bf16_exact(n, getattr(r, n))
    kw = dict(dy2=c.dy2.abs(), w2=c.w2.abs()) if has_projection(geom) else {}
    a = ref_dgrad(geom, c.dy.abs(), c.w.abs(), add=c.add_x.abs(), **kw)
    assert float(a.max()) < LIM_FP32
    # fp32 results: statistics (sum |y| <= sum y^2 for integers), BN-reduce sums, weight gradients
    for n, y in (("stats", r.y), ("stats_pre", r.y_pre)):
        s = getattr(r, n)
        seen[n] = _need_fp32_exact(n, s, torch.stack([y.abs().sum((0, 1, 2)), s[1]]))
    ry = relu_keep(c)
    for (dn, src), want in r.red.items():
        keep = ry if src == "y" else c.red_keep
        at = ref_bn_reduce(getattr(r, dn), keep, c.red_y, c.red_mean, c.red_invstd, absolute=True)
        # the kernels scale the finished sum by invstd: bound the unscaled sum as well
        at = torch.maximum(at, at / c.red_invstd.double())
        seen[f"red_{dn}_{src}"] = _need_fp32_exact(f"red {dn} {src}", want, at)
    for n, p_, b in (("dw", None, None), ("dw_base", None, c.dw_base), ("dw_pre", pre, None),
                     ("dw_pre_base", pre, c.dw_base)):
        at = ref_wgrad(geom, c.x, c.dy, base=b, pre=p_, absolute=True)
        seen[n] = _need_fp32_exact(n, getattr(r, n), at)
    return seen


# ------------------------------------------------------------------ guarded tensors
GUARD = 4096  # guard elements on each side
_PATTERN = {"out": 0xA5, "in": 0xFF}


def guarded(shape, dtype, dev, fill):
    """A contiguous, 16-byte-aligned tensor of `shape` inside a larger allocation with at
    least GUARD elements of guard on each side, and a checker of the guards.

    fill == "out": the tensor is all NaN (0xFF bytes) and the guards hold the byte 0xA5, so
      after the call under test an exact compare proves every element was written and
      check() proves nothing outside was.
    fill == "in": the guards are 0xFF bytes (NaN in bf16 / fp32, all-ones in a bit mask) and the
      caller copies the operand in: an out-of-tensor read that reaches a MAC poisons the output.
    check(what) asserts both guards are bit-identical to their fill."""
    item = torch.empty((), dtype=dtype).element_size()
    body = math.prod(shape) * item
    g = GUARD * item
    assert g % 16 == 0
    tail = g + (-body) % 16
    raw = torch.empty(g + body + tail, dtype=torch.uint8, device=dev)
    pat = _PATTERN[fill]
    raw.fill_(pat)
    raw[g:g + body].fill_(0xFF)
    view = raw[g:g + body].view(dtype).view(shape)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()

    def check(what="tensor"):
        for side, part, off in (("below", raw[:g], -g), ("above", raw[g + body:], body)):
            bad = (part != pat).nonzero()
            if bad.numel():
                first = int(bad[0]) + off
                raise AssertionError(
                    f"{what}: {bad.numel()} guard bytes {side} the tensor were overwritten; "
                    f"first at byte offset {first} from its start (element {first // item})")

    return view, check


# ------------------------------------------------------------------ exact compare
_AXES = {4: {"nyxc": ("n", "y", "x", "c"), "oikk": ("co", "ci", "kh", "kw")}}


def assert_exact(got, want, what, layout="nyxc"):
    """torch.equal on the float64 casts; on failure the mismatch count, the first 8 coordinates
    with got / want, and the affected indices per axis (so a wrong tap or tile edge shows)."""
    g = got.detach().double().cpu()
    w = want.detach().double().cpu()
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}"
    if torch.equal(g, w):
        return
    axes = _AXES.get(g.dim(), {}).get(layout) or tuple(f"d{i}" for i in range(g.dim()))
    bad = (g != w).nonzero()
    lines = [f"{what}: {bad.shape[0]} of {g.numel()} elements differ "
             f"({int(torch.isnan(g).sum())} NaN = never written or poisoned)"]
    for idx in bad[:8].tolist():
        at = ", ".join(f"{a}={i}" for a, i in zip(axes, idx))
        lines.append(f"  ({at}): got {g[tuple(idx)].item()} want {w[tuple(idx)].item()}")
    for d, a in enumerate(axes):
        u = bad[:, d].unique().tolist()
        txt = str(u) if len(u) <= 16 else f"{u[:8]} ... {u[-4:]} ({len(u)} values)"
        lines.append(f"  affected {a} ({len(u)} of {g.shape[d]}): {txt}")
    raise AssertionError("\n".join(lines))
