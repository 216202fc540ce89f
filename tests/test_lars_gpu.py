"""The fused LARS step (csrc/lars.hip) on the GPU against the float64 loop of
tests/lars_reference.py: chunk-boundary sizes, padding, determinism, clipping, a captured
step that follows a schedule, and ResNet-18's real parameter layout.

Bounds.  Update and momentum buffer: relative L2 error <= 1e-4 per tensor (an fp32 emulation
of test 1 with chunked fp32 sums gives at most 7.2e-6; the rest is room for FMA contraction
and summation order).  With lr*eta = 0.05 the update is ~5 % of the weights, so the bound
constrains the trust ratio.  Norms: rtol 1e-5, above the fp32 summation-error bound
(log2 n + 16) * 2^-24 ~ 2.4e-6 for these lengths; the trust ratio is a quotient of two such
norms (<= 2 * 2.4e-6 plus a few roundings), so it takes the same rtol.

Measured on an MI355X (largest over tensors and steps): update 4.3e-6 and buffer 4.9e-7 in
test 1, 5.0e-6 / 1.8e-7 with clipping, 9.5e-6 / 1.6e-7 on ResNet-18; G within 8.6e-8.
"""
import pytest
import torch

from lars_reference import lars_ref_step, rel_l2

pytestmark = pytest.mark.gpu

HP = dict(lr=1.0, eta=0.05, wd=1e-2, mu=0.9, grad_scale=0.5)
ZERO_GRAD, ZERO_W = 2, 4  # tensors (sizes 63 and 65) with an all-zero gradient / all-zero weights


def _sizes():
    from dmlab.ops._native import lib

    C = lib().lars_chunk()
    assert C % 4 == 0
    # 300C+17: more chunks than a workgroup has threads
    return [1, 7, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5, 300 * C + 17], [512, 512]


def _layout(dev, seed=0):
    """A FlatParams of 2-D (adapted) tensors of the sizes above plus two 1-D ones."""
    from dmlab.nn.flat import FlatParams

    two_d, one_d = _sizes()
    g = torch.Generator().manual_seed(seed)
    named = []
    for i, n in enumerate(two_d):
        w = torch.randn(1, n, generator=g) * 0.05
        if i == ZERO_W:
            w.zero_()
        named.append((f"t{i}", torch.nn.Parameter(w.to(dev))))
    for j, n in enumerate(one_d):
        named.append((f"v{j}", torch.nn.Parameter((torch.randn(n, generator=g) * 0.05).to(dev))))
    flat = FlatParams(named, dev)
    pad = torch.ones(flat.numel, dtype=torch.bool)
    for p, o in zip(flat.params, flat.offsets):
        pad[o:o + p.numel()] = False
    assert bool(pad.any())
    return flat, pad.to(dev)


def _fresh_grad(flat, seed):
    """A whole gradient buffer: N(0, 2^2) inside the tensors, NaN in every padding element."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = torch.full((flat.numel,), float("nan"))
    for i, (p, o) in enumerate(zip(flat.params, flat.offsets)):
        out[o:o + p.numel()] = 0.0 if i == ZERO_GRAD else torch.randn(p.numel(), generator=g) * 2
    return out.to(flat.device)


def _make_opt(flat, nesterov=False, max_grad_norm=None, lr=HP["lr"]):
    from dmlab.optim import LARS

    opt = LARS(flat.params, lr=lr, momentum=HP["mu"], weight_decay=HP["wd"],
               trust_coefficient=HP["eta"], nesterov=nesterov, max_grad_norm=max_grad_norm)
    opt.grad_scale = HP["grad_scale"]
    assert opt.flat is flat and opt._native()
    return opt


def _views(flat, buf):
    return [buf[o:o + p.numel()] for p, o in zip(flat.params, flat.offsets)]


def _step_and_check(flat, opt, pad, nesterov, max_grad_norm=None, lr=HP["lr"], tag=""):
    """One native step from the current state, checked against the float64 step from the
    same fp32 state.  Returns the reference's G."""
    adapted = [p.ndim > 1 for p in flat.params]
    w0 = [w.clone() for w in _views(flat, flat.data)]
    g0 = [g.clone() for g in _views(flat, flat.grad)]
    b0 = [b.clone() for b in _views(flat, opt.buf)]
    opt.step()
    rw, rb, rstats, rG = lars_ref_step(w0, g0, b0, adapted, lr=lr, eta=HP["eta"], wd=HP["wd"],
                                       mu=HP["mu"], grad_scale=opt.grad_scale,
                                       nesterov=nesterov, max_grad_norm=max_grad_norm)
    w1, b1 = _views(flat, flat.data), _views(flat, opt.buf)
    for i in range(len(w0)):
        dw = w1[i].double().cpu().reshape(-1) - w0[i].double().cpu().reshape(-1)
        e_w = rel_l2(dw, rw[i] - w0[i].double().cpu().reshape(-1))
        e_b = rel_l2(b1[i], rb[i])
        print(f"{tag} tensor {i} n={w0[i].numel()} rel err dw {e_w:.3e} buf {e_b:.3e}")
        assert e_w <= 1e-4 and e_b <= 1e-4, (tag, i, e_w, e_b)
    stats, gnorm = opt.stats()
    torch.testing.assert_close(stats.double().cpu(), rstats, rtol=1e-5, atol=0.0)
    for i, ad in enumerate(adapted):
        if not ad:  # plain momentum SGD without decay
            assert float(stats[i, 2]) == 1.0
    g_err = abs(float(gnorm) - rG) / rG
    print(f"{tag} G {float(gnorm):.6f} ref {rG:.6f} rel err {g_err:.3e}")
    assert g_err <= 1e-5
    assert bool((flat.data[pad] == 0).all()) and bool((opt.buf[pad] == 0).all())
    assert not bool(torch.isnan(flat.data).any()) and not bool(torch.isnan(opt.buf).any())
    return rG


@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_kernel_matches_float64(dev, nesterov):
    flat, pad = _layout(dev)
    opt = _make_opt(flat, nesterov)
    for step in range(3):
        flat.grad.copy_(_fresh_grad(flat, step))
        _step_and_check(flat, opt, pad, nesterov, tag=f"nesterov={nesterov} step {step}")
    # the zero-gradient tensor only decayed; the zero-weight one moved off zero
    assert float(_views(flat, flat.data)[ZERO_W].abs().sum()) > 0


def _run(dev, steps=3, lrs=None, **kw):
    flat, _ = _layout(dev)
    opt = _make_opt(flat, **kw)
    for step in range(steps):
        if lrs is not None:
            opt.lr = lrs[step]
        flat.grad.copy_(_fresh_grad(flat, step))
        opt.step()
    return flat.data.clone(), opt.buf.clone(), opt


def test_lars_is_deterministic(dev):
    w1, b1, _ = _run(dev)
    w2, b2, _ = _run(dev)
    assert torch.equal(w1, w2) and torch.equal(b1, b2)
    assert float(b1.abs().sum()) > 0


def test_lars_clipping(dev):
    flat, pad = _layout(dev)
    G = float((_fresh_grad(flat, 0).nan_to_num(0.0).double() * HP["grad_scale"]).norm())
    assert G > 100.0  # so max_grad_norm = 100 clips
    opt = _make_opt(flat, max_grad_norm=100.0)
    for step in range(2):
        flat.grad.copy_(_fresh_grad(flat, step))
        rG = _step_and_check(flat, opt, pad, False, max_grad_norm=100.0, tag=f"clip step {step}")
        assert rG > 100.0
    # a bound above G: c = 1 multiplies exactly
    w_free, b_free, _ = _run(dev)
    w_loose, b_loose, o = _run(dev, max_grad_norm=1e6)
    assert float(o.stats()[1]) < 1e6
    assert torch.equal(w_free, w_loose) and torch.equal(b_free, b_loose)


def test_lars_captured_step_follows_the_schedule(dev):
    lrs = [1.0, 0.5, 0.25]
    w_eager, b_eager, _ = _run(dev, lrs=lrs)
    flat, _ = _layout(dev)
    opt = _make_opt(flat)
    w_saved, b_saved = flat.data.clone(), opt.buf.clone()
    flat.grad.copy_(_fresh_grad(flat, 0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()  # eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        opt.step()
    flat.data.copy_(w_saved)
    opt.buf.copy_(b_saved)
    for step, lr in enumerate(lrs):
        opt.lr = lr
        flat.grad.copy_(_fresh_grad(flat, step))
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(flat.data, w_eager) and torch.equal(opt.buf, b_eager)


def test_lars_resnet18_step(dev):
    from dmlab.models import ResNet18
    from dmlab.nn import cross_entropy
    from dmlab.optim import LARS

    torch.manual_seed(0)
    model = ResNet18(num_classes=10).to(dev)
    opt = LARS(model.parameters(), lr=1.0, trust_coefficient=0.05, weight_decay=1e-2)
    assert opt.flat is model.flat and opt._native()
    x = torch.rand(8, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (8,), device=dev)
    loss = cross_entropy(model(x), y)
    opt.zero_grad()
    loss.backward()
    flat = model.flat
    adapted = [p.ndim > 1 for p in flat.params]
    w0 = [w.clone() for w in _views(flat, flat.data)]
    g0 = [g.clone() for g in _views(flat, flat.grad)]
    named = {n: (p.detach().clone(), p.grad.detach().clone()) for n, p in model.named_parameters()}
    opt.step()
    rw, rb, rstats, _ = lars_ref_step(w0, g0, [torch.zeros_like(w) for w in w0], adapted, lr=1.0,
                                      eta=0.05, wd=1e-2, mu=0.9)
    w1, b1 = _views(flat, flat.data), _views(flat, opt.buf)
    for i in range(len(w0)):
        w0d = w0[i].double().cpu()
        e_w = rel_l2(w1[i].double().cpu() - w0d, rw[i] - w0d)
        e_b = rel_l2(b1[i], rb[i])
        print(f"resnet18 tensor {i} n={w0[i].numel()} rel err dw {e_w:.3e} buf {e_b:.3e}")
        assert e_w <= 1e-4 and e_b <= 1e-4, (i, e_w, e_b)
    torch.testing.assert_close(opt.stats()[0].double().cpu(), rstats, rtol=1e-5, atol=0.0)
    excluded = 0
    for n, p in model.named_parameters():
        if n.endswith(("bn_weight", "bn_bias", "bias")):
            before, grad = named[n]
            assert torch.equal(p.detach(), before - 1.0 * grad), n
            excluded += 1
    assert excluded == 41
