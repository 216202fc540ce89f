"""The label-smoothed cross-entropy and evaluation-metric kernels (csrc/loss.hip) against
float64 torch references and the rank rule written out in torch; graph capture; and the
smoothed loss through the whole native ResNet-18 backward."""
import copy

import pytest
import torch
import torch.nn.functional as F

from dmlab.models import ResNet18
from dmlab.nn import EvalMetrics, count_correct, cross_entropy
from dmlab.ops._native import lib
from dmlab.utils.graph import CapturedStep
from loss_metrics_ref import (SHAPES, assert_mixed, planted_labels, ref_counts, ref_nll_sum)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _logits(dev, B, C, dtype, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed + 1000 * B + C)
    return (torch.randn(B, C, device=dev, generator=g) * 3).to(dtype)


def _state(m):
    return m.counts.clone(), m.loss_sum.clone()


# ------------------------------------------------------------------ smoothed cross-entropy
@pytest.mark.parametrize("eps", [0.1, 1.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", SHAPES)
def test_smoothed_cross_entropy_kernel(dev, dtype, B, C, eps):
    lib()  # fail loudly if the extension is missing
    x = _logits(dev, B, C, dtype).requires_grad_(True)
    y = torch.randint(0, C, (B,), device=dev)
    l1 = cross_entropy(x, y, label_smoothing=eps)
    l1.backward(torch.tensor(2.0, device=dev))
    xr = x.detach().double().requires_grad_(True)
    l2 = F.cross_entropy(xr, y, label_smoothing=eps)
    (2 * l2).backward()
    print(f"loss {l1.item():.7f} ref {l2.item():.7f} "
          f"max grad err {(x.grad.double() - xr.grad).abs().max().item():.3e}")
    torch.testing.assert_close(l1, l2.float(), rtol=1e-4, atol=1e-4)
    tol = 1e-6 if dtype == torch.float32 else 2e-3
    torch.testing.assert_close(x.grad.float(), xr.grad.float(), rtol=tol, atol=tol)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_smoothing_is_the_plain_path(dev, dtype):
    x = _logits(dev, 300, 1000, dtype)
    y = torch.randint(0, 1000, (300,), device=dev)
    out = []
    for kw in ({}, {"label_smoothing": 0.0}):
        xx = x.clone().requires_grad_(True)
        loss = cross_entropy(xx, y, **kw)
        loss.backward(torch.tensor(2.0, device=dev))
        out.append((loss.detach(), xx.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ------------------------------------------------------------------ metrics
def _ks(B, C):
    return [k for k in (1, 5, C, C + 3) if k != 1 or B >= 5]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", SHAPES)
def test_eval_metrics_kernel(dev, dtype, B, C):
    x = _logits(dev, B, C, dtype, seed=1)
    # one row cannot both hit and miss: B = 1 runs the two plantings (rank 0 and rank 5)
    for shift in ((0, 1) if B == 1 else (0,)):
        y = planted_labels(x, shift)
        ref_loss = ref_nll_sum(x, y).item() / B
        for k in _ks(B, C):
            if k < C and B >= 5:
                assert_mixed(x, y, k)  # on the reference, before the kernel is looked at
            want = ref_counts(x, y, k)
            r = EvalMetrics(k=k, device=dev).update(x, y).result()
            print(f"k={k} counts {[r['n'], r['top1'], r['topk']]} ref {want} "
                  f"loss {r['loss']:.7f} ref {ref_loss:.7f}")
            assert [r["n"], r["top1"], r["topk"]] == want
            assert abs(r["loss"] - ref_loss) <= 1e-4 + 1e-4 * abs(ref_loss)
            if k == 1:
                assert r["top1"] == r["topk"] == int(count_correct(x, y))
    if B == 1:
        hit = [EvalMetrics(k=5, device=dev).update(x, planted_labels(x, s)).result()["topk"]
               for s in (0, 1)]
        assert hit == [1, 0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", [(6, 65), (300, 1000)])
def test_eval_metrics_ties(dev, dtype, B, C):
    """Integer logits: every label sits inside a group of equal values, so the count of equal
    columns BEFORE the label decides the rank."""
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randint(-3, 4, (B, C), device=dev, generator=g).to(dtype)
    y = planted_labels(x, mult=2)
    same = x.float() == x.float().gather(1, y[:, None])
    assert bool((same.sum(1) >= 2).all())
    cols = torch.arange(C, device=dev)[None, :]
    assert bool((same & (cols < y[:, None])).any()) and bool((same & (cols > y[:, None])).any())
    for k in (1, 5, C, C + 3):
        if k < C:
            assert_mixed(x, y, k)
        r = EvalMetrics(k=k, device=dev).update(x, y).result()
        assert [r["n"], r["top1"], r["topk"]] == ref_counts(x, y, k)
        if k == 1:
            assert r["top1"] == int(count_correct(x, y))


def test_eval_metrics_label_guards(dev):
    """A label outside [0, C) is a miss with loss 0 (and is never used as an index); a NaN
    label logit is a miss; k >= C makes every other row a hit."""
    x = _logits(dev, 8, 10, torch.float32, seed=2)
    y = planted_labels(x)
    y[0], y[1] = -1, 10
    x[2, y[2]] = float("nan")
    r = EvalMetrics(k=13, device=dev).update(x, y).result()
    assert (r["n"], r["topk"]) == (8, 5)
    r = EvalMetrics(k=13, device=dev).update(x[:2], y[:2]).result()
    assert r == {"n": 2, "top1": 0, "topk": 0, "k": 13, "loss": 0.0}


def test_eval_metrics_deterministic_and_accumulating(dev):
    xs = [_logits(dev, B, 1000, torch.bfloat16, seed=s) for s, B in ((4, 300), (5, 300), (6, 5))]
    ys = [planted_labels(x) for x in xs]
    runs = []
    for _ in range(2):
        m = EvalMetrics(k=5, device=dev)
        for x, y in zip(xs, ys):
            m.update(x, y)
        runs.append(_state(m))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the B = 5 tail (one full 4-row block + one row) after full batches adds, not overwrites
    want = [sum(v) for v in zip(*(ref_counts(x, y, 5) for x, y in zip(xs, ys)))]
    assert runs[0][0].tolist() == want
    ref = sum(ref_nll_sum(x, y).item() for x, y in zip(xs, ys))
    assert abs(runs[0][1].item() - ref) <= 1e-4 * (605 + abs(ref))


# ------------------------------------------------------------------ capture
def test_loss_and_metrics_capture(dev):
    """One smoothed loss + backward and one EvalMetrics.update inside a hipGraph: the replay
    gives the bits of the eager calls."""
    B, C = 37, 1000
    xs = [_logits(dev, B, C, torch.bfloat16, seed=s) for s in (7, 8)]
    ys = [planted_labels(x, shift=s) for s, x in enumerate(xs)]
    up = torch.tensor(2.0, device=dev)
    m = EvalMetrics(k=5, device=dev)

    def step(met):
        def fn(x, y):
            xx = x.detach().requires_grad_(True)
            loss = cross_entropy(xx, y, label_smoothing=0.1)
            (grad,) = torch.autograd.grad(loss, xx, up)
            met.update(x, y)
            return loss.detach(), grad
        return fn

    cap = CapturedStep(step(m), [xs[0], ys[0]], warmup=2)
    m.reset()  # the warm-up calls counted; the graph keeps the state's pointers
    e = EvalMetrics(k=5, device=dev)
    eager = step(e)
    for x, y in zip(xs, ys):
        la, ga = (t.clone() for t in cap(x, y))
        lb, gb = eager(x, y)
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert torch.equal(m.counts, e.counts) and torch.equal(m.loss_sum, e.loss_sum)
    assert int(e.counts[0]) == 2 * B and 0 < int(e.counts[1]) < int(e.counts[2]) < 2 * B


# ------------------------------------------------------------------ model level
def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def test_resnet18_label_smoothing_matches_reference(dev):
    """tests/test_native_resnet_model.py::test_resnet18_native_matches_reference with
    label_smoothing=0.1 on every side: the smoothed seed flows through the whole native
    backward (native error <= 1.5 x autocast error + 0.05, per parameter)."""
    lib()
    torch.manual_seed(0)
    a = ResNet18(num_classes=10).to(dev)
    b = copy.deepcopy(a).set_backend("torch")
    b._flatten()
    c = copy.deepcopy(b)
    c._flatten()
    x = torch.rand(16, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (16,), device=dev)
    la = cross_entropy(a(x), y, label_smoothing=0.1)
    lb = F.cross_entropy(b(x), y, label_smoothing=0.1)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        oc = c(x)
    lc = F.cross_entropy(oc.float(), y, label_smoothing=0.1)
    for l in (la, lb, lc):
        l.backward()
    assert abs(la.item() - lb.item()) < 5e-2 * max(1.0, abs(lb.item()))
    bad = []
    for (n, pa), (_, pb), (_, pc) in zip(a.named_parameters(), b.named_parameters(),
                                         c.named_parameters()):
        rn, rc = _rel(pa.grad, pb.grad), _rel(pc.grad, pb.grad)
        if rn > 1.5 * rc + 0.05:
            bad.append((n, rn, rc))
    assert not bad, bad
    torch.testing.assert_close(a.stem.running_mean, b.stem.running_mean, rtol=2e-2, atol=2e-3)
