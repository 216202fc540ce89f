"""LARS and WarmupPolyLR on the CPU: the flat-buffer path (a Program), the per-tensor path
(a plain nn.Module), checkpoints, the schedule's closed form, gloo DDP and the task3 flags.
Every reference is the float64 loop of tests/lars_reference.py."""
import pytest
import torch
import torch.nn.functional as F

from dist_helpers import free_port, run_dist
from lars_reference import lars_ref_step

HP = dict(lr=0.5, eta=0.05, wd=1e-2, mu=0.9)


def _opt(params, exclude_1d=True, nesterov=False, max_grad_norm=None, lr=HP["lr"]):
    from dmlab.optim import LARS

    return LARS(params, lr=lr, momentum=HP["mu"], weight_decay=HP["wd"],
                trust_coefficient=HP["eta"], nesterov=nesterov, exclude_1d=exclude_1d,
                max_grad_norm=max_grad_norm)


def _lenet_batch(seed, n=6):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 1, 28, 28, generator=g), torch.randint(0, 10, (n,), generator=g)


def _bufs(opt):
    if opt.flat is None:
        return [b.clone() for b in opt.bufs]
    return [opt.buf[o:o + p.numel()].clone() for p, o in zip(opt.flat.params, opt.flat.offsets)]


def _check_three_steps(model, opt, batch_fn, loss_fn, exclude_1d, nesterov, max_grad_norm=None):
    params = opt.tensors  # the order of opt.stats(): the flat buffer's when there is one
    adapted = [not (exclude_1d and p.ndim <= 1) for p in params]
    for step in range(3):
        x, y = batch_fn(step)
        loss = loss_fn(model(x), y)
        opt.zero_grad()
        loss.backward()
        w0 = [p.detach().clone() for p in params]
        g0 = [p.grad.detach().clone() for p in params]
        b0 = _bufs(opt)
        opt.step()
        rw, rb, rstats, rG = lars_ref_step(w0, g0, b0, adapted, lr=HP["lr"], eta=HP["eta"],
                                           wd=HP["wd"], mu=HP["mu"], nesterov=nesterov,
                                           max_grad_norm=max_grad_norm)
        for i, (p, b) in enumerate(zip(params, _bufs(opt))):
            torch.testing.assert_close(p.detach().double().reshape(-1), rw[i], rtol=1e-5,
                                       atol=1e-7, msg=f"step {step} w[{i}]")
            torch.testing.assert_close(b.double().reshape(-1), rb[i], rtol=1e-5, atol=1e-7,
                                       msg=f"step {step} buf[{i}]")
            if not adapted[i]:
                assert rstats[i, 2] == 1.0
        stats, gnorm = opt.stats()
        torch.testing.assert_close(stats.double(), rstats, rtol=1e-5, atol=1e-7)
        assert abs(float(gnorm) - rG) <= 1e-5 * rG


@pytest.mark.parametrize("exclude_1d", [True, False])
@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_flat_cpu_matches_float64(exclude_1d, nesterov):
    from dmlab.models import Net

    torch.manual_seed(0)
    model = Net()
    opt = _opt(model.parameters(), exclude_1d, nesterov)
    assert opt.flat is model.flat and opt.flat.device.type == "cpu"
    _check_three_steps(model, opt, lambda s: _lenet_batch(10 + s), F.cross_entropy, exclude_1d,
                       nesterov)
    assert float(opt.flat.data.abs().sum()) > 0


@pytest.mark.parametrize("exclude_1d", [True, False])
def test_lars_per_tensor_path_matches_float64(exclude_1d):
    torch.manual_seed(1)
    model = torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    opt = _opt(model.parameters(), exclude_1d)
    assert opt.flat is None

    def batch(s):
        g = torch.Generator().manual_seed(20 + s)
        return torch.rand(8, 12, generator=g), torch.rand(8, 4, generator=g)

    _check_three_steps(model, opt, batch, F.mse_loss, exclude_1d, False)


def test_lars_clipping_cpu_matches_float64():
    """max_grad_norm far below the gradient norm: c < 1 enters every tensor's update."""
    from dmlab.models import Net

    torch.manual_seed(2)
    model = Net()
    opt = _opt(model.parameters(), max_grad_norm=1e-3)
    _check_three_steps(model, opt, lambda s: _lenet_batch(30 + s), F.cross_entropy, True, False,
                       max_grad_norm=1e-3)


def test_lars_grad_scale_is_folded():
    """grad_scale = 1/2 on doubled gradients gives the step of the plain gradients."""
    torch.manual_seed(3)
    m1 = torch.nn.Linear(6, 5)
    m2 = torch.nn.Linear(6, 5)
    m2.load_state_dict(m1.state_dict())
    o1, o2 = _opt(m1.parameters()), _opt(m2.parameters())
    o2.grad_scale = 0.5
    x = torch.rand(4, 6)
    m1(x).square().sum().backward()
    (2 * m2(x).square().sum()).backward()
    o1.step()
    o2.step()
    for a, b in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("flat", [True, False])
def test_lars_state_dict_resume_is_bit_identical(flat):
    from dmlab.models import Net
    from dmlab.models.reference import TorchLeNet

    make = Net if flat else TorchLeNet
    torch.manual_seed(4)
    a = make()
    oa = _opt(a.parameters(), nesterov=True)
    assert (oa.flat is not None) == flat

    def one(model, opt, s):
        x, y = _lenet_batch(40 + s)
        loss = F.cross_entropy(model(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()

    for s in range(2):
        one(a, oa, s)
    oa.lr = 0.25  # a scheduled rate travels with the checkpoint
    sd = oa.state_dict()
    assert any(torch.is_tensor(v) and float(v.abs().sum()) > 0 for v in sd.values())
    b = make()
    b.load_state_dict(a.state_dict())
    ob = _opt(b.parameters(), nesterov=True)
    ob.load_state_dict(sd)
    assert ob.lr == 0.25 and ob.step_count == 2
    one(a, oa, 2)
    one(b, ob, 2)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    for p, q in zip(_bufs(oa), _bufs(ob)):
        assert torch.equal(p, q)


def test_param_groups_lr_reaches_the_step():
    m = torch.nn.Linear(3, 3)
    opt = _opt(m.parameters())
    m(torch.ones(2, 3)).sum().backward()
    w0 = m.weight.detach().clone()
    for g in opt.param_groups:
        g["lr"] = 0.0
    opt.step()
    assert opt.lr == 0.0 and torch.equal(m.weight, w0)


def test_warmup_poly_lr_closed_form():
    from dmlab.optim import WarmupPolyLR

    class Opt:
        lr = 0.8

    base, warm, total, power, end = 0.8, 10, 50, 2.0, 0.01
    opt = Opt()
    sched = WarmupPolyLR(opt, warm, total, power=power, end_lr=end)

    def closed(t):
        if t < warm:
            return base * t / warm
        return end + (base - end) * (1 - (t - warm) / (total - warm)) ** power

    assert opt.lr == 0.0  # step 0
    seen = {0: opt.lr}
    for t in range(1, total + 1):
        sched.step()
        seen[t] = opt.lr
    for t in (0, 5, 10, 30, 50):  # step 0, mid warm-up, its end, mid decay, the last step
        assert seen[t] == pytest.approx(closed(t), rel=1e-12, abs=1e-15), t
    assert seen[5] == pytest.approx(0.4) and seen[10] == pytest.approx(0.8)
    assert seen[30] == pytest.approx(0.01 + 0.79 * 0.25) and seen[50] == pytest.approx(0.01)
    sched.step()  # past the end: stays at end_lr
    assert opt.lr == pytest.approx(end)
    # no warm-up: the base rate at step 0
    o2 = Opt()
    WarmupPolyLR(o2, 0, 10)
    assert o2.lr == pytest.approx(0.8)


def _lars_ddp(rank, ws, path):
    """Two gloo ranks with the 1/ws average folded into LARS: replicas stay bit-equal and
    match one process stepping on the concatenated batch."""
    import torch.distributed as dist

    from dmlab.models import Net
    from dmlab.parallel import DDP

    torch.manual_seed(0)
    model = Net()
    ref = Net()
    ref.load_state_dict(model.state_dict())
    X, Y = _lenet_batch(7, ws * 6)
    ddp = DDP(model, bucket_cap_mb=0.05, first_bucket_mb=0.01)
    opt = ddp.fold_average_into(_opt(model.parameters(), lr=0.1))
    assert opt.grad_scale == 1.0 / ws
    opt_ref = _opt(ref.parameters(), lr=0.1)
    for step in range(2):
        xs, ys = X[rank * 6:(rank + 1) * 6], Y[rank * 6:(rank + 1) * 6]
        loss = F.cross_entropy(ddp(xs), ys)
        opt.zero_grad()
        loss.backward()
        opt.step()
        lref = F.cross_entropy(ref(X), Y)
        opt_ref.zero_grad()
        lref.backward()
        opt_ref.step()
    mine = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    everyone = [torch.zeros_like(mine) for _ in range(ws)]
    dist.all_gather(everyone, mine)
    for other in everyone:
        assert torch.equal(other, mine), "replicas diverged"
    for (n, a), (_, b) in zip(model.named_parameters(), ref.named_parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=n)


@pytest.mark.slow
def test_lars_ddp_two_ranks_gloo():
    run_dist(_lars_ddp, 2, None)


def test_task3_lars_flags(tmp_path, monkeypatch):
    from dmlab.tasks import task3

    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    ck = str(tmp_path / "lars.pt")
    args = ["--device", "cpu", "--synthetic", "--optimizer", "lars", "--warmup-steps", "5",
            "--max-steps", "20", "--train-samples", "640", "--lr", "0.5", "--trust-coef", "0.02",
            "--weight-decay", "1e-4", "--no-test", "--save", ck]
    stats = task3.main(args)
    assert stats["optimizer"] == "lars" and stats["steps"] == 20
    assert "fused" not in stats  # --fused auto resolved to the layer-wise loop
    sd = torch.load(ck, weights_only=True)
    assert all(bool(torch.isfinite(v).all()) for v in sd["model"].values())
    assert sd["optimizer"]["lr"] == pytest.approx(0.0)  # the schedule ended at step 20
    assert float(sd["optimizer"]["buf"].abs().sum()) > 0
    with pytest.raises(SystemExit):
        task3.main(args + ["--fused", "1"])


def test_task3_default_reports_no_optimizer(monkeypatch):
    """With the new flags left alone the result carries no new key."""
    from dmlab.tasks import task3

    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    stats = task3.main(["--device", "cpu", "--synthetic", "--max-steps", "3", "--train-samples",
                        "96", "--no-test"])
    assert "optimizer" not in stats and stats["steps"] == 3
