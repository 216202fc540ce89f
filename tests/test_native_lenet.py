"""Native HIP LeNet / MLP / loss vs the PyTorch fp32 reference of the same ops."""
import copy

import pytest
import torch
import torch.nn.functional as F

from dmlab.models import ForwardNN, Net
from dmlab.nn import count_correct, cross_entropy
from dmlab.ops._native import lib

pytestmark = pytest.mark.gpu


def _pair(cls, dev, **kw):
    torch.manual_seed(0)
    a = cls(**kw).to(dev)
    b = copy.deepcopy(a).set_backend("torch")
    b._flatten()
    return a, b


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("B", [1, 32, 257])
def test_lenet_fwd_bwd_matches_torch(dev, B):
    lib()  # fail loudly if the extension is missing
    a, b = _pair(Net, dev)
    x = torch.rand(B, 1, 28, 28, device=dev)
    y = torch.randint(0, 10, (B,), device=dev)
    la = cross_entropy(a(x), y)
    lb = F.cross_entropy(b(x), y)
    la.backward()
    lb.backward()
    torch.testing.assert_close(la, lb, rtol=1e-4, atol=1e-5)
    ga, gb = _grads(a), _grads(b)
    for n in ga:
        torch.testing.assert_close(ga[n], gb[n], rtol=2e-3, atol=2e-5, msg=n)


@pytest.mark.parametrize("B", [32, 200])
def test_lenet_bf16_activations(dev, B):
    """BASELINE config 3 (task3 DDP CNN bf16): bf16 activations through every native LeNet
    kernel (thin conv + pool, MFMA linear, CE), fp32 master weights and gradients.  Error vs
    the fp32 PyTorch reference must stay within 2x that of PyTorch's own bf16 autocast."""
    a, b = _pair(Net, dev)
    _, c = _pair(Net, dev)  # same seed: same weights
    x = torch.rand(B, 1, 28, 28, device=dev)
    y = torch.randint(0, 10, (B,), device=dev)
    out = a(x.to(torch.bfloat16))
    assert out.dtype == torch.bfloat16
    la = cross_entropy(out, y)
    lb = F.cross_entropy(b(x), y)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        oc = c(x)
    lc = F.cross_entropy(oc.float(), y)
    for loss in (la, lb, lc):
        loss.backward()
    assert la.dtype == torch.float32
    torch.testing.assert_close(la, lb, rtol=2e-2, atol=2e-3)
    ga, gb, gc = _grads(a), _grads(b), _grads(c)
    for n in ga:
        assert ga[n].dtype == torch.float32
        rel = ((ga[n] - gb[n]).norm() / gb[n].norm().clamp_min(1e-12)).item()
        rel_autocast = ((gc[n] - gb[n]).norm() / gb[n].norm().clamp_min(1e-12)).item()
        assert rel < max(2 * rel_autocast, 1e-2), (n, rel, rel_autocast)


def test_lenet_grad_accumulation_semantics(dev):
    a, b = _pair(Net, dev)
    x = torch.rand(16, 1, 28, 28, device=dev)
    y = torch.randint(0, 10, (16,), device=dev)
    for m in (a, b):
        for _ in range(2):  # no zero_grad in between -> grads accumulate
            F.cross_entropy(m(x), y).backward()
    ga, gb = _grads(a), _grads(b)
    for n in ga:
        torch.testing.assert_close(ga[n], gb[n], rtol=2e-3, atol=4e-5, msg=n)


def test_lenet_input_grad(dev):
    a, b = _pair(Net, dev)
    x1 = torch.rand(8, 1, 28, 28, device=dev, requires_grad=True)
    x2 = x1.detach().clone().requires_grad_(True)
    a(x1).square().sum().backward()
    b(x2).square().sum().backward()
    torch.testing.assert_close(x1.grad, x2.grad, rtol=2e-3, atol=1e-5)


def test_mlp_matches_torch(dev):
    a, b = _pair(ForwardNN, dev)
    x = torch.rand(64, 1, 28, 28, device=dev)
    y = torch.randint(0, 10, (64,), device=dev)
    la = cross_entropy(a(x), y)
    lb = F.cross_entropy(b(x), y)
    la.backward()
    lb.backward()
    torch.testing.assert_close(la, lb, rtol=1e-4, atol=1e-5)
    ga, gb = _grads(a), _grads(b)
    for n in ga:
        torch.testing.assert_close(ga[n], gb[n], rtol=2e-3, atol=2e-5, msg=n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", [(300, 1000), (32, 10), (256, 1000), (1, 10)])
def test_cross_entropy_kernel(dev, dtype, B, C):
    x = (torch.randn(B, C, device=dev) * 3).to(dtype).requires_grad_(True)
    y = torch.randint(0, C, (B,), device=dev)
    l1 = cross_entropy(x, y)
    l1.backward(torch.tensor(2.0, device=dev))
    xr = x.detach().float().requires_grad_(True)
    l2 = F.cross_entropy(xr, y)
    (2 * l2).backward()
    torch.testing.assert_close(l1, l2, rtol=1e-4, atol=1e-4)
    tol = 1e-6 if dtype == torch.float32 else 2e-3
    torch.testing.assert_close(x.grad.float(), xr.grad, rtol=tol, atol=tol)


def test_argmax_count(dev):
    x = torch.randn(1000, 10, device=dev)
    y = torch.randint(0, 10, (1000,), device=dev)
    c = count_correct(x, y)
    assert int(c) == int((x.argmax(1) == y).sum())


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (33, 70, 129), (256, 1000, 512)])
@pytest.mark.parametrize("relu", [False, True])
def test_gemm_strided(dev, M, N, K, relu):
    A = torch.randn(M, K, device=dev)
    W = torch.randn(N, K, device=dev)
    bias = torch.randn(N, device=dev)
    C = torch.empty(M, N, device=dev)
    lib().gemm(A, None, W, C, None, bias, M, N, K, K, 1, 1, K, N, 1.0, 0.0, relu)
    ref = A @ W.T + bias
    if relu:
        ref = ref.relu()
    torch.testing.assert_close(C, ref, rtol=1e-4, atol=1e-4 * K ** 0.5)


@pytest.mark.parametrize("M,N,K", [(5, 70, 33), (256, 1000, 512)])
def test_gemm_bf16_lowp(dev, M, N, K):
    """bf16-MFMA path (ResNet head): fwd (fp32 weight rounded while staging, bias, bf16
    out), wgrad (transposed A, fp32 out with beta) and dgrad, vs fp32 math on the same
    bf16-rounded operands."""
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(M, K, device=dev, generator=g).bfloat16()
    W = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
    bias = torch.randn(N, device=dev, generator=g)
    Wb = W.bfloat16().float()
    y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    lib().gemm(x, None, W, y, None, bias, M, N, K, K, 1, 1, K, N, 1.0, 0.0, False, lowp=True)
    ref = x.float() @ Wb.T + bias
    torch.testing.assert_close(y.float(), ref, rtol=1e-2, atol=1e-2)
    dy = torch.randn(M, N, device=dev, generator=g).bfloat16()
    gw = torch.randn(N, K, device=dev, generator=g)
    base = gw.clone()
    lib().gemm(dy, None, x, None, gw, None, N, K, M, 1, N, K, 1, K, 1.0, 1.0, False, lowp=True)
    torch.testing.assert_close(gw, base + dy.float().T @ x.float(), rtol=1e-3, atol=1e-3 * M ** 0.5)
    dx = torch.empty(M, K, device=dev, dtype=torch.bfloat16)
    lib().gemm(dy, None, W, dx, None, None, M, K, N, N, 1, K, 1, K, 1.0, 0.0, False, lowp=True)
    torch.testing.assert_close(dx.float(), dy.float() @ Wb, rtol=1e-2, atol=2e-2)


def test_task3_bf16_on_gpu(dev, tmp_path):
    """task3 --dtype bf16 (BASELINE config 3) at world size 1: bf16 device-resident data,
    the native kernels, DDP wrapper and fused SGD; the loss is finite and falls."""
    from dmlab.tasks import task3

    stats = task3.main(["--synthetic", "--dtype", "bf16", "--epochs", "1", "--train-samples",
                        "4096", "--lr", "0.05", "--no-test", "--device", "cuda"])
    ls = stats["losses"]
    assert stats["steps"] == 128 and len(ls) == 6
    assert all(l == l and l < 10 for l in ls) and ls[-1] < ls[0]


def test_task3_fused_path_matches_layerwise(dev):
    """task3's GPU fast path (fused 2-dispatch step, device-side sampler cursor, hipGraph) and
    the layer-wise eager loop train the same model on the same shard order: the printed
    20-step loss averages agree (fp32; only the reduction order differs)."""
    from dmlab.tasks import task3

    args = ["--synthetic", "--epochs", "1", "--train-samples", "3200", "--lr", "0.05",
            "--no-test", "--device", "cuda"]
    fast = task3.main(args + ["--fused", "1"])
    slow = task3.main(args + ["--fused", "0"])
    assert fast.get("hip_graph") is True and "hip_graph" not in slow
    assert fast.get("hip_graph_steps") == 20  # 20 complete steps per replay
    assert fast["steps"] == slow["steps"] == 100
    assert len(fast["losses"]) == len(slow["losses"]) == 5
    for a, b in zip(fast["losses"], slow["losses"]):
        assert abs(a - b) < 2e-3 * max(1.0, abs(b)), (fast["losses"], slow["losses"])


def test_task3_graph_steps_match_single_step_graphs(dev):
    """20 steps per graph replay vs one: the same kernels in the same order, so the printed
    loss averages agree bit for bit -- over an epoch of 95 whole batches (4 blocks + 15
    single steps on the 1-step graph) plus the shard's partial last batch (10 samples, one
    eager fused step, as the reference DataLoader keeps it), and a --max-steps cut inside
    the second epoch."""
    from dmlab.tasks import task3

    args = ["--synthetic", "--epochs", "2", "--train-samples", "3050", "--lr", "0.05",
            "--no-test", "--device", "cuda", "--fused", "1", "--max-steps", "150"]
    k20 = task3.main(args + ["--graph-steps", "20"])
    k1 = task3.main(args + ["--graph-steps", "1"])
    eager = task3.main(args + ["--graph", "0"])
    assert k20["hip_graph_steps"] == 20 and k1["hip_graph_steps"] == 1
    assert k20["steps"] == k1["steps"] == eager["steps"] == 150
    assert k20["samples"] == 96 * 32 - 22 + 54 * 32  # epoch 1 incl. its 10-sample tail
    assert len(k20["losses"]) == len(k1["losses"]) == 6  # 4 in epoch 1, 2 before the cut
    for a, b, c in zip(k20["losses"], k1["losses"], eager["losses"]):
        assert a == b == c, (k20["losses"], k1["losses"], eager["losses"])


def test_task3_resume_keeps_momentum_on_the_graph_path(dev, tmp_path):
    """A resumed run restores SGD momentum from the checkpoint; the graph-captured fused loop
    must train from it exactly like the eager fused loop (the capture warm-up's momentum is
    restored, not zeroed)."""
    from dmlab.tasks import task3

    ck = str(tmp_path / "ck.pt")
    base = ["--synthetic", "--epochs", "1", "--train-samples", "1280", "--lr", "0.05",
            "--no-test", "--device", "cuda", "--fused", "1"]
    task3.main(base + ["--graph", "0", "--max-steps", "30", "--save", ck])
    sd = torch.load(ck, weights_only=True)
    assert float(sd["optimizer"]["buf"].abs().sum()) > 0  # non-zero momentum was saved
    g = task3.main(base + ["--resume", ck, "--max-steps", "40"])
    e = task3.main(base + ["--resume", ck, "--max-steps", "40", "--graph", "0"])
    assert g["hip_graph"] is True and g["hip_graph_steps"] == 20
    assert g["losses"] == e["losses"] and len(g["losses"]) == 2


def test_bench_lenet_graph_steps_bit_equal(tmp_path):
    """bench.py's 25-steps-per-replay LeNet loop vs 1 step per replay over an epoch rollover
    (25 warm-up + 1900 timed steps > 1875 batches): identical final loss and parameters."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    out = []
    for k in (25, 1):
        r = subprocess.run([sys.executable, str(root / "bench.py"), "--model", "lenet",
                            "--warmup", "25", "--steps", "1900", "--full", "--phases", "0",
                            "--graph-steps", str(k)], cwd=tmp_path, capture_output=True,
                           text=True, timeout=300, env=dict(os.environ))
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
    a, b = out
    assert a["config"]["hip_graph_steps"] == 25 and b["config"]["hip_graph_steps"] == 1
    assert a["final_loss"] == b["final_loss"]
    assert a["param_checksum"] == b["param_checksum"]


def test_task3_torchrun_fused_throughput(tmp_path):
    """BASELINE config 3's entry point under torchrun (one rank, RCCL group) on the fast
    path: the reference lab-3 loop at batch 32 runs at hundreds of thousands of samples/s
    (the reference-style eager loop: ~100k on this GPU)."""
    import os
    import re
    import subprocess
    import sys
    from pathlib import Path

    from dist_helpers import free_port

    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, PYTHONPATH=str(root))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m",
                        "dmlab.tasks.task3", "--synthetic", "--epochs", "1", "--no-test"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"Throughput: ([0-9.]+) samples/s", r.stdout)
    assert m, r.stdout[-2000:]
    assert len(re.findall(r"loss: (\d+\.\d+)", r.stdout)) == 1875 // 20
    # 20 steps per graph replay: >= 1.0 M img/s on one MI355X (0.89 M at one per replay)
    assert float(m.group(1)) > 900_000, r.stdout[-500:]


# ---------------------------------------------------------------- fused 2-dispatch step
@pytest.mark.parametrize("B", [32, 7, 200])
@pytest.mark.parametrize("xdtype", [torch.float32, torch.bfloat16])
def test_fused_lenet_step_matches_torch(dev, B, xdtype):
    """FusedLeNetStep (csrc/lenet_fused.hip: per-sample fwd+bwd workgroups, then the batch
    reduction fused with SGD) vs the plain PyTorch fp32 autograd step on the same weights:
    loss, every gradient, and the SGD-momentum update over three steps (first-step buffer
    init included)."""
    from dmlab.models.lenet_fused import FusedLeNetStep
    from dmlab.optim import SGD

    a, b = _pair(Net, dev)
    opt_a = SGD(a.parameters(), lr=0.05, momentum=0.9)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.05, momentum=0.9)
    step = FusedLeNetStep(a, opt_a)
    g = torch.Generator(device=dev).manual_seed(B)
    for it in range(3):
        x = torch.rand(B, 1, 28, 28, device=dev, generator=g)
        y = torch.randint(0, 10, (B,), device=dev, generator=g)
        xa = x.to(xdtype)
        la = step(xa, y)
        lb = F.cross_entropy(b(xa.float()), y)
        opt_b.zero_grad()
        lb.backward()
        torch.testing.assert_close(la, lb.detach(), rtol=1e-4, atol=1e-5)
        ga, gb = _grads(a), _grads(b)
        for n in ga:
            torch.testing.assert_close(ga[n], gb[n], rtol=2e-3, atol=2e-5, msg=f"{n} step {it}")
        opt_b.step()
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-6, msg=f"{n} step {it}")


def test_fused_lenet_step_grads_only(dev):
    """Without a fusable optimiser (Adam) the fused step writes the gradients and the
    optimiser runs after it; the loss is the batch mean."""
    from dmlab.models.lenet_fused import FusedLeNetStep
    from dmlab.optim import AdamOptimizer

    a, b = _pair(Net, dev)
    opt = AdamOptimizer(a.parameters(), lr=1e-3)
    step = FusedLeNetStep(a, opt)
    x = torch.rand(16, 1, 28, 28, device=dev)
    y = torch.randint(0, 10, (16,), device=dev)
    la = step(x, y)
    lb = F.cross_entropy(b(x), y)
    lb.backward()
    torch.testing.assert_close(la, lb.detach(), rtol=1e-4, atol=1e-5)
    ga, gb = _grads(a), _grads(b)
    for n in ga:
        torch.testing.assert_close(ga[n], gb[n], rtol=2e-3, atol=2e-5, msg=n)


def test_fused_lenet_step_graph_capture(dev):
    """The fused step replays from a hipGraph (2 kernel nodes) and matches eager."""
    from dmlab.models.lenet_fused import FusedLeNetStep
    from dmlab.optim import SGD
    from dmlab.utils.graph import CapturedStep

    a, b = _pair(Net, dev)
    c = copy.deepcopy(a)
    c._flatten()
    x = torch.rand(32, 1, 28, 28, device=dev)
    y = torch.randint(0, 10, (32,), device=dev)
    sa = FusedLeNetStep(a, SGD(a.parameters(), lr=0.01, momentum=0.9))
    sc = FusedLeNetStep(c, SGD(c.parameters(), lr=0.01, momentum=0.9))
    cap = CapturedStep(lambda xx, yy: sa(xx, yy).clone(), [x, y], warmup=2, bind_inputs=True)
    for _ in range(2):
        sc(x, y)  # the capture warm-up ran two eager steps on `a`
    for _ in range(3):
        la = cap(x, y)
        lc = sc(x, y).clone()
        torch.testing.assert_close(la, lc, rtol=0, atol=0)
    for p, q in zip(a.parameters(), c.parameters()):
        torch.testing.assert_close(p, q, rtol=0, atol=0)


def test_fused_lenet_step_device_cursor(dev):
    """The fused step fed by the device-resident loader: the sample kernel gathers its rows
    through the sampler's epoch order at the device cursor, the gradient kernel advances the
    cursor (wrapping at the epoch end); captured in a hipGraph it walks the shard exactly like
    explicit batches do eagerly."""
    from dmlab.data import DeviceLoader, MySampler, TensorDataset
    from dmlab.models.lenet_fused import FusedLeNetStep
    from dmlab.optim import SGD
    from dmlab.utils.graph import CapturedStep

    a, _ = _pair(Net, dev)
    c = copy.deepcopy(a)
    c._flatten()
    g = torch.Generator(device=dev).manual_seed(9)
    ds = TensorDataset(torch.rand(100, 1, 28, 28, device=dev, generator=g),
                       torch.randint(0, 10, (100,), device=dev, generator=g))
    ld = DeviceLoader(ds, 16, sampler=MySampler(ds, 2, 1, shuffle=True, seed=0), drop_last=True)
    cur = ld.cursor()
    assert cur.nbatch == 3
    sa = FusedLeNetStep(a, SGD(a.parameters(), lr=0.01, momentum=0.9))
    sc = FusedLeNetStep(c, SGD(c.parameters(), lr=0.01, momentum=0.9))
    cap = CapturedStep(lambda xx, yy: sa(xx, yy, cursor=cur).clone(), [ds.images, ds.labels],
                       warmup=2, bind_inputs=True)
    cur.refill(0)
    order = cur.order.clone()
    # the capture warm-up ran two eager steps on `a` (batches 0, 1); refill rewound the
    # cursor, so the 7 replays take batches 0, 1, 2, 0, ... (wrapping at the epoch end)
    seq = [0, 1] + [k % 3 for k in range(7)]
    for k in seq[:2]:
        sc(*ds.batch(order[k * 16:(k + 1) * 16]))
    for k in seq[2:]:
        la = cap(ds.images, ds.labels)
        lc = sc(*ds.batch(order[k * 16:(k + 1) * 16])).clone()
        torch.testing.assert_close(la, lc, rtol=0, atol=0)
    assert int(cur.cursor) == 7 % 3
    for p, q in zip(a.parameters(), c.parameters()):
        torch.testing.assert_close(p, q, rtol=0, atol=0)


@pytest.mark.parametrize("B", [8, 100])
@pytest.mark.parametrize("bf16", [False, True])
def test_tp_head_native_matches_full_model(dev, B, bf16):
    """Tensor-parallel LeNet head on the native path (degree 1 on one GPU): the row-split
    fc2's local GEMM into fp32, bias + ReLU + cast in one kernel after the all-reduce, the
    ReLU mask and bias gradient from the GEMM / column-sum kernels -- against the full
    single-device model on the PyTorch reference path."""
    from dmlab.parallel.tensor_parallel import TPLeNet

    torch.manual_seed(0)
    full = Net().to(dev)
    ref = copy.deepcopy(full).set_backend("torch")
    ref._flatten()
    tp = TPLeNet().to(dev).load_from_full(full)
    x = torch.rand(B, 1, 28, 28, device=dev)
    y = torch.randint(0, 10, (B,), device=dev)
    out = tp(x.to(torch.bfloat16) if bf16 else x)
    assert out.dtype == (torch.bfloat16 if bf16 else torch.float32)
    la = cross_entropy(out, y)
    lb = F.cross_entropy(ref(x), y)
    la.backward()
    lb.backward()
    tol = dict(rtol=3e-2, atol=3e-3) if bf16 else dict(rtol=2e-3, atol=2e-5)
    torch.testing.assert_close(la.float(), lb, **tol)
    torch.testing.assert_close(tp.fc2.rbias.grad, ref.fc2.bias.grad, **tol)
    torch.testing.assert_close(tp.fc2.weight.grad, ref.fc2.weight.grad, **tol)
    torch.testing.assert_close(tp.fc1.weight.grad, ref.fc1.weight.grad, **tol)
    torch.testing.assert_close(tp.conv1.weight.grad, ref.conv1.weight.grad, **tol)
