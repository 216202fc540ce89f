"""The q8 gradient codec on the CPU: the torch path against the float64 reference
(tests/gradq_ref.py), the aggregator / DDP plumbing on gloo ranks against a hand simulation,
the task flags, and a training sanity check."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gradq_ref as R
from dist_helpers import free_port, run_dist

ROOT = Path(__file__).resolve().parent.parent
SIZES = [1, 4, 255, 256, 257, 1027]
LENET_FLAT = 52160  # LeNet's 51,902 parameters, each tensor's slot padded to 64 elements


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def encode(g, r=None):
    """numpy in, numpy out: (scales, codes, new residual or None) from the torch path."""
    from dmlab.parallel.compress import encode_torch, payload_bytes

    n = g.shape[0]
    assert payload_bytes(n) == R.payload_bytes(n)
    payload = torch.full((payload_bytes(n),), 0xA5, dtype=torch.uint8)
    rt = None if r is None else _t(r).clone()
    encode_torch(_t(g), rt, payload)
    s, q = R.split_payload(payload.numpy(), n)
    return s, q, payload.numpy(), (None if rt is None else rt.numpy())


def decode(payloads, n, c):
    from dmlab.parallel.compress import decode_mean_torch

    out = torch.full((n,), 7.0)
    decode_mean_torch(_t(np.stack(payloads)), out, c)
    return out.numpy()


# ------------------------------------------------------------------ layout
def test_payload_bytes_layout():
    from dmlab.parallel.compress import payload_bytes

    for n in SIZES + [51902, LENET_FLAT, 300001, 11_700_000]:
        pb = payload_bytes(n)
        assert pb == R.payload_bytes(n) and pb % 16 == 0
        assert 0 <= pb - (4 * R.n_blocks(n) + n) < 16
    assert abs(4 * 11_700_000 / payload_bytes(11_700_000) - 3.94) < 0.01


# ------------------------------------------------------------------ exact inputs
@pytest.mark.parametrize("k", [-20, 0, 7])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("ef", [True, False])
def test_exact_integer_blocks(n, k, ef):
    g, ints = R.exact_ints(n, k, seed=n)
    s, q, _, r = encode(g, np.zeros(n, np.float32) if ef else None)
    assert (s == np.float32(2.0 ** k)).all()
    assert (q == ints).all()
    if ef:
        assert (r == 0).all()


@pytest.mark.parametrize("k", [-20, 0, 7])
@pytest.mark.parametrize("n", SIZES)
def test_half_integer_blocks_round_to_even(n, k):
    g, odd = R.half_ints(n, k, seed=n)
    s, q, _, r = encode(g, np.zeros(n, np.float32))
    assert (s == np.float32(2.0 * 2.0 ** k)).all()
    want = R.half_int_codes(odd)
    assert (q == want).all() and (q[np.abs(odd) < 254] % 2 == 0).all()
    # the residual is exactly e - q*s: +-2^k, and 0 at the block's maximum
    assert (r.astype(np.float64) == (odd - 2 * want) * 2.0 ** k).all()
    assert (np.abs(r[np.abs(odd) < 254]) == np.float32(2.0 ** k)).all()


def test_residual_enters_the_sum_exactly():
    """e = g + r: integers split between the gradient and the carried residual."""
    n = 1027
    g, ints = R.exact_ints(n, 0, seed=3)
    part = np.random.default_rng(1).integers(-40, 41, size=n).astype(np.float32)
    s, q, _, r = encode(g - part, part)
    assert (s == 1).all() and (q == ints).all() and (r == 0).all()


# ------------------------------------------------------------------ random inputs
@pytest.mark.parametrize("n", [257, 1027, 300001])
@pytest.mark.parametrize("ef", [True, False])
def test_random_normal_properties(n, ef):
    g, r0 = R.random_pair(n)
    r0 = r0 if ef else None
    s, q, _, r = encode(g, r0)
    ref = R.check_encode_properties(g, r0, s, q, r)
    # away from ties the codes are the float64 reference's
    keep = R.tie_free(ref["x"])
    assert (q[keep] == ref["q"][keep]).all()
    assert 1.0 - keep.mean() <= 1e-3


def test_tie_margin_share_of_the_seeds():
    """The random-input checks (here and in tests/test_gradq_gpu.py) leave elements within
    2^-12 of a tie out of their code comparison and cap their share at 0.1 %: with the
    reference alone, the chosen seeds stay under the cap (normal data puts about 0.05 % of
    values that close to a tie)."""
    for n in R.SEEDS:
        g, r0 = R.random_pair(n)
        for r in (None, r0):
            assert 1.0 - R.tie_free(R.encode_ref(g, r)["x"]).mean() <= 1e-3, n


# ------------------------------------------------------------------ special blocks
def test_special_blocks():
    n = 6 * 256 + 10
    g = R.random_normal(n, seed=9)
    g[0:256] = 0.0                                  # all zero
    g[256:512] = 0.0
    g[300] = -3.5                                   # a single nonzero
    g[512:768] = np.float32(1e-44) * np.sign(g[512:768])   # denormal: a / 127 == 0
    g[800] = np.inf                                 # a block holding inf
    g[1100] = np.nan                                # a block holding nan
    r0 = np.zeros(n, np.float32)
    r0[1024:1280] = 0.25
    assert np.float32(1e-44) / np.float32(127) == 0
    s, q, payload, r = encode(g, r0)
    assert s[0] == 0 and (q[:256] == 0).all() and (r[:256] == 0).all()
    assert s[1] == np.float32(3.5) / np.float32(127)
    assert q[300] == -127 and (np.delete(q[256:512], 44) == 0).all()
    assert s[2] == 0 and (q[512:768] == 0).all() and (r[512:768] == g[512:768]).all()
    for b in (3, 4):  # non-finite: NaN scale, zero codes, zero residual
        assert np.isnan(s[b]) and (q[b * 256:(b + 1) * 256] == 0).all()
        assert (r[b * 256:(b + 1) * 256] == 0).all()
    R.check_encode_properties(g[1280:], r0[1280:], s[5:], q[1280:], r[1280:])  # the rest is sane
    out = decode([payload, payload], n, 0.5)
    assert np.isnan(out[768:1280]).all() and np.isfinite(out[:768]).all()
    assert np.isfinite(out[1280:]).all() and (out[:256] == 0).all() and (out[512:768] == 0).all()


# ------------------------------------------------------------------ decode-mean
@pytest.mark.parametrize("ws", [1, 2, 3, 8])
def test_decode_mean_exact_on_integers(ws):
    n = 1027
    payloads, total = [], np.zeros(n)
    for rk in range(ws):
        g, ints = R.exact_ints(n, rk - 3, seed=10 + rk)
        _, _, p, _ = encode(g)
        payloads.append(p)
        total += ints * 2.0 ** (rk - 3)  # exact: small integers times powers of two
    for c in (1.0, 1.0 / ws):
        want = (total * np.float64(np.float32(c))).astype(np.float32)  # one fp32 rounding
        assert (decode(payloads, n, c) == want).all()


@pytest.mark.parametrize("ws", [1, 2, 3, 8])
def test_decode_mean_random(ws):
    n = 300001
    payloads = [encode(R.random_normal(n, seed=20 + rk) * (1 + rk))[2] for rk in range(ws)]
    s, q = R.split_payload(np.stack(payloads), n)
    for c in (1.0, 1.0 / ws):
        want = R.decode_mean_ref(s, q, np.float64(np.float32(c)))
        got = decode(payloads, n, c)
        assert np.abs(got - want).max() <= ws * 2.0 ** -23 * np.abs(want).max()


# ------------------------------------------------------------------ error feedback
def test_error_feedback_telescopes():
    """Over 20 steps at ws = 1: sum_t decode_t + r_T == sum_t g_t (each step's residual is
    what the decode missed), within 20 * 2^-22 * max |g|."""
    from dmlab.parallel.compress import Q8Compressor, payload_bytes

    n, steps = 1027, 20
    comp = Q8Compressor(n, "cpu")
    payload = torch.zeros(payload_bytes(n), dtype=torch.uint8)
    out = torch.zeros(n)
    sum_g, sum_d, gmax = np.zeros(n), np.zeros(n), 0.0
    for t in range(steps):
        g = R.random_normal(n, seed=100 + t)
        comp.encode(_t(g), 0, payload)
        comp.decode_mean(payload.view(1, -1), out, 1.0)
        sum_g += g
        sum_d += out.numpy()
        gmax = max(gmax, float(np.abs(g).max()))
    err = np.abs(sum_d + comp.residual.numpy().astype(np.float64) - sum_g).max()
    assert err <= steps * 2.0 ** -22 * gmax, err / gmax


def test_no_error_feedback_keeps_no_residual():
    from dmlab.parallel.compress import Q8Compressor, payload_bytes

    n = 1027
    comp = Q8Compressor(n, "cpu", error_feedback=False)
    assert comp.residual is None and comp.state_dict()["residual"] is None
    g = R.random_normal(n, seed=1)
    s, q, _, _ = encode(g)
    payload = torch.zeros(payload_bytes(n), dtype=torch.uint8)
    for _ in range(2):  # the same input gives the same payload: nothing is carried
        comp.encode(_t(g), 0, payload)
        s2, q2 = R.split_payload(payload.numpy(), n)
        assert (s2 == s).all() and (q2 == q).all()


def test_compressor_state_dict_roundtrip():
    from dmlab.parallel.compress import Q8Compressor, payload_bytes

    n = 700
    a, b = Q8Compressor(n, "cpu"), Q8Compressor(n, "cpu")
    a.encode(_t(R.random_normal(n, seed=2)), 0, torch.zeros(payload_bytes(n), dtype=torch.uint8))
    assert a.residual.abs().max() > 0
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.residual, b.residual)
    with pytest.raises(ValueError):
        Q8Compressor(n, "cpu", error_feedback=False).load_state_dict(a.state_dict())


# ------------------------------------------------------------------ gloo ranks
def _data(ws, per, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(ws * per, 1, 28, 28, generator=g),
            torch.randint(0, 10, (ws * per,), generator=g))


def _simulate(ws, steps, bounds, X, Y, per, c, grad_scale, ef=True):
    """One process plays every rank: each rank's gradient of the shared weights, then the torch
    codec by hand per bucket (encode with that rank's residual, stack, decode-mean), then SGD.
    Returns (flat parameters, per-rank residuals)."""
    from dmlab.models import Net
    from dmlab.optim import SGD
    from dmlab.parallel.compress import decode_mean_torch, encode_torch, payload_bytes

    torch.manual_seed(0)
    model = Net()
    opt = SGD(model.parameters(), lr=0.1, momentum=0.9)
    opt.grad_scale = grad_scale
    n = model.flat.grad.numel()
    res = [torch.zeros(n) for _ in range(ws)]
    for _ in range(steps):
        grads = []
        for rk in range(ws):
            opt.zero_grad()
            F.cross_entropy(model(X[rk * per:(rk + 1) * per]), Y[rk * per:(rk + 1) * per]).backward()
            grads.append(model.flat.grad.clone())
        out = grads[0].clone()  # elements outside every bucket (none) would stay local
        for lo, hi in bounds:
            rows = torch.zeros((ws, payload_bytes(hi - lo)), dtype=torch.uint8)
            for rk in range(ws):
                encode_torch(grads[rk][lo:hi], res[rk][lo:hi] if ef else None, rows[rk])
            decode_mean_torch(rows, out[lo:hi], c)
        model.flat.grad.copy_(out)
        opt.step()
    return model.flat.data.clone(), res


def _same_on_every_rank(t, ws):
    import torch.distributed as dist

    rows = [torch.empty_like(t) for _ in range(ws)]
    dist.all_gather(rows, t.contiguous())
    for r in rows:
        assert torch.equal(r, rows[0])


def _ddp_q8(rank, ws, ef):
    from dmlab.models import Net
    from dmlab.optim import SGD
    from dmlab.parallel import DDP

    per, steps = 6, 3
    X, Y = _data(ws, per)
    torch.manual_seed(0)
    model = Net()
    ddp = DDP(model, bucket_cap_mb=0.05, first_bucket_mb=0.01, compress="q8", error_feedback=ef)
    assert len(ddp.buckets) >= 2 and ddp._native is None
    assert (ddp.compressor.residual is not None) == ef
    opt = ddp.fold_average_into(SGD(model.parameters(), lr=0.1, momentum=0.9))
    for _ in range(steps):
        opt.zero_grad()
        F.cross_entropy(ddp(X[rank * per:(rank + 1) * per]), Y[rank * per:(rank + 1) * per]).backward()
        opt.step()
    assert ddp.buckets_launched == steps * len(ddp.buckets)
    from dmlab.parallel.compress import payload_bytes

    assert ddp.comm_bytes_per_step == sum(payload_bytes(b.hi - b.lo) for b in ddp.buckets)
    want, res = _simulate(ws, steps, [(b.lo, b.hi) for b in ddp.buckets], X, Y, per, 1.0,
                          1.0 / ws, ef)
    assert torch.equal(model.flat.data, want)
    if ef:
        assert torch.equal(ddp.compressor.residual, res[rank])
    _same_on_every_rank(model.flat.data, ws)


@pytest.mark.parametrize("ws", [2, 4])
def test_ddp_q8_ranks_bit_identical_to_simulation(ws):
    run_dist(_ddp_q8, ws, True)


def test_ddp_q8_without_error_feedback():
    run_dist(_ddp_q8, 2, False)


def _agg_q8(rank, ws, _):
    from dmlab.models import Net
    from dmlab.optim import SGD
    from dmlab.parallel import comm
    from dmlab.parallel.compress import payload_bytes

    per, steps = 6, 3
    X, Y = _data(ws, per)
    torch.manual_seed(0)
    model = Net()
    agg = comm.GradAggregator(model, "allgather_q8")
    n = model.flat.grad.numel()
    assert n == LENET_FLAT and agg.bytes_per_call == payload_bytes(n)
    assert comm.GradAggregator(model, "allreduce").bytes_per_call == 4 * n
    assert comm.GradAggregator(model, "allgather").bytes_per_call == 4 * n
    assert comm.GradAggregator(model, "allreduce", "per_param").bytes_per_call == 4 * 51902
    with pytest.raises(ValueError, match="flat"):
        comm.GradAggregator(model, "allgather_q8", granularity="per_param")
    opt = SGD(model.parameters(), lr=0.1, momentum=0.9)
    for _ in range(steps):
        opt.zero_grad()
        F.cross_entropy(model(X[rank * per:(rank + 1) * per]), Y[rank * per:(rank + 1) * per]).backward()
        agg()
        opt.step()
    assert agg.calls == steps and agg.comm_time > 0
    want, res = _simulate(ws, steps, [(0, n)], X, Y, per, 1.0 / ws, 1.0)
    assert torch.equal(model.flat.data, want)
    assert torch.equal(agg.compressor.residual, res[rank])
    _same_on_every_rank(model.flat.data, ws)


@pytest.mark.parametrize("ws", [2, 4])
def test_aggregator_q8_ranks_bit_identical_to_simulation(ws):
    run_dist(_agg_q8, ws, None)


def _generic_module_q8(rank, ws, _):
    """A plain nn.Module under DDP(compress='q8') and under the aggregator: every rank ends
    with the same gradients, close to the mean of the local ones (|error| <= s/2 per rank)."""
    from dmlab.models.reference import TorchLeNet
    from dmlab.parallel import DDP, comm

    X, Y = _data(ws, 4, seed=3)
    xs, ys = X[rank * 4:(rank + 1) * 4], Y[rank * 4:(rank + 1) * 4]
    torch.manual_seed(0)
    ref = TorchLeNet()
    F.cross_entropy(ref(X), Y).backward()
    exact = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
    for kind in ("ddp", "agg"):
        torch.manual_seed(0)
        m = TorchLeNet()
        if kind == "ddp":
            ddp = DDP(m, bucket_cap_mb=0.05, first_bucket_mb=0.01, compress="q8")
            F.cross_entropy(ddp(xs), ys).backward()
            assert ddp.buckets_launched == len(ddp.buckets) >= 2
        else:
            F.cross_entropy(m(xs), ys).backward()
            comm.GradAggregator(m, "allgather_q8")()
        got = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
        _same_on_every_rank(got, ws)
        # each rank's block error is at most s/2 = max|e|/254; the mean's is no larger
        assert (got - exact).abs().max() <= 2 * exact.abs().max() / 254 * ws


def test_generic_module_q8():
    run_dist(_generic_module_q8, 2, None)


def _no_sync_q8(rank, ws, _):
    from dmlab.models import Net
    from dmlab.parallel import DDP

    torch.manual_seed(0)
    model = Net()
    ddp = DDP(model, bucket_cap_mb=0.05, first_bucket_mb=0.01, compress="q8")
    X, Y = _data(ws, 4, seed=5)
    xs, ys = X[rank * 4:(rank + 1) * 4], Y[rank * 4:(rank + 1) * 4]
    with ddp.no_sync():
        F.cross_entropy(ddp(xs), ys).backward()
    assert ddp.buckets_launched == 0 and ddp.compressor.residual.abs().max() == 0
    F.cross_entropy(ddp(xs * 0.5), ys).backward()  # accumulates, then reduces once
    assert ddp.buckets_launched == len(ddp.buckets)
    _same_on_every_rank(model.flat.grad, ws)
    # average=False decodes with c = 1: at two ranks exactly twice the averaged gradient
    torch.manual_seed(0)
    summed = Net()
    sddp = DDP(summed, bucket_cap_mb=0.05, first_bucket_mb=0.01, compress="q8", average=False)
    with sddp.no_sync():
        F.cross_entropy(sddp(xs), ys).backward()
    F.cross_entropy(sddp(xs * 0.5), ys).backward()
    assert ws == 2 and torch.equal(summed.flat.grad, 2 * model.flat.grad)


def test_ddp_q8_no_sync_reduces_once():
    run_dist(_no_sync_q8, 2, None)


def test_ddp_compress_argument_checks():
    from dmlab.models import Net
    from dmlab.parallel import DDP

    with pytest.raises(ValueError, match="comm_dtype"):
        DDP(Net(), compress="q8", comm_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="xgmi"):
        DDP(Net(), compress="q8", small_allreduce="xgmi")
    with pytest.raises(ValueError):
        DDP(Net(), compress="q4")
    one = DDP(Net(), compress="q8")  # one rank, no communication: nothing to compress
    assert one.compressor is None and one._native is None


# ------------------------------------------------------------------ tasks
def _run(args, tmp_path, ok=True, timeout=300):
    env = dict(os.environ, PYTHONPATH=str(ROOT), OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable] + args, cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout + r.stderr


def _torchrun(n):
    return ["-m", "torch.distributed.run", "--nproc-per-node", str(n), "--master-addr",
            "127.0.0.1", "--master-port", str(free_port())]


def test_task2_allgather_q8_two_ranks(tmp_path):
    """task2 prints the byte line after the communication time and writes the figure to its
    JSON.  The coalesced methods send the flat gradient buffer, which for LeNet holds 52,160
    elements (51,902 parameters, every tensor's slot padded to 64 so that it starts on 16
    bytes): the exact figures are payload_bytes(52160) for allgather_q8 and 4 * 52160 for
    allreduce, not those of the bare parameter count."""
    from dmlab.parallel.compress import payload_bytes

    base = ["-m", "dmlab.tasks.task2", "--device", "cpu", "--synthetic", "--train-samples", "1280",
            "--epochs", "1", "--max-steps", "20", "--no-test"]
    out = _run(_torchrun(2) + base + ["--aggregation", "allgather_q8", "--json",
                                      str(tmp_path / "q8.json")], tmp_path)
    m = re.search(r"Total communication time: [\d.eE+-]+\nCommunication bytes per step: (\d+)\n",
                  out)
    assert m and int(m.group(1)) == payload_bytes(LENET_FLAT)
    assert re.search(r"Device: 0 epoch: 1, iters:    20, loss: \d\.\d{3}", out)
    js = json.loads((tmp_path / "q8.json").read_text())
    assert js["comm_bytes_per_step"] == payload_bytes(LENET_FLAT) and js["aggregation"] == "allgather_q8"
    _run(_torchrun(2) + base + ["--aggregation", "allreduce", "--json", str(tmp_path / "ar.json")],
         tmp_path)
    assert json.loads((tmp_path / "ar.json").read_text())["comm_bytes_per_step"] == 4 * LENET_FLAT
    assert 3.9 < 4 * LENET_FLAT / payload_bytes(LENET_FLAT) < 3.95
    # one rank with the collectives forced, residual off
    out = _run(base + ["--aggregation", "allgather_q8", "--no-error-feedback", "--backend", "gloo",
                       "--force-comm", "--master_port", str(free_port())], tmp_path)
    assert f"Communication bytes per step: {payload_bytes(LENET_FLAT)}" in out
    # blocks are defined on the flat buffer
    err = _run(base + ["--aggregation", "allgather_q8", "--granularity", "per_param",
                       "--master_port", str(free_port())], tmp_path, ok=False)
    assert "granularity must be 'flat'" in err


def test_task3_compress_q8_save_resume_residual(tmp_path):
    """--save writes every rank's residual; --resume puts each rank's row back bit for bit
    (a resumed run of zero epochs saves exactly what it loaded)."""
    base = ["-m", "dmlab.tasks.task3", "--device", "cpu", "--synthetic", "--train-samples", "640",
            "--compress", "q8", "--no-test", "--lr", "0.01"]
    ck, ck2 = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    _run(_torchrun(2) + base + ["--epochs", "1", "--max-steps", "5", "--save", ck, "--json",
                                str(tmp_path / "t3.json")], tmp_path)
    js = json.loads((tmp_path / "t3.json").read_text())
    assert js["compress"] == "q8" and 0 < js["comm_bytes_per_step"] < 4 * LENET_FLAT / 3.9
    a = torch.load(ck, weights_only=True)["extra"]["q8_residual"]
    assert a.shape == (2, LENET_FLAT) and a[0].abs().max() > 0 and not torch.equal(a[0], a[1])
    _run(_torchrun(2) + base + ["--epochs", "0", "--resume", ck, "--save", ck2], tmp_path)
    b = torch.load(ck2, weights_only=True)["extra"]["q8_residual"]
    assert torch.equal(a, b)
    for bad in (["--dp", "manual"], ["--allreduce", "xgmi"]):
        assert "--compress q8" in _run(base + bad + ["--master_port", str(free_port())],
                                       tmp_path, ok=False)


# ------------------------------------------------------------------ training sanity
# pixel noise 0.5 (the data sets' default 0.35 is learnt to a loss of 1e-3 within 60 steps, which
# compares nothing) and a rate at which the fp32 run is still descending at step 60
NOISE, LR = 0.5, 0.02


def _train_losses(rank, ws, seed, path):
    """60 steps of LeNet on synthetic data, 2 ranks x batch 16, SGD 0.02 / 0.9: the mean
    training loss of the last 10 steps for fp32 all-reduce, q8 with and without feedback."""
    from dmlab.data.datasets import synthetic_classification
    from dmlab.models import Net
    from dmlab.optim import SGD
    from dmlab.parallel import DDP

    steps, per = 60, 16
    ds = synthetic_classification(steps * ws * per, (1, 28, 28), 10, seed=seed, noise=NOISE)
    final = {}
    for name, kw in (("fp32", {}), ("q8_ef", dict(compress="q8")),
                     ("q8_no_ef", dict(compress="q8", error_feedback=False))):
        torch.manual_seed(seed)
        model = Net()
        ddp = DDP(model, bucket_cap_mb=0.05, first_bucket_mb=0.01, **kw)
        opt = ddp.fold_average_into(SGD(model.parameters(), lr=LR, momentum=0.9))
        losses = []
        for t in range(steps):
            lo = (t * ws + rank) * per
            loss = F.cross_entropy(ddp(ds.images[lo:lo + per]), ds.labels[lo:lo + per])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        final[name] = sum(losses[-10:]) / 10
    if rank == 0:
        Path(path).write_text(json.dumps(final))


# measured on the CPU with this file's _train_losses over seeds 0..4 (the table in
# docs/KERNELS.md, "q8 training sanity"): the fp32 run's final losses were 0.5366, 0.1019, 0.4571,
# 0.5382, 0.0138 -- a seed-to-seed standard deviation (n-1) of 0.2521; the margin is 3 x that
SPREAD_FP32 = 0.2521
TRAIN_SEED = 0


def test_training_sanity_q8_with_error_feedback(tmp_path):
    """q8 with error feedback trains LeNet like the uncompressed exchange: after 60 steps on
    2 gloo ranks its final loss (rank 0, mean of the last 10 steps) is within the fp32 run's
    plus 3 x 0.2521 = 0.756, three times the seed-to-seed standard deviation of the fp32 run's
    final loss over seeds 0..4 (measured with _train_losses on the CPU; SPREAD_FP32 above and
    docs/KERNELS.md hold the figures; q8 itself ended within 0.021 of fp32 at every seed)."""
    out = tmp_path / "losses.json"
    run_dist(_train_losses, 2, TRAIN_SEED, str(out))
    final = json.loads(out.read_text())
    print("final losses", final)
    assert final["q8_ef"] <= final["fp32"] + 3 * SPREAD_FP32, final
