"""The topk gradient codec on the CPU: the torch path against the numpy reference
(tests/gradk_ref.py) bit for bit, the selection rules on built blocks, exact conservation under
error feedback, the decode order, the DDP plumbing on gloo ranks against the codec applied by
hand, and the task flags."""
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

import gradk_ref as R
from dist_helpers import free_port, run_dist

ROOT = Path(__file__).resolve().parent.parent
SIZES = [1, 31, 32, 33, 2047, 2048, 2049, 3 * 2048 + 5]
KEEPS = [1, 5, 32, 256]
LENET_FLAT = 52160  # LeNet's 51,902 parameters, each tensor's slot padded to 64 elements
FILL = 0xA5


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and (_bits(a) == _bits(b)).all()


def encode(g, r, keep):
    """numpy in, numpy out: (payload bytes, new residual or None) from the torch path."""
    from dmlab.parallel.compress import topk_encode_torch, topk_payload_bytes

    n = g.shape[0]
    assert topk_payload_bytes(n, keep) == R.payload_bytes(n, keep)
    payload = torch.full((topk_payload_bytes(n, keep),), FILL, dtype=torch.uint8)
    rt = None if r is None else _t(r).clone()
    g_in = _t(g).clone()
    topk_encode_torch(g_in, rt, payload, keep)
    assert _same_bits(g_in.numpy(), g)  # the gradient is read only
    return payload.numpy(), (None if rt is None else rt.numpy())


def want_encode(g, r, keep):
    vals, idx, rn = R.encode_ref(g, r, keep)
    return R.join_payload(vals, idx, g.shape[0], FILL), rn


def decode(payloads, n, c, keep):
    from dmlab.parallel.compress import topk_decode_mean_torch

    out = torch.full((n,), 7.0)
    topk_decode_mean_torch(_t(np.stack(payloads)), out, c, keep)
    return out.numpy()


# ------------------------------------------------------------------ layout
def test_payload_bytes_layout():
    from dmlab.parallel.compress import (Q8Compressor, TopKCompressor, payload_bytes,
                                         topk_n_blocks, topk_payload_bytes)

    for n in SIZES + [51902, LENET_FLAT, 300001, 11_700_000]:
        for keep in KEEPS:
            pb = topk_payload_bytes(n, keep)
            assert pb == R.payload_bytes(n, keep) and pb % 16 == 0
            assert topk_n_blocks(n) == R.n_blocks(n)
            assert 0 <= pb - 6 * R.n_blocks(n) * keep < 16
    assert abs(4 * 2048 * 1000 / topk_payload_bytes(2048 * 1000, 32) - 42.67) < 0.01
    assert abs(4 * 2048 * 1000 / topk_payload_bytes(2048 * 1000, 256) - 5.33) < 0.01
    assert TopKCompressor(100, "cpu", keep=5).payload_bytes(100) == topk_payload_bytes(100, 5)
    assert Q8Compressor(100, "cpu").payload_bytes(100) == payload_bytes(100)
    for bad in (0, 257, -1):
        with pytest.raises(ValueError, match="keep"):
            topk_payload_bytes(100, bad)
        with pytest.raises(ValueError, match="keep"):
            TopKCompressor(100, "cpu", keep=bad)


# ------------------------------------------------------------------ the mirror == the reference
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("ef", [True, False], ids=["ef", "noef"])
def test_torch_path_equals_reference(n, keep, ef):
    g, r0 = R.random_pair(n, seed=n + keep)
    r0 = r0 if ef else None
    got_p, got_r = encode(g, r0, keep)
    want_p, want_r = want_encode(g, r0, keep)
    assert _same_bits(got_p, want_p)  # values, indices and the untouched padding
    if ef:
        assert _same_bits(got_r, want_r)
    else:
        assert got_r is None


@pytest.mark.parametrize("keep", [1, 32, 256])
def test_special_blocks(keep):
    g, d = R.special_blocks()
    n = d["n"]
    r0 = np.zeros(n, np.float32)
    payload, r = encode(g, r0, keep)
    want_p, want_r = want_encode(g, r0, keep)
    assert _same_bits(payload, want_p) and _same_bits(r, want_r)
    vals, idx = R.split_payload(payload, n, keep)
    # equal magnitudes with mixed signs: the first K indices
    assert (idx[d["ties"]] == np.arange(keep)).all()
    assert _same_bits(vals[d["ties"]], g[:keep])
    # fewer than K non-zeros: the non-zeros plus the lowest-index zeros (of either sign)
    nz = [5, 700, 2047]
    want = sorted((nz + [i for i in range(R.B) if i not in nz])[:keep]) if keep >= 3 else \
        sorted([700, 2047][:keep])
    assert idx[d["zeros"]].tolist() == want
    # a NaN and an Inf are both sent (NaN first in rank, so K = 1 sends the NaN)
    sent = idx[d["nonfinite"]].tolist()
    assert 100 in sent and (keep == 1 or 1900 in sent)
    assert np.isnan(vals[d["nonfinite"]][sent.index(100)])
    # denormals are ordered like any other value
    assert 77 in idx[d["denormal"]].tolist()
    # m = 5 < K: the unused slots
    tail_i, tail_v = idx[d["tail"]], vals[d["tail"]]
    k5 = min(keep, 5)
    assert (tail_i[k5:] == R.UNUSED).all() and (_bits(tail_v[k5:]) == 0).all()
    if keep >= 5:
        assert tail_i[:5].tolist() == [0, 1, 2, 3, 4] and _same_bits(tail_v[:5], g[-5:])
        assert (_bits(r[-5:]) == 0).all()
    # the residual is +0.0 exactly where an entry was sent, e elsewhere
    sel = np.zeros(n, bool)
    for b in range(R.n_blocks(n)):
        used = idx[b] != R.UNUSED
        sel[b * R.B + idx[b][used].astype(np.int64)] = True
    e = g + r0  # fp32; -0.0 + 0.0 is +0.0
    assert (_bits(r[sel]) == 0).all() and _same_bits(r[~sel], e[~sel])
    # a non-finite entry decodes to a non-finite value on every rank
    out = decode([payload, payload], n, 0.5, keep)
    assert np.isnan(out[2 * R.B + 100])


# ------------------------------------------------------------------ decode-mean
def test_decode_order_is_rank_order():
    """Three ranks list one element with 2^24, 1, -2^24: rank order gives (2^24 + 1) - 2^24 =
    0 in fp32 (2^24 + 1 rounds to 2^24), any other order gives 1."""
    n, keep = 2049, 1
    rows = []
    for v in (2.0 ** 24, 1.0, -2.0 ** 24):
        g = np.zeros(n, np.float32)
        g[1234] = v
        g[2048] = v
        rows.append(encode(g, None, keep)[0])
    out = decode(rows, n, 1.0, keep)
    assert out[1234] == 0.0 and out[2048] == 0.0 and (out == 0).all()
    assert decode([rows[0], rows[2], rows[1]], n, 1.0, keep)[1234] == 1.0


@pytest.mark.parametrize("ws", [1, 2, 3, 8])
@pytest.mark.parametrize("keep", [1, 32])
def test_decode_mean_against_reference(ws, keep):
    n = 3 * 2048 + 5
    rows, total = [], np.zeros(n)
    rand = []
    for rk in range(ws):
        g, ints = R.small_ints(n, rk - 3, seed=10 + rk)
        p, _ = encode(g, None, keep)
        rows.append(p)
        vals, idx, _ = R.encode_ref(g, None, keep)
        sent = np.zeros(n)
        for b in range(R.n_blocks(n)):
            used = idx[b] != R.UNUSED
            sent[b * R.B + idx[b][used].astype(np.int64)] = vals[b][used]
        total += sent
        rand.append(encode(R.random_normal(n, 20 + rk) * (1 + rk), None, keep)[0])
    for c in (1.0, 1.0 / ws):
        c32 = np.float64(np.float32(c))
        # sums of small integers times powers of two are exact, then one fp32 rounding
        assert (decode(rows, n, c, keep) == (total * c32).astype(np.float32)).all()
        v, i = R.split_payload(np.stack(rand), n, keep)
        want = R.decode_mean_ref(v, i, n, c32)
        got = decode(rand, n, c, keep)
        assert np.abs(got - want).max() <= ws * 2.0 ** -23 * np.abs(want).max()
        assert (got[want == 0] == 0).all()  # every element is written, zeros included


# ------------------------------------------------------------------ error feedback
def test_conservation_is_exact():
    """Gradients that are small integers times a power of two: every sum below is exact in
    fp32, so after T steps  sum_t decoded_t + r_T == sum_t g_t  element for element.  Without
    error feedback what is not sent is lost."""
    from dmlab.parallel.compress import TopKCompressor, topk_payload_bytes

    n, keep, T = 2 * 2048 + 100, 32, 5
    for ef in (True, False):
        comp = TopKCompressor(n, "cpu", keep=keep, error_feedback=ef)
        sent, fed = np.zeros(n, np.float64), np.zeros(n, np.float64)
        for t in range(T):
            g, _ = R.small_ints(n, -6, seed=100 + t)
            payload = torch.zeros(topk_payload_bytes(n, keep), dtype=torch.uint8)
            out = torch.empty(n)
            comp.encode(_t(g), 0, payload)
            comp.decode_mean(payload.view(1, -1), out, 1.0)
            sent += out.numpy()
            fed += g
        if ef:
            assert (sent + comp.residual.numpy() == fed).all()
            assert comp.residual.abs().max() > 0
        else:
            assert comp.residual is None
            assert (sent != fed).any()


def test_compressor_state_dict_roundtrip_and_bucket_slices():
    from dmlab.parallel.compress import TopKCompressor, topk_payload_bytes

    n, keep = 5000, 5
    a, b = TopKCompressor(n, "cpu", keep=keep), TopKCompressor(n, "cpu", keep=keep)
    lo, m = 1280, 2500  # a bucket inside the buffer: its blocks count from lo
    g = R.random_normal(m, seed=2)
    payload = torch.zeros(topk_payload_bytes(m, keep), dtype=torch.uint8)
    a.encode(_t(g), lo, payload)
    want_p, want_r = want_encode(g, np.zeros(m, np.float32), keep)
    assert _same_bits(payload.numpy()[:6 * 2 * keep], want_p[:6 * 2 * keep])
    assert _same_bits(a.residual.numpy()[lo:lo + m], want_r)
    assert a.residual[:lo].abs().max() == 0 and a.residual[lo + m:].abs().max() == 0
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.residual, b.residual)
    with pytest.raises(ValueError):
        TopKCompressor(n, "cpu", keep=keep, error_feedback=False).load_state_dict(a.state_dict())
    with pytest.raises(ValueError):
        TopKCompressor(n + 1, "cpu", keep=keep).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="outside"):
        a.encode(_t(g), n - 10, payload)


# ------------------------------------------------------------------ gloo ranks
def _data(ws, per, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(ws * per, 1, 28, 28, generator=g),
            torch.randint(0, 10, (ws * per,), generator=g))


def _simulate(ws, steps, bounds, X, Y, per, c, grad_scale, keep, ef=True):
    """One process plays every rank: each rank's gradient of the shared weights, then the torch
    codec by hand per bucket (encode with that rank's residual, stack, decode-mean), then SGD.
    Returns (flat parameters, per-rank residuals, the last decoded gradient)."""
    from dmlab.models import Net
    from dmlab.optim import SGD
    from dmlab.parallel.compress import (topk_decode_mean_torch, topk_encode_torch,
                                         topk_payload_bytes)

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
        out = grads[0].clone()
        for lo, hi in bounds:
            rows = torch.zeros((ws, topk_payload_bytes(hi - lo, keep)), dtype=torch.uint8)
            for rk in range(ws):
                topk_encode_torch(grads[rk][lo:hi], res[rk][lo:hi] if ef else None, rows[rk], keep)
            topk_decode_mean_torch(rows, out[lo:hi], c, keep)
        model.flat.grad.copy_(out)
        opt.step()
    return model.flat.data.clone(), res, out


def _same_on_every_rank(t, ws):
    import torch.distributed as dist

    rows = [torch.empty_like(t) for _ in range(ws)]
    dist.all_gather(rows, t.contiguous())
    for r in rows:
        assert torch.equal(r, rows[0])


def _ddp_topk(rank, ws, ef, keep):
    from dmlab.models import Net
    from dmlab.optim import SGD
    from dmlab.parallel import DDP
    from dmlab.parallel.compress import TopKCompressor, topk_payload_bytes

    per, steps = 6, 3
    X, Y = _data(ws, per)
    torch.manual_seed(0)
    model = Net()
    ddp = DDP(model, bucket_cap_mb=0.05, first_bucket_mb=0.01, compress="topk",
              compress_keep=keep, error_feedback=ef)
    assert len(ddp.buckets) >= 2 and ddp._native is None
    assert isinstance(ddp.compressor, TopKCompressor) and ddp.compressor.keep == keep
    assert (ddp.compressor.residual is not None) == ef
    opt = ddp.fold_average_into(SGD(model.parameters(), lr=0.1, momentum=0.9))
    for _ in range(steps):
        opt.zero_grad()
        F.cross_entropy(ddp(X[rank * per:(rank + 1) * per]), Y[rank * per:(rank + 1) * per]).backward()
        last = model.flat.grad.clone()
        opt.step()
    assert ddp.buckets_launched == steps * len(ddp.buckets)
    assert ddp.comm_bytes_per_step == sum(topk_payload_bytes(b.hi - b.lo, keep)
                                          for b in ddp.buckets)
    want, res, want_grad = _simulate(ws, steps, [(b.lo, b.hi) for b in ddp.buckets], X, Y, per,
                                     1.0, 1.0 / ws, keep, ef)
    assert torch.equal(last, want_grad)  # the codec by hand, bit for bit
    assert torch.equal(model.flat.data, want)
    _same_on_every_rank(model.flat.data, ws)
    if ef:
        assert torch.equal(ddp.compressor.residual, res[rank])
        # residual_state is a collective: every rank's row, and it loads back bit for bit
        rows = ddp.residual_state()
        assert rows.shape == (ws, model.flat.grad.numel())
        for rk in range(ws):
            assert torch.equal(rows[rk], res[rk])
        ddp.compressor.residual.zero_()
        assert ddp.load_residual_state(rows)
        assert torch.equal(ddp.compressor.residual, res[rank])
        assert not ddp.load_residual_state(rows[:1])
    else:
        assert ddp.residual_state() is None


def test_ddp_topk_two_ranks_bit_identical_to_codec_by_hand():
    run_dist(_ddp_topk, 2, True, 32)


def test_ddp_topk_without_error_feedback_keep_5():
    run_dist(_ddp_topk, 2, False, 5)


def _no_sync_and_aggregator(rank, ws, _):
    from dmlab.models import Net
    from dmlab.optim import SGD
    from dmlab.parallel import DDP, comm
    from dmlab.parallel.compress import topk_payload_bytes

    torch.manual_seed(0)
    model = Net()
    ddp = DDP(model, bucket_cap_mb=0.05, first_bucket_mb=0.01, compress="topk")
    X, Y = _data(ws, 4, seed=5)
    xs, ys = X[rank * 4:(rank + 1) * 4], Y[rank * 4:(rank + 1) * 4]
    with ddp.no_sync():
        F.cross_entropy(ddp(xs), ys).backward()
    assert ddp.buckets_launched == 0 and ddp.compressor.residual.abs().max() == 0
    F.cross_entropy(ddp(xs * 0.5), ys).backward()  # accumulates, then reduces once
    assert ddp.buckets_launched == len(ddp.buckets)
    _same_on_every_rank(model.flat.grad, ws)
    # the aggregator: one flat bucket
    per, steps, keep = 6, 3, 5
    X, Y = _data(ws, per)
    torch.manual_seed(0)
    model = Net()
    agg = comm.GradAggregator(model, "allgather_topk", keep=keep)
    n = model.flat.grad.numel()
    assert n == LENET_FLAT and agg.bytes_per_call == topk_payload_bytes(n, keep)
    with pytest.raises(ValueError, match="flat"):
        comm.GradAggregator(model, "allgather_topk", granularity="per_param")
    with pytest.raises(ValueError, match="keep"):
        comm.GradAggregator(model, "allgather_topk", keep=0)
    opt = SGD(model.parameters(), lr=0.1, momentum=0.9)
    for _ in range(steps):
        opt.zero_grad()
        F.cross_entropy(model(X[rank * per:(rank + 1) * per]), Y[rank * per:(rank + 1) * per]).backward()
        agg()
        opt.step()
    want, res, _ = _simulate(ws, steps, [(0, n)], X, Y, per, 1.0 / ws, 1.0, keep)
    assert torch.equal(model.flat.data, want)
    assert torch.equal(agg.compressor.residual, res[rank])
    _same_on_every_rank(model.flat.data, ws)


def test_ddp_topk_no_sync_reduces_once_and_aggregator():
    run_dist(_no_sync_and_aggregator, 2, None)


def test_ddp_compress_topk_argument_checks():
    from dmlab.models import Net
    from dmlab.parallel import DDP

    with pytest.raises(ValueError, match="comm_dtype"):
        DDP(Net(), compress="topk", comm_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="xgmi"):
        DDP(Net(), compress="topk", small_allreduce="xgmi")
    with pytest.raises(ValueError, match="keep"):
        DDP(Net(), compress="topk", compress_keep=257)
    with pytest.raises(ValueError, match="keep"):
        DDP(Net(), compress="topk", compress_keep=0)
    with pytest.raises(ValueError):
        DDP(Net(), compress="top-k")
    one = DDP(Net(), compress="topk")  # one rank, no communication: nothing to compress
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


def test_task2_allgather_topk_two_ranks(tmp_path):
    from dmlab.parallel.compress import topk_payload_bytes

    base = ["-m", "dmlab.tasks.task2", "--device", "cpu", "--synthetic", "--train-samples", "1280",
            "--epochs", "1", "--max-steps", "20", "--no-test"]
    out = _run(_torchrun(2) + base + ["--aggregation", "allgather_topk", "--json",
                                      str(tmp_path / "k.json")], tmp_path)
    m = re.search(r"Total communication time: [\d.eE+-]+\nCommunication bytes per step: (\d+)\n",
                  out)
    assert m and int(m.group(1)) == topk_payload_bytes(LENET_FLAT, 32)
    js = json.loads((tmp_path / "k.json").read_text())
    assert js["comm_bytes_per_step"] == topk_payload_bytes(LENET_FLAT, 32)
    assert js["aggregation"] == "allgather_topk"
    assert 40 < 4 * LENET_FLAT / topk_payload_bytes(LENET_FLAT, 32) < 42.7
    # one rank with the collectives forced, K = 5, residual off
    out = _run(base + ["--aggregation", "allgather_topk", "--compress-keep", "5",
                       "--no-error-feedback", "--backend", "gloo", "--force-comm",
                       "--master_port", str(free_port())], tmp_path)
    assert f"Communication bytes per step: {topk_payload_bytes(LENET_FLAT, 5)}" in out
    err = _run(base + ["--aggregation", "allgather_topk", "--granularity", "per_param",
                       "--master_port", str(free_port())], tmp_path, ok=False)
    assert "granularity must be 'flat'" in err
    err = _run(base + ["--aggregation", "allgather_topk", "--compress-keep", "300",
                       "--master_port", str(free_port())], tmp_path, ok=False)
    assert "keep must be in 1..256" in err


def _uninterrupted(rank, ws, path):
    """What `task3 --compress topk` computes on the CPU when one epoch is run, saved, resumed and
    run again (a resumed run starts at epoch 0 of the sampler), but in one process with no
    checkpoint in between: the same model, data, sampler, optimiser and DDP, trained twice."""
    from dmlab.data import DeviceLoader, MySampler, load_mnist
    from dmlab.models import Net
    from dmlab.nn import CrossEntropyLoss
    from dmlab.optim import SGD
    from dmlab.parallel import DDP
    from dmlab.tasks import task3
    from dmlab.tasks.common import train

    a = task3.parse_args(["--lr", "0.01", "--compress", "topk"])
    torch.manual_seed(4321 + rank)
    model = Net(1, 10)
    train_set = load_mnist(a.data, True, synthetic=True, n=192)
    loader = DeviceLoader(train_set, a.batch_size,
                          sampler=MySampler(train_set, ws, rank, shuffle=True, seed=0,
                                            mode=a.sampler))
    opt = SGD(model.parameters(), lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay)
    net = DDP(model, bucket_cap_mb=a.bucket_mb, compress="topk", compress_keep=a.compress_keep)
    net.fold_average_into(opt)
    for _ in range(2):
        train(net, loader, CrossEntropyLoss(0.0), opt, 1, rank=rank, batch_size=a.batch_size,
              print_fn=lambda *x, **k: None)
    rows = net.residual_state()
    if rank == 0:
        torch.save({"model": {k: v.detach().clone() for k, v in model.state_dict().items()},
                    "residual": rows}, path)


def test_task3_compress_topk_save_resume_continues_bit_equal(tmp_path):
    """--save writes every rank's residual as topk_residual; a run of one epoch (3 steps) that is
    saved, resumed and run for one more ends with the parameters and the residuals of the same
    six steps taken without the interruption."""
    base = ["-m", "dmlab.tasks.task3", "--device", "cpu", "--synthetic", "--train-samples", "192",
            "--compress", "topk", "--no-test", "--lr", "0.01"]
    ck1, ck2, ck3, whole = (str(tmp_path / f) for f in ("a.pt", "b.pt", "c.pt", "whole.pt"))
    _run(_torchrun(2) + base + ["--epochs", "1", "--save", ck1, "--json",
                                str(tmp_path / "t3.json")], tmp_path)
    _run(_torchrun(2) + base + ["--epochs", "1", "--resume", ck1, "--save", ck3], tmp_path)
    run_dist(_uninterrupted, 2, whole)
    c, w = torch.load(ck3, weights_only=True), torch.load(whole, weights_only=True)
    for k, v in w["model"].items():
        assert torch.equal(c["model"][k], v), k
    assert torch.equal(c["extra"]["topk_residual"], w["residual"])
    js = json.loads((tmp_path / "t3.json").read_text())
    from dmlab.parallel.compress import topk_payload_bytes

    assert js["compress"] == "topk"
    assert 0 < js["comm_bytes_per_step"] <= topk_payload_bytes(LENET_FLAT, 32) + 6 * 32 * 8
    a = torch.load(ck1, weights_only=True)
    ra = a["extra"]["topk_residual"]
    assert "q8_residual" not in a["extra"]
    assert ra.shape == (2, LENET_FLAT) and ra[0].abs().max() > 0 and not torch.equal(ra[0], ra[1])
    # zero further epochs: saves exactly what it loaded
    _run(_torchrun(2) + base + ["--epochs", "0", "--resume", ck1, "--save", ck2], tmp_path)
    assert torch.equal(torch.load(ck2, weights_only=True)["extra"]["topk_residual"], ra)
    # a checkpoint of the other codec is reported, not loaded
    out = _run(_torchrun(2) + [x if x != "topk" else "q8" for x in base]
               + ["--epochs", "0", "--resume", ck1], tmp_path)
    assert "not restored" in out
    for bad in (["--dp", "manual"], ["--allreduce", "xgmi"]):
        assert "--compress topk" in _run(base + bad + ["--master_port", str(free_port())],
                                         tmp_path, ok=False)
    assert "--compress-keep" in _run(
        [x if x != "topk" else "q8" for x in base] + ["--compress-keep", "8", "--master_port",
                                                      str(free_port())], tmp_path, ok=False)
