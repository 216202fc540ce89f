"""Fused optimiser steps on the ResNet-18 flat buffer: momentum SGD vs LARS.

    python tools/bench_optim.py [--reps 100] [--inner 5] [--out FILE]

Times ``lib().sgd_step`` (momentum, one launch, 20 B/element) and the full LARS step
(``csrc/lars.hip``: partial sums 8 B/element, per-tensor totals, update 20 B/element),
interleaved in one process: every round times each variant once, ``--inner`` back-to-back
calls between two HIP events, and the result is the median over ``--reps`` rounds.  The LARS launches
are also timed one by one to say where the time goes.
Prints one JSON line; ``--out`` also writes it to a file.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 50:
        raise SystemExit("--reps: at least 50 rounds for a median worth quoting")
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim needs a HIP device")
    from dmlab.models import ResNet18
    from dmlab.ops._native import lib
    from dmlab.optim import LARS

    L = lib()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = ResNet18().to(dev)
    flat = model.flat
    n = sum(p.numel() for p in flat.params)
    flat.grad.copy_(torch.randn(flat.numel, device=dev) * 1e-3)
    sgd_buf = torch.zeros_like(flat.data)
    opt = LARS(model.parameters(), lr=0.1, weight_decay=1e-4)

    def sgd():
        L.sgd_step(flat.data, flat.grad, sgd_buf, None, 1e-3, 0.9, 0.0, 0.0, 1.0, False, False)

    def lars(launches):
        def f():
            L.lars_step(flat.data, flat.grad, opt.buf, opt._seg, opt._chunks, opt._hyper,
                        opt._partial, opt._tot, opt._stats, opt._gnorm, False, launches)
        return f

    variants = {"sgd": sgd, "lars": opt.step, "lars_partial": lars(1), "lars_totals": lars(2),
                "lars_update": lars(4)}
    for _ in range(a.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, f in variants.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.inner * 1e3)  # us per call
    assert bool(torch.isfinite(flat.data).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"bench": "optim_resnet18_flat", "elements": n, "flat_numel": flat.numel,
           "chunks": int(opt._chunks.shape[0]), "reps": a.reps, "inner": a.inner}
    for k in variants:
        res[f"{k}_us"] = round(med[k], 2)
        res[f"{k}_us_min"] = round(min(times[k]), 2)
    res["lars_over_sgd"] = round(med["lars"] / med["sgd"], 3)
    res["sgd_tb_s"] = round(20 * n / med["sgd"] / 1e6, 2)
    res["lars_tb_s"] = round(28 * n / med["lars"] / 1e6, 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return res


if __name__ == "__main__":
    main()
