"""The two gradient codecs' kernels on one bucket, side by side.

    python tools/bench_codec.py [--numel 6553600] [--keep 32] [--rows 2] [--reps 200]
                                [--out profiles/codec_topk_<tag>.txt]

HIP-event timings of ``q8_encode`` / ``topk_encode`` (with the residual, as training runs them)
and of ``q8_decode_mean`` / ``topk_decode_mean`` over ``--rows`` locally filled rows on one
bucket of ``--numel`` fp32 elements (default: DDP's 25 MB ResNet-18 bucket).  After a warm-up,
every round times each kernel once, in turn (``--inner`` back-to-back calls between two
events), so the kernels see the same machine state; the figure is the median over ``--reps``
rounds.  One JSON line per kernel:

    {"kernel": ..., "numel": n, "us": median us per call, "min_us": ..., "gbps": ...}

``gbps`` is the traffic of the gradient-sized arrays over the median time: ``g`` + ``r`` read
and ``r`` written (12 B/element) for the encoders, ``out`` written (4 B/element) for the
decoders; the payloads are left out so that both codecs are rated on the same bytes.
``topk_vs_q8`` on the topk lines is the time ratio to the q8 kernel of the same round.  The
gradient is random normal data, and each encoder carries its residual from call to call as
training does: topk's selection cost depends on how many elements share the threshold's
leading key bits, so the median is the error-feedback steady state (what is not sent piles up
below the threshold) and ``min_us`` is the first rounds, where the residual is still zero.
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
    ap.add_argument("--numel", type=int, default=25 * 2**20 // 4)
    ap.add_argument("--keep", type=int, default=32)
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 50:
        raise SystemExit("--reps: at least 50 rounds for a median worth quoting")
    if not torch.cuda.is_available():
        raise SystemExit("bench_codec needs a HIP device")
    from dmlab.ops._native import lib
    from dmlab.parallel.compress import payload_bytes, topk_payload_bytes

    L = lib()
    dev = torch.device("cuda", 0)
    n, K, ws = a.numel, a.keep, a.rows
    torch.manual_seed(0)
    g = torch.randn(n, device=dev) * 1e-3
    rq = torch.zeros(n, device=dev)
    rk = torch.zeros(n, device=dev)
    pq = torch.zeros(payload_bytes(n), dtype=torch.uint8, device=dev)
    pk = torch.zeros(topk_payload_bytes(n, K), dtype=torch.uint8, device=dev)
    L.q8_encode(g, None, pq)
    L.topk_encode(g, None, pk, K)
    gq = pq.expand(ws, -1).contiguous()
    gk = pk.expand(ws, -1).contiguous()
    out = torch.empty(n, device=dev)
    variants = {
        "q8_encode": (lambda: L.q8_encode(g, rq, pq), 12 * n),
        "topk_encode": (lambda: L.topk_encode(g, rk, pk, K), 12 * n),
        "q8_decode_mean": (lambda: L.q8_decode_mean(gq, out, 1.0 / ws), 4 * n),
        "topk_decode_mean": (lambda: L.topk_decode_mean(gk, out, K, 1.0 / ws), 4 * n),
    }
    for _ in range(a.warmup):
        for f, _b in variants.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, (f, _b) in variants.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.inner * 1e3)  # us per call
    assert bool(torch.isfinite(out).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = []
    for k, (_f, nbytes) in variants.items():
        row = dict(kernel=k, numel=n, keep=K if k.startswith("topk") else None,
                   rows=ws if "decode" in k else None, us=round(med[k], 2),
                   min_us=round(min(times[k]), 2), gbps=round(nbytes / med[k] / 1e3, 1),
                   reps=a.reps, device=torch.cuda.get_device_name(0))
        if k.startswith("topk"):
            row["topk_vs_q8"] = round(med[k] / med[k.replace("topk", "q8")], 3)
        lines.append(json.dumps({k2: v for k2, v in row.items() if v is not None}))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return text


if __name__ == "__main__":
    main()
