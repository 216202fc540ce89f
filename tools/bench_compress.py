"""The q8 gradient codec's two kernels, timed next to the streaming kernels they sit beside.

    python tools/bench_compress.py [--reps 100] [--out profiles/gradq_kernels.txt]

For n = 51,902 (LeNet's gradients) and n = 11.7 M (ResNet-18's): ``q8_encode`` with and
without the residual, ``q8_decode_mean`` over 1, 2 and 8 locally filled rows (no collective
runs), and on the same n in the same process the yardsticks ``cast_f32_bf16`` (the bf16
communication path's pack) and ``rows_mean`` (the fp32 all-gather path's reduction).  Every
round times each variant once (``--inner`` back-to-back calls between two HIP events, more
for the small n); the figure is the median over ``--reps`` rounds, given as microseconds per
call and as GB/s of the bytes the kernel has to move:

    encode      g 4n (+ residual read 4n and write 4n) + codes n + scales 4*ceil(n/256)
    decode      rows * (n + 4*ceil(n/256)) + out 4n
    cast        4n + 2n
    rows_mean   rows * 4n + 4n

Both sizes fit the 256 MiB Infinity Cache, so these are cache-assisted rates, not HBM rates; the
ratios to the yardsticks (same n, same cache state) are what the table is for.  Whether
compression pays end to end depends on the links between several GPUs, which this does not
measure.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

SIZES = (("lenet", 51_902), ("resnet18", 11_700_000))
ROWS = (1, 2, 8)


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
        raise SystemExit("bench_compress needs a HIP device")
    from dmlab.ops._native import lib
    from dmlab.parallel.compress import n_blocks, payload_bytes

    L = lib()
    dev = torch.device("cuda", 0)
    lines = [f"q8 codec kernels on {torch.cuda.get_device_name(0)}: median of {a.reps} rounds, "
             f"events around back-to-back calls", ""]
    lines.append(f"{'n':>10} {'kernel':<22} {'us/call':>10} {'min us':>10} {'MB moved':>10} "
                 f"{'GB/s':>9}")
    ratios = []
    for name, n in SIZES:
        inner = a.inner if n > 1_000_000 else a.inner * 10
        torch.manual_seed(0)
        g = torch.randn(n, device=dev) * 1e-3
        r = torch.zeros(n, device=dev)
        pb, nb = payload_bytes(n), n_blocks(n)
        payload = torch.zeros(pb, dtype=torch.uint8, device=dev)
        gathered = torch.zeros((max(ROWS), pb), dtype=torch.uint8, device=dev)
        L.q8_encode(g, None, payload)
        gathered.copy_(payload.expand(max(ROWS), pb))
        out = torch.empty(n, device=dev)
        bf = torch.empty(n, dtype=torch.bfloat16, device=dev)
        rows32 = torch.randn(max(ROWS), n, device=dev)
        variants = {
            "q8_encode (residual)": (lambda: L.q8_encode(g, r, payload), 13 * n + 4 * nb),
            "q8_encode (none)": (lambda: L.q8_encode(g, None, payload), 5 * n + 4 * nb),
            "cast_f32_bf16": (lambda: L.cast_f32_bf16(g, bf), 6 * n),
        }
        for ws in ROWS:
            variants[f"q8_decode_mean x{ws}"] = (
                lambda ws=ws: L.q8_decode_mean(gathered[:ws], out, 1.0 / ws),
                ws * (n + 4 * nb) + 4 * n)
            variants[f"rows_mean x{ws}"] = (
                lambda ws=ws: L.rows_mean(rows32[:ws], out, 1.0 / ws), ws * 4 * n + 4 * n)
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
                for _ in range(inner):
                    f()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / inner * 1e3)  # us per call
        assert bool(torch.isfinite(out).all())
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, (_f, nbytes) in variants.items():
            lines.append(f"{n:>10} {k:<22} {med[k]:>10.2f} {min(times[k]):>10.2f} "
                         f"{nbytes / 1e6:>10.3f} {nbytes / med[k] / 1e3:>9.1f}")
        lines.append("")
        ratios.append(f"{name} (n = {n}): encode with residual / cast_f32_bf16 = "
                      f"{med['q8_encode (residual)'] / med['cast_f32_bf16']:.2f}x the time, "
                      f"encode without / cast = "
                      f"{med['q8_encode (none)'] / med['cast_f32_bf16']:.2f}x; decode-mean / "
                      "rows_mean = " + ", ".join(
                          f"{med[f'q8_decode_mean x{ws}'] / med[f'rows_mean x{ws}']:.2f}x at "
                          f"{ws} row{'s' if ws > 1 else ''}" for ws in ROWS))
    lines += ["time ratios to the yardsticks (same n, same process):"] + ratios
    lines += ["", "single GPU, rows filled locally: no collective ran, and nothing here says "
              "whether compression pays end to end"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return text


if __name__ == "__main__":
    main()
