"""Device time of the loss and evaluation kernels (csrc/loss.hip) at the headline head shape.

``cross_entropy`` without and with label smoothing (forward, writing the gradient seed) and
one ``EvalMetrics.update``, each two launches.  A single launch is shorter than an event's
resolution and than the host's enqueue, so ``--calls`` calls are captured into one hipGraph
and a replay is timed with HIP events; the three graphs alternate over ``--rounds`` rounds
after a warm-up and the medians per call are printed as one JSON line.  Needs a GPU.

    python tools/bench_loss.py [--batch 1024] [--classes 1000] [--dtype bf16]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dmlab.nn import EvalMetrics, cross_entropy  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--calls", type=int, default=100, help="calls per captured graph")
    ap.add_argument("--rounds", type=int, default=41)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    x = (torch.randn(a.batch, a.classes, device=dev) * 3).to(
        torch.bfloat16 if a.dtype == "bf16" else torch.float32).requires_grad_(True)
    y = torch.randint(0, a.classes, (a.batch,), device=dev)
    metrics = EvalMetrics(k=5, device=dev)

    def ce(eps):
        def f():
            for _ in range(a.calls):
                cross_entropy(x, y, label_smoothing=eps)
        return f

    def ev():
        xd = x.detach()
        for _ in range(a.calls):
            metrics.update(xd, y)

    graphs = {}
    side = torch.cuda.Stream()
    for name, f in (("ce_eps0", ce(0.0)), ("ce_eps0.1", ce(0.1)), ("eval_update", ev)):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            f()  # eager warm-up: code objects loaded, allocator grown
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            f()
        graphs[name] = g
    for g in graphs.values():
        for _ in range(5):
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for name, g in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            g.replay()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1000.0 / a.calls)
    res = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3),
               "max_us": round(max(v), 3)} for k, v in times.items()}
    res.update(device=torch.cuda.get_device_name(0), batch=a.batch, classes=a.classes,
               dtype=a.dtype, calls_per_graph=a.calls, rounds=a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
