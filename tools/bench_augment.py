"""Device time of the augmentation kernel (csrc/augment.hip) and its cost inside a step.

(a) ``kernel``: one ``augment_apply`` call at batch 1024, 224 x 224 x 3 uint8 with random-
resized-crop parameters, against ``images.index_select(0, idx)`` of the same batch (the gather
this kernel replaces).  The two alternate in one process; each sample is ``--group`` calls
between two HIP events, ``--rounds`` samples each after a warm-up.  Reported: median / min /
max ms per call and GB/s of output bytes.

(b) ``step``: ResNet-18 bf16 training steps at batch 1024 fed by ``DeviceLoader`` without a
transform (``iter_gathered``: the stem gathers the rows itself) and with the rrc transform,
as ``--pairs`` interleaved (plain, augmented) measurements of ``--steps`` steps each.

Each part writes one text file (``--out-dir``): ``augment_kernel.txt`` and
``augment_step_ab.txt``.  Needs a GPU.

    python tools/bench_augment.py [--part kernel|step|both] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dmlab.data import DeviceAugment, DeviceLoader, SyntheticImageNet  # noqa: E402
from dmlab.ops._native import lib  # noqa: E402


def _timed(fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def _stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
            "max_ms": round(max(v), 4)}


def bench_kernel(a, dev):
    ds = SyntheticImageNet(a.dataset, a.res, 1000, device=dev, dtype=torch.uint8, seed=0)
    im = ds.images  # (N,3,H,W) channels_last
    aug = DeviceAugment.random_resized_crop(a.res, flip=0.5, seed=1, size=(a.res, a.res))
    g = torch.Generator().manual_seed(0)
    idx_h = torch.randperm(a.dataset, generator=g)[: a.batch]
    idx, par = idx_h.to(dev), aug.params(idx_h, 0).to(dev)
    # both as the loader calls them: a fresh output tensor per call (caching allocator)
    runs = {"augment_apply": lambda: aug.apply(im, idx, par),
            "index_select": lambda: im.index_select(0, idx)}
    lib()  # fail loudly if the extension is missing
    for f in runs.values():
        _timed(f, 20)
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, f in runs.items():
            times[k].append(_timed(f, a.group))
    nbytes = a.batch * a.res * a.res * 3
    lines = [f"# tools/bench_augment.py --part kernel: {torch.cuda.get_device_name(0)}",
             f"# batch {a.batch}, {a.res}x{a.res}x3 uint8 from a {a.dataset}-image dataset, rrc "
             f"parameters (scale 0.08-1, flip 0.5); {a.rounds} alternating samples of {a.group} "
             f"calls = {a.rounds * a.group} calls each; output {nbytes / 1e6:.1f} MB per call"]
    res = {}
    for k, v in times.items():
        s = _stat(v)
        s["out_GBps"] = round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 1)
        res[k] = s
        lines.append(f"{k:14s} median {s['median_ms']:.4f} ms  min {s['min_ms']:.4f}  max "
                     f"{s['max_ms']:.4f}  {s['out_GBps']:.1f} GB/s of output")
    ratio = res["augment_apply"]["median_ms"] / res["index_select"]["median_ms"]
    lines.append(f"augment_apply / index_select = {ratio:.2f}x")
    lines.append(json.dumps(res))
    return lines


def bench_step(a, dev):
    from dmlab.models import ResNet18
    from dmlab.nn import cross_entropy
    from dmlab.optim import SGD

    ds = SyntheticImageNet(a.dataset, a.res, 1000, device=dev, dtype=torch.uint8, seed=0)
    aug = DeviceAugment.random_resized_crop(a.res, flip=0.5, seed=1)
    loaders = {"plain": DeviceLoader(ds, a.batch, shuffle=True, drop_last=True),
               "augment": DeviceLoader(ds, a.batch, shuffle=True, drop_last=True, transform=aug)}
    torch.manual_seed(0)
    model = ResNet18(num_classes=1000).to(dev)
    opt = SGD(model.parameters(), lr=0.01, momentum=0.9)
    state = {k: {"epoch": 0, "it": None} for k in loaders}

    def batch(k):
        st = state[k]
        while True:
            if st["it"] is None:
                loaders[k].set_epoch(st["epoch"])
                st["epoch"] += 1
                st["it"] = loaders[k].iter_gathered()
            try:
                return next(st["it"])
            except StopIteration:
                st["it"] = None

    def step(k):
        x, y = batch(k)
        loss = cross_entropy(model(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()

    for k in loaders:
        _timed(lambda: step(k), a.warmup)
    times = {k: [] for k in loaders}
    for _ in range(a.pairs):
        for k in loaders:
            _timed(lambda: step(k), 2)
            times[k].append(_timed(lambda: step(k), a.steps))
    lines = [f"# tools/bench_augment.py --part step: {torch.cuda.get_device_name(0)}",
             f"# ResNet-18 bf16 training step, batch {a.batch}, {a.res}x{a.res} uint8 from a "
             f"{a.dataset}-image device-resident dataset; {a.pairs} interleaved pairs of "
             f"{a.steps} steps (ms per step)"]
    for i in range(a.pairs):
        p, q = times["plain"][i], times["augment"][i]
        lines.append(f"pair {i}: plain {p:.3f} ms  augment {q:.3f} ms  diff {q - p:+.3f} ms")
    mp, mq = statistics.median(times["plain"]), statistics.median(times["augment"])
    spread = max(max(v) - min(v) for v in times.values())
    lines.append(f"median: plain {mp:.3f} ms  augment {mq:.3f} ms  diff {mq - mp:+.3f} ms  "
                 f"(largest spread inside one arm {spread:.3f} ms)")
    lines.append(json.dumps({"plain_ms": [round(t, 4) for t in times["plain"]],
                             "augment_ms": [round(t, 4) for t in times["augment"]]}))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", default="both", choices=["kernel", "step", "both"])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--dataset", type=int, default=4096, help="images in the resident dataset")
    ap.add_argument("--group", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out-dir", default="profiles")
    a = ap.parse_args(argv)
    if a.rounds * a.group < 200 or a.pairs < 3:
        raise SystemExit("time at least 200 calls (--rounds x --group) and 3 pairs")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(a.out_dir, exist_ok=True)
    for part, fn, name in (("kernel", bench_kernel, "augment_kernel.txt"),
                           ("step", bench_step, "augment_step_ab.txt")):
        if a.part in (part, "both"):
            lines = fn(a, dev)
            with open(os.path.join(a.out_dir, name), "w") as f:
                f.write("\n".join(lines) + "\n")
            print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
