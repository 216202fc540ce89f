"""Device time of the mixing augmentation kernel (csrc/augment_mix.hip).

One call at batch 1024, 224 x 224 x 3 uint8 with random-resized-crop parameters, for

* ``augment_apply``: the unmixed kernel (csrc/augment.hip), the yardstick;
* ``mix_unmixed`` / ``mix_cutmix`` / ``mix_mixup``: ``augment_mix_apply`` with an all-unmixed
  table, an all-CutMix table (α = 1) and an all-mixup table (α = 1);
* ``composite``: what the fused kernel replaces for a mixup batch: two ``augment_apply`` calls
  (the batch and its mirrored partners) and the blend in torch ops.

By load count unmixed and CutMix read one source per pixel (about 1x ``augment_apply``) and
mixup two (about 2x).  The variants alternate in one process; each sample is ``--group`` calls
between two HIP events, ``--rounds`` samples each after a warm-up.  Reported: median / min / max
ms per call, the ratio to ``augment_apply`` and the ratio of ``mix_mixup`` to the composite.
Writes ``<out-dir>/mix_kernel_<tag>.txt``.  Needs a GPU.

    python tools/bench_mix.py [--tag mi355x] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dmlab.data import DeviceAugment, DeviceMix, SyntheticImageNet  # noqa: E402
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


def bench(a, dev):
    ds = SyntheticImageNet(a.dataset, a.res, 1000, device=dev, dtype=torch.uint8, seed=0)
    im = ds.images  # (N,3,H,W) channels_last
    aug = DeviceAugment.random_resized_crop(a.res, flip=0.5, seed=1, size=(a.res, a.res))
    g = torch.Generator().manual_seed(0)
    idx_h = torch.randperm(a.dataset, generator=g)[: a.batch]
    idx, par = idx_h.to(dev), aug.params(idx_h, 0).to(dev)
    out_hw = (a.res, a.res)
    tabs = {"mix_unmixed": DeviceMix(mixup_alpha=1.0, prob=0.0),
            "mix_cutmix": DeviceMix(cutmix_alpha=1.0, seed=1),
            "mix_mixup": DeviceMix(mixup_alpha=1.0, seed=1)}
    mixers, note = {}, []
    for k, m in tabs.items():
        tab, lam = m.params(idx_h, 0, out_hw)
        mixers[k] = (m, tab.to(dev))
        blend = int((tab[:, 1] < 65536).sum())
        boxed = int((tab[:, 2] != 1).sum())
        note.append(f"{k}: {blend} blended rows, {boxed} rows with a box, mean lam "
                    f"{lam.mean().item():.3f}")
    # the composite of a mixup batch: the batch, its mirrored partners, the blend in torch
    L = mixers["mix_mixup"][1][:, 1].float().view(-1, 1, 1, 1)
    ridx, rpar = idx.flip(0).contiguous(), par.flip(0).contiguous()

    def composite():
        xa = aug.apply(im, idx, par)
        xp = aug.apply(im, ridx, rpar)
        return ((L * xa + (65536.0 - L) * xp + 32768.0) * (1.0 / 65536.0)).to(torch.uint8)

    # all as the loader calls them: a fresh output tensor per call (caching allocator)
    runs = {"augment_apply": lambda: aug.apply(im, idx, par)}
    for k, (m, tab) in mixers.items():
        runs[k] = (lambda m=m, tab=tab: m.apply(aug, im, idx, par, tab))
    runs["composite"] = composite
    lib()  # fail loudly if the extension is missing
    same = torch.equal(runs["mix_unmixed"](), runs["augment_apply"]())
    for f in runs.values():
        _timed(f, 20)
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, f in runs.items():
            times[k].append(_timed(f, a.group))
    nbytes = a.batch * a.res * a.res * 3
    lines = [f"# tools/bench_mix.py: {torch.cuda.get_device_name(0)}",
             f"# batch {a.batch}, {a.res}x{a.res}x3 uint8 from a {a.dataset}-image dataset, rrc "
             f"parameters (scale 0.08-1, flip 0.5); {a.rounds} alternating samples of {a.group} "
             f"calls = {a.rounds * a.group} calls each; output {nbytes / 1e6:.1f} MB per call",
             "# " + "; ".join(note),
             f"# mix_unmixed bit-equal to augment_apply: {same}"]
    res = {}
    base = statistics.median(times["augment_apply"])
    for k, v in times.items():
        s = _stat(v)
        s["vs_augment_apply"] = round(s["median_ms"] / base, 3)
        res[k] = s
        lines.append(f"{k:14s} median {s['median_ms']:.4f} ms  min {s['min_ms']:.4f}  max "
                     f"{s['max_ms']:.4f}  {s['vs_augment_apply']:.2f}x augment_apply")
    ratio = res["composite"]["median_ms"] / res["mix_mixup"]["median_ms"]
    lines.append(f"composite / mix_mixup = {ratio:.2f}x")
    lines.append(json.dumps(res))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--dataset", type=int, default=4096, help="images in the resident dataset")
    ap.add_argument("--group", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out-dir", default="profiles")
    a = ap.parse_args(argv)
    if a.rounds * a.group < 200:
        raise SystemExit("time at least 200 calls (--rounds x --group)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(a.out_dir, exist_ok=True)
    lines = bench(a, dev)
    with open(os.path.join(a.out_dir, f"mix_kernel_{a.tag}.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
