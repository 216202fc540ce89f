"""Lab 3 — data parallelism with random-partition / random-sampling data splits.

Reference: codes/task3/model.py — ``MySampler(train_set, n_devices, rank,
shuffle=True, seed=rank)`` (its ``__iter__`` is an unimplemented skeleton,
sampler.py:16-22), batch 32, SGD lr .001 momentum .9, 2 epochs, per-parameter
all-reduce + ``/= ws`` after backward (dist_utils.py:40-46).

Here ``--sampler {partition,random}`` selects the two strategies the lab asks
for (sections/task3.tex:21-23) and ``--dp {ddp,manual}`` selects
bucketed/overlapped DDP (default) or the reference's aggregate-after-backward
loop.  ``--model resnet18`` runs the BASELINE headline CNN (bf16, NHWC).

    torchrun --nproc-per-node 8 -m dmlab.tasks.task3 --sampler random
    python -m dmlab.tasks.task3 --n_devices 2 --rank r --master_addr A   (reference CLI)
"""
from __future__ import annotations

import argparse
import json

import torch

from dmlab.data import DeviceAugment, DeviceLoader, DeviceMix, MySampler, ShardSampler, load_mnist
from dmlab.models import Net, ResNet18
from dmlab.nn import CrossEntropyLoss
from dmlab.optim import LARS, SGD, WarmupPolyLR
from dmlab.parallel import DDP, comm, env
from dmlab.tasks.common import evaluate, test, train


def dist_backend():
    import torch.distributed as dist

    return dist.get_backend() if dist.is_initialized() else None


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n_devices", default=1, type=int)
    p.add_argument("--rank", default=0, type=int)
    p.add_argument("--gpu", default=None, type=str)
    p.add_argument("--master_addr", default="127.0.0.1", type=str)
    p.add_argument("--master_port", default="12355", type=str)
    p.add_argument("--device", default=None, choices=[None, "cpu", "cuda"])
    p.add_argument("--backend", default=None, choices=[None, "nccl", "gloo"])
    p.add_argument("--model", default="lenet", choices=["lenet", "resnet18"])
    p.add_argument("--sampler", "--mode", dest="sampler", default="partition",
                   choices=["partition", "random", "division"])
    p.add_argument("--dp", default="ddp", choices=["ddp", "manual"])
    p.add_argument("--batch-size", type=int, default=32)
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"],
                   help="activation dtype (master weights and gradients stay fp32); "
                        "BASELINE config 3 is bf16.  ResNet-18 always runs bf16")
    p.add_argument("--epochs", type=int, default=2)
    p.add_argument("--lr", type=float, default=0.001)
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "lars"],
                   help="lars: layer-wise adaptive rate scaling (large batches); BN parameters "
                        "and biases are neither adapted nor decayed")
    p.add_argument("--weight-decay", type=float, default=0.0)
    p.add_argument("--trust-coef", type=float, default=0.001, help="LARS trust coefficient")
    p.add_argument("--warmup-steps", type=int, default=0,
                   help="> 0: linear warm-up over this many steps, then polynomial (power 2) "
                        "decay to 0 at the last step; 0 keeps --lr constant")
    p.add_argument("--label-smoothing", type=float, default=0.0,
                   help="train against (1-E)*onehot + E/C (the LARS ResNet recipes use 0.1); "
                        "like --optimizer lars it needs the layer-wise loop")
    p.add_argument("--topk", type=int, default=0,
                   help="> 0: evaluation also reports top-K accuracy and the test loss; 0 "
                        "keeps the reference's top-1 test")
    p.add_argument("--eval", default="rank0", choices=["rank0", "sharded"],
                   help="rank0: rank 0 evaluates the whole test set; sharded: every rank "
                        "evaluates its unpadded shard and the metrics are all-reduced")
    p.add_argument("--augment", default="none", choices=["none", "pad-crop", "rrc"],
                   help="on-device training augmentation, drawn per (seed, dataset index, "
                        "epoch): pad-crop = zero-pad by --aug-pad and crop at a random offset; "
                        "rrc = random resized crop to the image size (evaluation then uses "
                        "the centre crop).  Like --optimizer lars it needs the layer-wise loop")
    p.add_argument("--aug-pad", type=int, default=4, help="pad-crop: padding in pixels")
    p.add_argument("--aug-scale", type=float, nargs=2, default=(0.08, 1.0), metavar=("LO", "HI"),
                   help="rrc: range of the crop's area as a fraction of the image")
    p.add_argument("--aug-flip", type=float, default=None,
                   help="horizontal-flip probability (default 0.5 for resnet18, 0 for lenet)")
    p.add_argument("--aug-seed", type=int, default=0)
    p.add_argument("--mixup", type=float, default=0.0, metavar="A",
                   help="on-device mixup: each sample blended with the one at the mirrored "
                        "batch position, weight ~ Beta(A, A) drawn per (--aug-seed, dataset "
                        "index, epoch); 0 = off.  The loss takes both labels")
    p.add_argument("--cutmix", type=float, default=0.0, metavar="A",
                   help="on-device CutMix: a box of the mirrored sample pasted in, area "
                        "fraction ~ 1 - Beta(A, A); 0 = off.  Like --augment, mixing needs the "
                        "layer-wise loop, and evaluation is unmixed")
    p.add_argument("--mix-prob", type=float, default=1.0, metavar="P",
                   help="probability that a sample is mixed at all")
    p.add_argument("--mix-switch-prob", type=float, default=0.5, metavar="P",
                   help="with --mixup and --cutmix: probability that a mixed sample is CutMix")
    p.add_argument("--bucket-mb", type=float, default=25.0)
    p.add_argument("--allreduce", default="auto", choices=["auto", "rccl", "xgmi"],
                   help="small-bucket all-reduce: RCCL ring or the one-shot xGMI kernel.  At "
                        "world size > 1 on GPUs a startup self-check runs one xGMI call against "
                        "RCCL (exact); auto/xgmi use the kernel for LeNet only if it passes on "
                        "every rank (RCCL otherwise); ResNet-18 stays on RCCL under auto")
    p.add_argument("--compress", default="none", choices=["none", "q8", "topk"],
                   help="q8: DDP exchanges block-wise int8 gradients with error feedback "
                        "(all-gather + decode-mean) instead of all-reducing fp32; topk: the "
                        "--compress-keep largest entries of every 2048-element block as "
                        "(value, index) pairs, with error feedback, on the same path")
    p.add_argument("--no-error-feedback", action="store_true",
                   help="--compress q8 / topk: do not carry the compression error to the next "
                        "step")
    p.add_argument("--compress-keep", type=int, default=32, metavar="K",
                   help="--compress topk: entries kept per 2048-element block (1..256)")
    p.add_argument("--data", default="./data")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--train-samples", type=int, default=None)
    p.add_argument("--max-steps", type=int, default=None)
    p.add_argument("--no-test", action="store_true")
    p.add_argument("--json", default=None)
    p.add_argument("--save", default=None, help="checkpoint path written after training")
    p.add_argument("--resume", default=None, help="checkpoint to load before training")
    p.add_argument("--image-size", type=int, default=64,
                   help="ResNet-18 synthetic image side (224 = the BASELINE/ImageNet shape)")
    p.add_argument("--num-classes", type=int, default=10,
                   help="ResNet-18 classifier width (1000 = the BASELINE/ImageNet head)")
    p.add_argument("--fused", default="auto", choices=["auto", "0", "1"],
                   help="LeNet on the GPU: the fused 2-dispatch training step fed by the "
                        "device-side sampler cursor (auto: on for LeNet + DDP + SGD on a GPU)")
    p.add_argument("--graph-steps", type=int, default=20,
                   help="fused path with --graph: complete training steps per graph replay (a "
                        "divisor of the 20-step log interval; 1 = one replay per step)")
    p.add_argument("--graph", default="auto", choices=["auto", "0", "1"],
                   help="capture the fused step (with its all-reduce) in a hipGraph (auto: "
                        "on when --fused is, unless the group is gloo at ws > 1)")
    p.add_argument("--sync-bn", default="off", choices=["off", "on", "force"],
                   help="resnet18: BatchNorm statistics over every rank's shard (one small "
                        "all-gather per layer and forward, one all-reduce per layer and "
                        "backward, on a process group of their own); force: also at one rank, "
                        "so a one-GPU box runs the multi-rank kernels and collectives")
    a = p.parse_args(argv)
    if a.sync_bn != "off" and a.model == "lenet":
        p.error("--sync-bn needs --model resnet18 (LeNet has no BatchNorm)")
    return a


def main(argv=None):
    a = parse_args(argv)
    if a.fused == "1" and (a.optimizer != "sgd" or a.warmup_steps > 0):
        raise SystemExit("--fused 1 runs constant-rate SGD inside the fused LeNet step; "
                         "--optimizer lars and --warmup-steps need the layer-wise loop "
                         "(--fused auto or 0)")
    if not 0.0 <= a.label_smoothing <= 1.0:
        raise SystemExit("--label-smoothing must be in [0, 1]")
    if a.fused == "1" and a.label_smoothing > 0:
        raise SystemExit("--fused 1 computes its own unsmoothed loss inside the fused LeNet "
                         "step; --label-smoothing needs the layer-wise loop (--fused auto or 0)")
    if a.topk < 0:
        raise SystemExit("--topk must be >= 0")
    if a.compress != "none" and a.dp != "ddp":
        raise SystemExit(f"--compress {a.compress} runs inside DDP's buckets: it needs --dp ddp")
    if a.compress != "none" and a.allreduce == "xgmi":
        raise SystemExit(f"--compress {a.compress} all-gathers its payload: not with "
                         "--allreduce xgmi")
    if a.no_error_feedback and a.compress == "none":
        raise SystemExit("--no-error-feedback belongs to --compress q8 or topk")
    if a.compress != "topk" and a.compress_keep != 32:
        raise SystemExit("--compress-keep belongs to --compress topk")
    if not 1 <= a.compress_keep <= 256:
        raise SystemExit("--compress-keep must be in 1..256")
    if a.fused == "1" and a.augment != "none":
        raise SystemExit("--fused 1 reads the dataset rows inside the fused LeNet step; "
                         "--augment needs the layer-wise loop (--fused auto or 0)")
    mixing = a.mixup != 0 or a.cutmix != 0
    if a.fused == "1" and mixing:
        raise SystemExit("--fused 1 reads the dataset rows inside the fused LeNet step; "
                         "--mixup and --cutmix need the layer-wise loop (--fused auto or 0)")
    mix = None
    if mixing:
        try:
            mix = DeviceMix(a.mixup, a.cutmix, prob=a.mix_prob, switch_prob=a.mix_switch_prob,
                            seed=a.aug_seed)
        except ValueError as e:
            raise SystemExit(f"--mixup / --cutmix: {e}")
    aug = None
    if a.augment != "none":
        if a.aug_flip is None:
            a.aug_flip = 0.5 if a.model == "resnet18" else 0.0
        try:
            side = a.image_size if a.model == "resnet18" else 28
            if a.augment == "pad-crop":
                aug = DeviceAugment.pad_crop(a.aug_pad, flip=a.aug_flip, seed=a.aug_seed)
            else:
                aug = DeviceAugment.random_resized_crop(side, scale=tuple(a.aug_scale),
                                                        flip=a.aug_flip, seed=a.aug_seed)
        except ValueError as e:
            raise SystemExit(f"--augment: {e}")
    dev =env.init(a.n_devices, a.rank, a.master_addr, a.master_port, backend=a.backend,
                   device_type=a.device)
    rank, ws = env.get_rank(), env.get_world_size()
    checks = {}
    if a.compress != "none" and a.allreduce == "auto":
        a.allreduce = "rccl"  # compressed buckets go through the group's all-gather
    if ws > 1:
        # the device paths this run depends on, proven before training (selfcheck module)
        from dmlab.parallel import selfcheck

        checks.update(selfcheck.allreduce_selfcheck(dev))
        if checks["allreduce_selfcheck"] != "pass":
            raise SystemExit(f"all-reduce self-check failed: {checks}")
        want = a.allreduce == "xgmi" or (a.allreduce == "auto" and a.model == "lenet")
        if want and dev.type == "cuda" and a.dp == "ddp":
            checks.update(selfcheck.xgmi_selfcheck(dev))
        else:
            checks.update(xgmi_selfcheck="skipped", small_allreduce_used="rccl")
        a.allreduce = checks["small_allreduce_used"]
        if rank == 0:
            print("self-check: " + ", ".join(f"{k}={v}" for k, v in checks.items()))
    elif a.allreduce == "auto":
        a.allreduce = "rccl"
    torch.manual_seed(4321 + rank)
    if a.model == "lenet":
        model = Net(1, 10).to(dev)
        train_set = load_mnist(a.data, True, synthetic=True if a.synthetic else None,
                               n=a.train_samples)
        test_set = load_mnist(a.data, False, synthetic=True if a.synthetic else None)
    else:
        from dmlab.data import synthetic_classification

        # --image-size 224 --num-classes 1000: the headline config of bench.py / BASELINE.json
        # (ResNet-18 on ImageNet-shaped data); the default 64x64 / 10 classes keeps lab runs short
        model = ResNet18(num_classes=a.num_classes).to(dev)
        n = a.train_samples or 4096
        shape = (3, a.image_size, a.image_size)
        train_set = synthetic_classification(n, shape, a.num_classes, seed=0)
        test_set = synthetic_classification(512, shape, a.num_classes, seed=7)
    # seed=rank as the reference passes (task3/model.py:111); the partition
    # strategy needs a shared permutation so it uses seed 0 on every rank.
    seed = rank if a.sampler == "random" else 0
    sampler = MySampler(train_set, ws, rank, shuffle=True, seed=seed, mode=a.sampler)
    # bf16 activations: the device-resident data is stored in bf16 once; every native
    # kernel downstream then runs bf16 in / fp32 accumulate (GPU only: the CPU torch path
    # keeps fp32)
    act = torch.bfloat16 if (a.dtype == "bf16" and a.model == "lenet" and dev.type == "cuda") \
        else None
    if aug is None and mix is None:
        loader = DeviceLoader(train_set.to(dev, dtype=act), a.batch_size, sampler=sampler)
    else:  # the augmentation kernel reads channel-innermost rows
        # mixing runs inside the augmentation launch: without --augment, the identity transform
        tf = aug if aug is not None else DeviceAugment.pad_crop(0, flip=0.0, seed=a.aug_seed)
        loader = DeviceLoader(train_set.to(dev, dtype=act, memory_format=torch.channels_last),
                              a.batch_size, sampler=sampler, transform=tf, mix=mix)
    if a.optimizer == "lars":
        opt = LARS(model.parameters(), lr=a.lr, momentum=a.momentum,
                   weight_decay=a.weight_decay, trust_coefficient=a.trust_coef)
    else:
        opt = SGD(model.parameters(), lr=a.lr, momentum=a.momentum,
                  weight_decay=a.weight_decay)
    resumed = {}
    if a.resume:
        from dmlab.utils import checkpoint

        resumed = checkpoint.load(a.resume, model, opt)
    if a.sync_bn != "off":  # before DDP wraps the model; every rank (creates a process group)
        from dmlab.nn import convert_sync_batchnorm

        convert_sync_batchnorm(model, force=a.sync_bn == "force")
    if a.dp == "ddp":
        net = DDP(model, bucket_cap_mb=a.bucket_mb,  # broadcasts rank-0 params
                  small_allreduce="xgmi" if a.allreduce == "xgmi" and dev.type == "cuda" else None,
                  compress=None if a.compress == "none" else a.compress,
                  error_feedback=not a.no_error_feedback, compress_keep=a.compress_keep)
        net.fold_average_into(opt)
        if resumed.get("q8_residual") is not None and net.compressor is not None \
                and a.compress == "q8":
            # the residual is per-rank training state; it only fits the same world size
            if not net.load_residual_state(resumed["q8_residual"]) and rank == 0:
                print("checkpoint: q8 residual not restored (world size, buffer size or "
                      "--no-error-feedback differs); starting from a zero residual")
        elif resumed.get("topk_residual") is not None and net.compressor is not None \
                and a.compress == "topk":
            if not net.load_residual_state(resumed["topk_residual"]) and rank == 0:
                print("checkpoint: topk residual not restored (world size, buffer size or "
                      "--no-error-feedback differs); starting from a zero residual")
        elif net.compressor is not None and rank == 0:
            other = {"q8": "topk_residual", "topk": "q8_residual"}[a.compress]
            if resumed.get(other) is not None:
                print(f"checkpoint: its {other.split('_')[0]} residual belongs to the other "
                      f"codec and is not restored; --compress {a.compress} starts from a zero "
                      "residual")
        agg = None
    else:
        comm.init_parameters(model)
        net = model
        agg = comm.GradAggregator(model, "allreduce", timing="events")
    fused = a.fused == "1" or (a.fused == "auto" and a.model == "lenet" and dev.type == "cuda"
                               and a.dp == "ddp" and a.optimizer == "sgd"
                               and a.warmup_steps == 0 and a.label_smoothing == 0
                               and aug is None and mix is None)
    if fused:
        if a.model != "lenet" or dev.type != "cuda" or a.dp != "ddp":
            raise SystemExit("--fused 1 needs --model lenet on a GPU with --dp ddp")
        from dmlab.tasks.common import train_fused

        capturable = ws == 1 or dist_backend() == "nccl" or a.allreduce == "xgmi"
        graph = a.graph == "1" or (a.graph == "auto" and capturable)
        # whole batches replay the captured fixed-shape step; the shard's partial last batch
        # (if any) runs as one eager fused step, as the reference DataLoader keeps it
        stats = train_fused(model, loader, opt, a.epochs, ddp=net, rank=rank, graph=graph,
                            graph_steps=a.graph_steps, max_steps=a.max_steps)
        stats.update(fused=True, hip_graph=graph, hip_graph_steps=stats.pop("graph_steps"))
    else:
        after_step = None
        if a.warmup_steps > 0:  # the schedule sets the rate of step t+1 after step t
            opt.lr = a.lr  # a resumed run restarts the schedule from its base rate
            total = a.epochs * len(loader)
            if a.max_steps is not None:
                total = min(total, a.max_steps)
            sched = WarmupPolyLR(opt, min(a.warmup_steps, total), total)
            after_step = lambda _step: sched.step()  # noqa: E731
        stats = train(net, loader, CrossEntropyLoss(a.label_smoothing), opt, a.epochs, rank=rank,
                      aggregate=agg, batch_size=a.batch_size, max_steps=a.max_steps,
                      after_step=after_step)
    if a.optimizer != "sgd":
        stats["optimizer"] = a.optimizer
    if a.label_smoothing > 0:
        stats["label_smoothing"] = a.label_smoothing
    if aug is not None:
        stats.update(augment=a.augment, aug_seed=a.aug_seed, aug_flip=a.aug_flip)
    if mix is not None:
        stats.update(mixup=a.mixup, cutmix=a.cutmix, mix_prob=a.mix_prob)
    print("Training time: {}".format(stats["train_time"]))
    if rank == 0:
        print("Throughput: {:.1f} samples/s (whole job, {} rank{})".format(
            stats["samples"] * ws / stats["train_time"], ws, "s" if ws > 1 else ""))
    if hasattr(net, "sync_buffers"):
        net.sync_buffers()  # every rank: rank 0's BN statistics for the save and the test
    if a.save:
        from dmlab.utils import checkpoint

        extra = {}
        if a.compress != "none":  # every rank's residual (a collective), kept by rank 0
            extra[f"{a.compress}_residual"] = net.residual_state()
        checkpoint.save(a.save, model, opt, epochs=a.epochs, **extra)
    sharded = a.eval == "sharded"
    ev_kw = {}
    if a.augment == "rrc":  # evaluate on the deterministic centre crop of the same size
        ev_kw = dict(transform=aug.eval())
        test_set = test_set.to(dev, dtype=act, memory_format=torch.channels_last)
    if not a.no_test and (sharded or (a.topk > 0 and rank == 0)):
        # top-k and the test loss; sharded: every rank takes its unpadded shard of the test set
        shard = ShardSampler(test_set, ws, rank) if sharded else None
        ev = evaluate(model, DeviceLoader(test_set.to(dev, dtype=act), 32, sampler=shard, **ev_kw),
                      k=a.topk or 5, sharded=sharded)
        stats.update(ev, accuracy=ev["top1"])
    elif not a.no_test and a.topk == 0 and rank == 0:
        stats["accuracy"] = test(model, DeviceLoader(test_set.to(dev, dtype=act), 32, **ev_kw))
    stats.update(checks)
    if a.sync_bn != "off":
        stats.update(sync_bn=a.sync_bn, sync_bn_collectives=model.sync_bn_collectives)
    stats.update(rank=rank, world_size=ws, sampler=a.sampler, dp=a.dp, compress=a.compress,
                 comm_bytes_per_step=(net.comm_bytes_per_step if a.dp == "ddp"
                                      else agg.bytes_per_call),
                 samples_per_s=stats["samples"] * ws / stats["train_time"])
    if a.json and rank == 0:
        with open(a.json, "w") as f:
            json.dump(stats, f)
    env.barrier()
    env.destroy()
    return stats


if __name__ == "__main__":
    main()
