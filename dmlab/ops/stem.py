"""First-layer ("stem") path of :class:`dmlab.nn.layers.ConvBN` / ``ConvBNPool``: the input is
a raw image batch (NCHW / channels_last tensor or a ``dmlab.data.Gathered`` loader batch), not
an internal NHWC bf16 tensor, and there is no data gradient.  :func:`stem_fwd` picks one path,
records it in ``ctx["stem"]``, and :func:`stem_bwd` follows it:

``"fused"`` (:func:`stem_fused_ok`): the K-dense 7x7 conv + BN statistics + max-pool kernel
    (csrc/stem_fused.hip); the conv output is never written.  ctx: img, gidx, nsc, nbi, wk
    (the kernel's operands, re-read by the backward), yarg (pooled BN input at each window's
    argmax), idx (window codes), mean, invstd, scale, shift, M (conv output pixels), total.
``"s2d"`` (:func:`use_s2d`): 7x7/s2 as a 4x4/s1 conv over the space-to-depth input
    (csrc/conv_stem.hip).  ctx: x (the packed input), y, mean, invstd, scale, shift, total
    and, under a max-pool, idx (argmax codes) and yarg (y at the argmax; None for eval-mode BN).
``"plain"``: anything else (odd image sizes): ``as_nhwc`` + the regular cfg.  ctx as "s2d".

Readers besides :func:`stem_bwd`: ``convbn._dgrad_red`` (yarg or y, mean, invstd, scale,
shift), which leaves ``pre_sums`` here from the first block's last data gradient.  The
extension is taken through ``convbn.lib()`` (one place to observe every launch).
"""
from __future__ import annotations

import os

import torch

from . import convbn as CB
from .convbn import (_bn_finalize, _cpad, as_nhwc, bn_bwd, conv_stats, empty_nhwc, launch_wgrad,
                     packed_weights, pick_cfg)

_STEM_CFG = 60
_STEM_FUSED_DEFAULT = "1"  # GPU-validated (tests/test_stem_fused.py); bench A/B +1.9 %


def use_s2d(layer, x):
    """7x7/s2 stem on a small-channel input with even H, W -> space-to-depth 4x4/s1."""
    return (layer.k == 7 and layer.stride == 2 and layer.padding == 3 and layer.cin <= 4
            and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0)


def packed_weights_s2d(layer):
    prog = layer._prog
    cache = getattr(layer, "_wcache_s2d", None)
    if cache is None or cache[0] != prog._wver:
        w = layer.weight.detach()
        wf = torch.empty((layer.cout, 4, 4, _cpad(4 * layer.cin)), device=w.device,
                         dtype=torch.bfloat16)
        CB.lib().pack_weights_s2d(w, wf)
        cache = (prog._wver, wf)
        object.__setattr__(layer, "_wcache_s2d", cache)
    return cache[1]


def packed_weights_stem(layer):
    """[64][176] bf16 K-dense stem weights (k = ky*24 + kx*3 + c), cached per weight version."""
    prog = layer._prog
    cache = getattr(layer, "_wcache_k176", None)
    if cache is None or cache[0] != prog._wver:
        wk = cache[1] if cache is not None else torch.empty(
            (64, 176), device=layer.weight.device, dtype=torch.bfloat16)
        CB.lib().stem_pack_weights(layer.weight.detach(), wk)
        cache = (prog._wver, wk)
        object.__setattr__(layer, "_wcache_k176", cache)
    return cache[1]


def _stem_image(x):
    """(images, idx) of a stem input: a loader batch by index (dmlab.data.Gathered) or an
    image tensor ((N,3,H,W) channels_last or (N,H,W,3)); None if it is neither."""
    if not isinstance(x, torch.Tensor):
        return x.images, x.idx
    if x.dim() == 4 and x.shape[1] == 3 and not getattr(x, "_dm_nhwc", False):
        if not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        return x, None
    return None


def stem_fused_ok(layer, x):
    """The K-dense fused stem (csrc/stem_fused.hip) serves this layer and input:
    7x7/s2/p3 conv 3 -> 64 + BN + ReLU + 3x3/s2/p1 max-pool, on a raw fp32 / bf16 / u8 image
    batch whose size the kernel supports, BN in training mode or eval (not eval-BN with
    gradients).  DMLAB_STEM_FUSED=0 selects the space-to-depth path (A/B)."""
    if os.environ.get("DMLAB_STEM_FUSED", _STEM_FUSED_DEFAULT) == "0":
        return False
    if not (getattr(layer, "pool_k", 0) == 3 and layer.pool_s == 2 and layer.pool_p == 1
            and layer.k == 7 and layer.stride == 2 and layer.padding == 3 and layer.cin == 3
            and layer.cout == 64 and layer.relu):
        return False
    im = _stem_image(x)
    if im is None:
        return False
    img = im[0]
    if img.dtype not in (torch.float32, torch.bfloat16, torch.uint8) or not img.is_cuda:
        return False
    H, W = (img.shape[2], img.shape[3]) if img.shape[1] == 3 else (img.shape[1], img.shape[2])
    return bool(CB.lib().stem_fused_supported(H, W))


def stem_fwd(layer, x, ctx, train):
    """First-layer forward on the "fused", else the "s2d", else the "plain" path."""
    L = CB.lib()
    if (layer.training or not train) and stem_fused_ok(layer, x):  # not eval-BN with gradients
        return _stem_fused_fwd(layer, x, ctx, train)
    gidx = None
    if not isinstance(x, torch.Tensor):  # dmlab.data.Gathered: a loader batch by row index
        if use_s2d(layer, x.images) and x.images.dtype in (torch.float32, torch.bfloat16):
            x, gidx = x.images, x.idx  # the s2d packing below gathers the rows itself
        else:
            x = x.materialize()
    assert not getattr(x, "_dm_nhwc", False), "a first layer takes a raw image batch"
    s2d = use_s2d(layer, x)
    if s2d:
        # stem as a 4x4/s1 conv over the space-to-depth input (pad 2 top/left, 1 bottom/right)
        k, s, p = 4, 1, 2
        OH, OW = x.shape[2] // 2, x.shape[3] // 2
        xs = empty_nhwc(gidx.numel() if gidx is not None else x.shape[0], OH, OW,
                        _cpad(4 * x.shape[1]), x)
        L.pack_input_s2d(x if x.dtype in (torch.float32, torch.bfloat16) else x.float(), xs, gidx)
        x = xs
        wf = packed_weights_s2d(layer)
        # the resident-weight stem kernel (60, csrc/conv_stem.hip) stages the weights and the
        # input halo once per 256 pixels (the v3 128x64 tile, 16, re-stages one 4-tap K-slice
        # per step: 382 TFLOP/s at batch 512, profiles/conv_stem_s2d_r1s4.jsonl)
        cfg = _STEM_CFG
    else:
        x = as_nhwc(x, _cpad(layer.cin))
        k, s, p = layer.k, layer.stride, layer.padding
        H, W = x.shape[1:3]
        OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        wf, _ = packed_weights(layer, need_wd=False)
        cfg = pick_cfg(x.shape[0] * OH * OW, layer.cout, k, s, x.shape[3],
                       W=OW if (OH, OW) == (H, W) else 0)
    y, scale, shift, mean, invstd, total = conv_stats(L, layer, x, wf, k, s, p, cfg, {}, OH, OW)
    if train:
        ctx.update(stem="s2d" if s2d else "plain", x=x, y=y, mean=mean, invstd=invstd,
                   scale=scale, shift=shift, total=total)
    N, cout = x.shape[0], layer.cout
    if not getattr(layer, "pool_k", 0):  # a plain ConvBN fed a raw image
        out = empty_nhwc(N, OH, OW, cout, x)
        L.bn_apply(y, None, scale, shift, out, layer.relu, mask=None)
        return out
    # fused BN + ReLU + max-pool: the BN output is never materialised
    pk, ps, pp = layer.pool_k, layer.pool_s, layer.pool_p
    PH, PW = (OH + 2 * pp - pk) // ps + 1, (OW + 2 * pp - pk) // ps + 1
    out = empty_nhwc(N, PH, PW, cout, x)
    idx = torch.empty((N, PH, PW, cout), device=x.device, dtype=torch.uint8)
    # training: also keep y at each window's argmax, so the backward reduces the BN
    # sums over the pooled grid (see bn_relu_maxpool_kernel)
    yarg = empty_nhwc(N, PH, PW, cout, x) if (train and layer.training) else None
    L.bn_relu_maxpool(y, scale, shift, out, idx, pk, ps, pp, yarg=yarg)
    if train:
        ctx.update(idx=idx, yarg=yarg)
    return out


def _pooled_sums(L, dout, ctx):
    """Σdz, Σdz·x̂ over the pooled grid (pooled grad masked at the argmax, x̂ from y at the
    argmax) -- reads 2 pooled-size tensors instead of y + grad + codes; as bn_backward's
    pre_sums.  Skipped when the first block's last data gradient already reduced them."""
    pre_sums = ctx.pop("pre_sums", None) or {}
    if ctx.get("yarg") is None or pre_sums:
        return pre_sums
    cout = dout.shape[3]
    part = torch.empty(L.bn_bwd_rows(ctx["yarg"].numel() // cout, cout) * 2 * cout,
                       device=dout.device, dtype=torch.float32)
    rows = L.bn_bwd_reduce_masked(dout, ctx["yarg"], ctx["mean"], ctx["invstd"], ctx["scale"],
                                  ctx["shift"], part)
    return dict(pre_slab=part, pre_rows=rows)


def stem_bwd(layer, dout, ctx):
    """Weight and BN-parameter gradients of a first layer; returns None (no data gradient)."""
    if ctx["stem"] == "fused":
        return _stem_fused_bwd(layer, dout, ctx)
    L = CB.lib()
    s2d = ctx["stem"] == "s2d"
    x, y = ctx["x"], ctx["y"]
    N, OH, OW, cout = y.shape
    k, s, p = (4, 1, 2) if s2d else (layer.k, layer.stride, layer.padding)
    acc = 1.0 if layer.accumulate else 0.0
    dout = dout.contiguous()
    pool = getattr(layer, "pool_k", 0)
    work = torch.empty(L.bn_bwd_work(N * OH * OW, cout), device=y.device, dtype=torch.float32)
    pre_sums = _pooled_sums(L, dout, ctx)
    # synchronized BatchNorm (ctx["total"]: the global count of the forward's merge) takes the
    # unfused mode-3 backward below, which has the two stages
    if (pool and s2d and pre_sums and ctx["total"] is None
            and L.stem_bwd_fused_supported(y, x)):
        # BN-backward apply fused into the s2d weight gradient -- the full-resolution dy is
        # never written (csrc/conv_stem.hip stem_wgrad_ws_kernel)
        slab = torch.empty(L.stem_bwd_slab_floats(N, OH), device=y.device, dtype=torch.float32)
        L.stem_bwd_fused(y, ctx["mean"], ctx["invstd"], layer.bn_weight.detach(),
                         layer.grad_slot("bn_weight"), layer.grad_slot("bn_bias"), acc,
                         ctx["scale"], ctx["shift"], dout, ctx["idx"], pre_sums["pre_slab"],
                         pre_sums["pre_rows"], x, layer.cin, layer.grad_slot("weight"), acc,
                         work, slab)
        return None
    # 3: dz gathered from the max-pool gradient, ReLU mask from y; 2 / 0: ReLU mask from y / none
    mode = 3 if pool else 2 if layer.relu else 0
    dy, _ = bn_bwd(L, layer, ctx, mode, dout, None, pre_sums, work)
    launch_wgrad(L, layer, x, dy, None, k, s, p, s2d=s2d)


def _stem_fused_fwd(layer, x, ctx, train):
    """Fused stem forward: pooled BN-input extremum + window codes + BN statistics in one
    kernel, then BN + ReLU on the pooled tensor.  The conv output is never written."""
    from dmlab.data import input_affine

    L = CB.lib()
    img, idx = _stem_image(x)
    B = idx.numel() if idx is not None else img.shape[0]
    H, W = (img.shape[2], img.shape[3]) if img.shape[1] == 3 else (img.shape[1], img.shape[2])
    PH, PW = H // 4, W // 4
    dev = img.device
    nsc, nbi = input_affine(img.dtype)
    wk = packed_weights_stem(layer)
    pext = empty_nhwc(B, PH, PW, 64, img)
    code = torch.empty((B, PH, PW, 32), device=dev, dtype=torch.uint8)
    grid = L.stem_fused_grid(B)
    stats = (torch.empty(grid * 128, device=dev, dtype=torch.float32) if layer.training
             else None)
    L.stem_fwd_fused(img, idx, nsc, nbi, wk, layer.bn_weight.detach(), pext, code, stats, grid)
    M = B * (H // 2) * (W // 2)
    scale, shift, mean, invstd, total = _bn_finalize(L, layer, stats, grid, M)
    out = empty_nhwc(B, PH, PW, 64, img)
    code4 = torch.empty((B, PH, PW, 32), device=dev, dtype=torch.uint8) if train else None
    L.stem_pool_apply(pext, code if train else None, scale, shift, out, code4)
    if train:
        ctx.update(stem="fused", img=img, gidx=idx, nsc=nsc, nbi=nbi, wk=wk, yarg=pext,
                   idx=code4, mean=mean, invstd=invstd, scale=scale, shift=shift, M=M,
                   total=total)
    return out


def _stem_fused_bwd(layer, dout, ctx):
    """Fused stem backward: BN-backward coefficients from the pooled-domain sums, then the
    weight gradient of dy = a*dz + b*y + cc with y recomputed from the raw input (never
    stored), reduced in fixed order into the OIHW gradient."""
    L = CB.lib()
    dout = dout.contiguous()
    acc = 1.0 if layer.accumulate else 0.0
    pre_sums = _pooled_sums(L, dout, ctx)
    B = dout.shape[0]
    grid = L.stem_fused_grid(B)
    f32 = dict(device=dout.device, dtype=torch.float32)
    work = torch.empty(L.bn_bwd_work(ctx["M"], 64), **f32)
    dslab = torch.empty(L.stem_bwd_slab_len(grid), **f32)
    sync_kw = {}
    if ctx["total"] is not None:
        # synchronized BatchNorm: dgamma / dbeta from this rank's sums, the coefficients from
        # the sums of every rank and the global count
        sums = torch.empty(128, device=dout.device, dtype=torch.float64)
        L.bn_bwd_sums(pre_sums["pre_slab"], pre_sums["pre_rows"], 64, layer.grad_slot("bn_weight"),
                      layer.grad_slot("bn_bias"), acc, work, sums)
        layer._sync_bn.reduce_sums(sums)
        sync_kw = dict(sums=sums, total=ctx["total"])
    L.stem_bwd_fused2(ctx["img"], ctx["gidx"], ctx["nsc"], ctx["nbi"], ctx["wk"], dout,
                      ctx["idx"], ctx["mean"], ctx["invstd"], layer.bn_weight.detach(),
                      layer.grad_slot("bn_weight"), layer.grad_slot("bn_bias"), acc,
                      pre_sums["pre_slab"], pre_sums["pre_rows"], layer.grad_slot("weight"), acc,
                      work, dslab, grid, **sync_kw)
