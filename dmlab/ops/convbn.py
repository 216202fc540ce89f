"""Native path of :class:`dmlab.nn.layers.ConvBN` (NHWC bf16, ResNet family).

Forward : implicit-GEMM MFMA conv whose epilogue also emits per-tile Σy/Σy² →
          BN statistics finalize (+ running-stat update) → fused BN-apply
          [+ residual] [+ ReLU].
Backward: BN backward (reduce + apply, also emitting the residual-branch grad) →
          weight-gradient implicit GEMM (split-M fp32 slabs, fixed-order reduce into
          the OIHW fp32 grad slot) → data-gradient implicit GEMM (parity-class
          decomposition for stride 2), optionally fused with the skip-connection
          add.

Activations are plain contiguous ``[N, H, W, C]`` bf16 tensors.  Packed bf16
weights ([Cout][KH][KW][Cpad] for forward, [Cin][KH][KW][Cout] for dgrad) are
cached per layer and refreshed when the fp32 master changes.

:func:`convbn_fwd` / :func:`convbn_bwd` serve interior layers (input already internal NHWC);
a first layer (raw image input) goes through :mod:`dmlab.ops.stem`, which shares
:func:`conv_stats`, :func:`bn_bwd` and :func:`launch_wgrad` with them.

ctx of an interior ConvBN (written by convbn_fwd in training; readers in brackets):
  x, y        conv input (un-normalised when ``pre`` is set) and output [bn_bwd, launch_wgrad,
              _dgrad; y also _dgrad_red of the producing layer's data gradient]
  mean, invstd, scale, shift   batch statistics (None in eval mode) and the BN affine
              [bn_bwd, _dgrad_red; BasicBlock reads c1's scale / shift as c2's ``pre``]
  pre         (scale, shift) of the previous BN when x is its raw conv output [launch_wgrad]
  total       global element count under synchronized BatchNorm, else None [bn_bwd]
  has_res     the forward added a residual [convbn_bwd: BN mode, the (dx, dres) return]
  out, mask   with a residual: the output and, with ReLU, its 1-bit (out > 0) mask
              [convbn_bwd modes 1 / 4, _dgrad_red, the fused skip add of the next dgrad]
  pre_sums    left by _dgrad_red of the layer above: this BN's backward sums [convbn_bwd pops]
  _bn_out     (dy, dres) between phase 1 and phase 2 of convbn_bwd
"""
from __future__ import annotations

import contextlib
import math

import torch

from ._native import lib


def _cpad(c):
    return max(8, (c + 7) // 8 * 8)


# What every kernel config id is and can do is one table, csrc/conv_cfg.h (read here through
# _cfg); this module only decides which id a layer gets.  Measured on MI355X
# (tools/bench_conv.py -> profiles/conv_kernels_r1.jsonl, conv_halo_tiles_b512_r1s4.jsonl):
#   * strided taps, stride-2 dgrad parity classes below 256 channels, 1x1/s2 below 256
#     channels: v3 tiles 15 / 13 / 11 by the block-count rule below (256-row tiles lose
#     there: one workgroup per CU exposes the staging latency).
TILE_CFG = (15, 13, 11)
# The round-3 A/B switches (DMLAB_NO_PIPE / NO_RES64 / NO_FUSED_SKIP / NO_DGRAD_RED /
# NO_WRES64 / WRES64_S / TAIL_WGRAD_FULL / WGRAD_BLOCKS / RES64_ADD_RED / STEM_CFG) are
# settled and removed; their measurements stay in docs/KERNELS.md and profiles/.
# So are round 6's (MERGE_SHORTCUT / MERGE_PIPE, RES64_RED_ADD, DOWN_FWD_STREAM, AUX_STREAM,
# FIN_DIRECT, STEM_GRID / SPLIT / ABLATE / TRACE); docs/ARCHITECTURE.md lists the variables
# that remain.


_CFG_INFO = {}


def _cfg(cfg, L=None, wgrad=False):
    """The csrc/conv_cfg.h row of a forward-style (``wgrad``: weight-gradient) config id as a
    dict, None for an id the table does not have; looked up once per id."""
    key = (wgrad, cfg)
    if key not in _CFG_INFO:
        L = L or lib()
        _CFG_INFO[key] = L.wgrad_cfg_info(cfg) if wgrad else L.conv_cfg_info(cfg)
    return _CFG_INFO[key]


def _can(cfg, what, L=None, wgrad=False):
    """Capability ``what`` (a boolean field of the config's table row); False for an unknown id."""
    info = _cfg(cfg, L, wgrad)
    return bool(info and info[what])


def dgrad_cfg(M, cin, k, stride, cout, W=0):
    """Kernel config of a data-gradient GEMM (dX has M pixels of ``cin`` channels)."""
    return pick_cfg(M, cin, k, stride, cout, W=W)


def pick_cfg(M, ncols, k=0, stride=0, cin=0, W=0):
    """Kernel config for a forward-style conv GEMM with M output pixels and ncols
    output channels.  ``k``/``stride``/``cin`` (kernel size, tap stride, input
    channels) enable the unit-stride halo kernel when they describe a k x k conv with
    unit tap stride over 64-channel-aligned input; ``W`` (image width, 0 = unknown)
    enables the resident-weight 64-channel kernel."""
    # 80: persistent resident-weight 64 -> 64 channel 3x3 conv (csrc/conv_res64.hip; its
    # 128-pixel tile's halo, 128 + 2W + 2 rows, must fit the 256-row LDS image; the input
    # below 1 GiB: its DMA pad pieces are addressed past 2^30)
    if (k == 3 and stride == 1 and cin == 64 and ncols == 64 and 0 < W <= 63
            and M * 128 < 2**30 - 2**14):
        return 80
    # 90: the pipelined LDS-DMA 256 x 256 tile (csrc/conv_pipe.hip), for >= 256 output
    # channels and 64-channel-aligned input, any tap geometry.  tools/bench_conv.py at batch
    # 1024 (profiles/conv_pipe_vs_halo_b1024_r3a.jsonl, TFLOP/s fwd/dgrad, best previous tile):
    #   layer3 3x3 975/1004 (41: 897/971), layer4 3x3 1151/1160 (41: 933/957),
    #   layer4 3x3/s2 1030/901 (15: 750/724), layer3 3x3/s2 fwd 778 (42: 690),
    #   layer4 1x1/s2 442/367 (15: 351/299); the 64/128-channel layers keep the halo tiles
    if ncols % 256 == 0 and cin % 64 == 0 and cin > 0:
        return 90
    if k == 3 and stride == 1 and cin % 64 == 0 and ncols % 64 == 0:
        # 64 output channels: the 256-pixel halo tile (2 x 2 waves of 128 x 32) amortises
        # the single-chunk halo prologue over twice the rows
        # 42: the 128-pixel BN-128 tile with two weight tiles of register prefetch;
        # 41: 256-pixel tile of 4 x 1 waves, each 64 x 64 (one LDS fragment read per MFMA
        # pair instead of 1.5; BN 64 doubles the column blocks).  tools/bench_conv.py
        # (profiles/conv_halo_tiles_b512_r1s4.jsonl, batch 512 / 256, TFLOP/s fwd/dgrad):
        #   layer2 (128 ch): 42 807/834, 20 761/818, 41 781/817   (b256: 42 647/681)
        #   layer3 (256 ch): 41 852/867, 42 834/840                (b256: 41 722/762)
        #   layer4 (512 ch): 41 856/867, 43 812/820                (b256: 41 822/848)
        #   layer1 (64 ch) : 39 612/683, 41 580/642
        if ncols >= 256:
            return 41
        return 42 if ncols >= 128 else 39
    if ncols % 128 == 0 and math.ceil(M / 128) * (ncols // 128) >= 192:
        t = 0  # 64x64 per wave beats the narrower tile even at ~1 block per CU
    elif math.ceil(M / 128) * math.ceil(ncols / 64) >= 480:
        t = 1
    else:
        t = 2
    return TILE_CFG[t]


# weight-gradient blocks per launch (m-split target): ~2 per CU.  These run on the side
# stream for the whole kernel and hold LDS the critical-path kernels need.  Measured
# (profiles/wgrad_blocks_r2c.jsonl, one call): 512 -> 44.2/44.4k img/s, 384 44.2k,
# 256 43.6/43.7k, 768 43.4k, 1024 43.4/43.5k; at 1024 images per GPU 512 -> 46.6k,
# 768 45.5-45.8k, 1024 46.0-46.2k (profiles/wgrad_blocks_b1024_r2c.jsonl); re-measured under
# the high-priority step stream in round 4: 160-1024 blocks and CU-masked weight-gradient
# streams all lose to 512 (profiles/wgrad_blocks_sidemask_ab_r4m.txt); round 6, a larger
# budget for layers 3-4 only (>= 256 output channels): 768 -1.5 %, 1024 -0.4 %
# (profiles/merged_shortcut_ab_r6.txt, "wide768" / "wide1024")
_WGRAD_BLOCKS = 512
_CUS = {}


def _cu_count():
    if not torch.cuda.is_available():
        return 256
    d = torch.cuda.current_device()
    if d not in _CUS:
        _CUS[d] = torch.cuda.get_device_properties(d).multi_processor_count
    return _CUS[d]


def _wgrad_plan(M, cout, K, k=0, stride=0, cin=0, force=None, W=0, rows=0, tail=False,
                even=0):
    """(cfg, S) for the weight-gradient GEMM dW[cout, K] = Σ_m dY[m, cout] X_col[m, K].

    cfg 8: row-streaming 64 -> 64 channel 3x3 kernel (csrc/wgrad_res64.hip; ``W`` = image
    width <= 60, ``rows`` = N*H image rows, S = 5/8 of the CUs); cfg 4/5: halo-staged 3x3
    unit-stride kernel (csrc/wgrad_halo.hip) with 9 / 3 taps per block; cfg 7: the stride-2
    3x3 kernel over the input's parity planes (same file); cfg 2/3/6: v2 igemm tiles
    128x128 / 64x128 / 64x256.
    S splits the m reduction over blocks into fp32 slabs summed by a fixed-order reduce:
    ~2 blocks per CU, each split >= 8 row steps, slab bytes S*cout*K*4."""
    halo = k == 3 and stride == 1 and cin % 64 == 0 and cout % 8 == 0
    res64 = k == 3 and stride == 1 and cin == 64 and cout == 64 and 0 < W <= 60 and rows > 0
    if force == 8 or (force is None and res64):
        # 5/8 of the CUs: the kernel runs on the side stream next to the dgrad + BN-backward
        # chain, and leaving that chain CUs of its own is 0.8% faster per step than one
        # workgroup on every CU (128-192 of 256 tie; profiles/wgrad_res64_slabs_ab_r3s3.txt)
        # ``tail``: the last conv before the stem, whose weight gradient runs next to the stem's
        # fused BN-backward + weight-gradient kernel at the end of the step, not next to a
        # dgrad chain: there it takes every CU (5/8 there, or the main stream instead of the
        # side stream, measure the same or slower: profiles/tail_wgrad_placement_ab_r4i.txt)
        S = _cu_count() if tail else max(1, _cu_count() * 5 // 8)
        return 8, max(1, min(rows, S))
    # ``even``: output width of a stride-2 conv whose output is exactly half the input in both
    # dims (0 otherwise); the 3x3 plane staging holds rows up to a width of 31
    # (1x1 projections on a one-tap variant of it measured slower than the igemm tile:
    # profiles/wgrad_s2_1x1_rejected_r4ao.txt)
    s2 = stride == 2 and k == 3 and cin % 64 == 0 and cout % 8 == 0 and 0 < even <= 31
    if force is not None:
        cfg = force
    elif s2:
        # stride-2 3x3 (first conv of layers 2-4): the parity-plane kernel, 9 taps per block
        cfg = 7
    elif halo:
        # 9 taps per block share every dY fragment, but a layer with few (cout, cin)
        # tiles then needs many m-splits (slab traffic ~ S * cout * K); 3 taps per block
        # triples the tiles
        cfg = 4 if math.ceil(cout / 64) * (cin // 64) >= 4 else 5
    else:
        cfg = 2 if cout % 128 == 0 else 3
    if cfg in (4, 5, 7):
        tiles = max(1, math.ceil(cout / 64) * (cin // 64) * (3 if cfg == 5 else 1))
        max_split = max(1, M // 512)
    else:
        bm = 128 if cfg == 2 else 64
        tiles = math.ceil(cout / bm) * math.ceil(K / (256 if cfg == 6 else 128))
        # >= 8 row steps of 64 per split: the small-K layers (1x1/s2 downsample: K = Cin)
        # have one or two output tiles, so the m-split is their only parallelism
        max_split = max(1, M // 512)
    # (2x / 4x more splits for cfg 7 measured -0.4 / -1.0 %: profiles/wgrad_s2_splits_ab_r4ap.txt)
    S = max(1, min(max_split, math.ceil(_WGRAD_BLOCKS / tiles)))
    return cfg, S


def as_nhwc(x, cpad=None):
    """Accept [N,H,W,C] bf16 (internal layout) or a user NCHW / channels_last tensor."""
    if x.dim() == 4 and x.dtype == torch.bfloat16 and x.is_contiguous() and getattr(x, "_dm_nhwc", False):
        return x
    N, C, H, W = x.shape
    cp = cpad or _cpad(C)
    y = torch.empty((N, H, W, cp), device=x.device, dtype=torch.bfloat16)
    lib().pack_input(x if x.dtype in (torch.float32, torch.bfloat16) else x.float(), y)
    return _mark(y)


def _mark(t):
    t._dm_nhwc = True
    return t


def empty_nhwc(N, H, W, C, like):
    return _mark(torch.empty((N, H, W, C), device=like.device, dtype=torch.bfloat16))


def _bn_finalize(L, layer, stats, T, M):
    """Statistics slab [T][2C] -> (scale, shift, mean, invstd, total) + the running statistics;
    ``stats`` None (eval-mode BN): scale / shift from the running statistics, the rest None.
    Per-rank BatchNorm: one finalize over this rank's M elements, total None.  Synchronized
    (dmlab.nn.syncbn): local float64 row -> all-gather -> merge in rank order; total is the
    global element count as a float64 device scalar (it never visits the host)."""
    g, b = layer.bn_weight.detach(), layer.bn_bias.detach()
    C = layer.cout
    f32 = dict(device=g.device, dtype=torch.float32)
    scale, shift = torch.empty(C, **f32), torch.empty(C, **f32)
    if stats is None:
        L.bn_eval_coeffs(g, b, layer.running_mean, layer.running_var, layer.eps, scale, shift)
        return scale, shift, None, None, None
    mean, invstd, work = torch.empty(C, **f32), torch.empty(C, **f32), torch.empty(512 * C, **f32)
    sync = layer._sync_bn
    if sync is None:
        L.bn_stats_finalize(stats, T, float(M), g, b, layer.running_mean, layer.running_var,
                            layer.momentum, layer.eps, scale, shift, mean, invstd, work,
                            layer.num_batches_tracked)
        return scale, shift, mean, invstd, None
    row = torch.empty(2 * C + 1, device=stats.device, dtype=torch.float64)
    L.bn_sync_local(stats, T, float(M), C, row, work)
    rows = sync.gather_rows(row)
    total = torch.empty(1, device=stats.device, dtype=torch.float64)
    L.bn_sync_finalize(rows, g, b, layer.running_mean, layer.running_var, layer.momentum,
                       layer.eps, scale, shift, mean, invstd, layer.num_batches_tracked, total)
    return scale, shift, mean, invstd, total


def packed_weights(layer, need_wd=True):
    prog = layer._prog
    ver = prog._wver
    cache = getattr(layer, "_wcache", None)
    cp = _cpad(layer.cin)
    if cache is None or cache[0] != ver or (need_wd and cache[2] is None):
        w = layer.weight.detach()
        k = layer.k
        wf = torch.empty((layer.cout, k, k, cp), device=w.device, dtype=torch.bfloat16)
        wd = (torch.empty((layer.cin, k, k, layer.cout), device=w.device, dtype=torch.bfloat16)
              if need_wd else None)
        lib().pack_weights(w, wf, wd, cp)
        cache = (ver, wf, wd)
        object.__setattr__(layer, "_wcache", cache)
    return cache[1], cache[2]


def pack_all(prog, layers):
    """Refresh the packed bf16 weights (wf [Cout][KH][KW][Cpad], wd [Cin][KH][KW][Cout]) of
    every conv in ``layers`` with ONE kernel launch; :func:`packed_weights` then hits the
    cache.  Buffers persist across steps (stable pointers, graph-capturable); the device
    descriptor table is rebuilt only when a weight's storage moves."""
    ver = prog._wver
    layers = [m for m in layers if m.k * m.k <= 64][:32]
    if not layers:
        return
    key = tuple(m.weight.data_ptr() for m in layers)
    st = getattr(prog, "_pack_state", None)
    if st is None or st["key"] != key:
        dev = layers[0].weight.device
        bufs, rows, pre, tpre = [], [], [0], [0]
        for m in layers:
            cp = _cpad(m.cin)
            wf = torch.empty((m.cout, m.k, m.k, cp), device=dev, dtype=torch.bfloat16)
            wd = torch.empty((m.cin, m.k, m.k, m.cout), device=dev, dtype=torch.bfloat16)
            bufs.append((wf, wd))
            rows.append([m.weight.data_ptr(), wf.data_ptr(), wd.data_ptr(), m.cout, m.cin, cp,
                         m.k, m.k])
            pre.append(pre[-1] + m.cout * m.k * m.k * cp)
            tpre.append(tpre[-1] + -(-m.cout // 32) * -(-max(cp, m.cin) // 32))
        st = dict(key=key, bufs=bufs, total=pre[-1], ntiles=tpre[-1],
                  tprefix=torch.tensor(tpre, dtype=torch.int32).to(dev),
                  desc=torch.tensor(rows, dtype=torch.int64).reshape(-1).to(dev),
                  prefix=torch.tensor(pre, dtype=torch.int64).to(dev))
        object.__setattr__(prog, "_pack_state", st)
    for m in layers:
        assert m.weight.is_contiguous()
    lib().pack_weights_tiled(st["desc"], st["tprefix"], st["ntiles"])
    for m, (wf, wd) in zip(layers, st["bufs"]):
        object.__setattr__(m, "_wcache", (ver, wf, wd))


def _materialise(x, pre):
    """relu(x*scale + shift) as a tensor (fallback when a consumer cannot fuse it)."""
    out = empty_nhwc(*x.shape, x)
    lib().bn_apply(x, None, pre[0], pre[1], out, True)
    return out


def conv_stats(L, layer, x, wf, k, s, p, cfg, pre_kw, OH, OW):
    """Shared forward step (interior layers and dmlab.ops.stem): the conv, whose epilogue emits
    the BN statistics slab in training mode, then the BN coefficients (_bn_finalize).
    Returns y, scale, shift, mean, invstd, total."""
    N, cout = x.shape[0], layer.cout
    M = N * OH * OW
    y = empty_nhwc(N, OH, OW, cout, x)
    T, stats = 0, None
    if layer.training:
        T = L.conv_stats_rows(M, cfg)
        stats = torch.empty(T * 2 * cout, device=x.device, dtype=torch.float32)
    L.conv_fwd(x, wf, y, stats, None, k, k, s, p, cfg, **pre_kw)
    return (y,) + _bn_finalize(L, layer, stats, T, M)


def convbn_fwd(layer, x, ctx, train, residual=None, raw=False, pre=None):
    """Interior ConvBN forward: x is an internal NHWC bf16 tensor (module docstring: ctx)."""
    L = lib()
    k, s, p = layer.k, layer.stride, layer.padding
    N, H, W, C = x.shape
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    cout = layer.cout
    wf, _ = packed_weights(layer, need_wd=train)
    cfg = pick_cfg(N * OH * OW, cout, k, s, C, W=OW if (OH, OW) == (H, W) else 0)
    pre_kw = {}
    if pre is not None:
        # the halo tiles (layer 2) and the layer-1 kernel normalise y1 on the fly; for the
        # pipelined tiles of layers 3-4 (cfg 90-93) materialising relu(bn1(y1)) is 1.7 % faster
        # per step than the in-LDS transform that delayed every pipeline stage (and layer 2
        # measures the same either way, as does layer 1: profiles/pipe_pre_materialise_ab_r4q.txt,
        # profiles/layer12_pre_materialise_ab_r4u.txt)
        if _can(cfg, "pre_bn", L):
            pre_kw = dict(pre_scale=pre[0], pre_shift=pre[1])
        else:  # not a halo-kernel shape: materialise the previous BN output
            x = _materialise(x, pre)
            pre = None
    y, scale, shift, mean, invstd, total = conv_stats(L, layer, x, wf, k, s, p, cfg, pre_kw,
                                                      OH, OW)
    if train:
        ctx.update(x=x, y=y, mean=mean, invstd=invstd, has_res=residual is not None,
                   scale=scale, shift=shift, pre=pre, total=total)
    if raw:
        ctx["scale"], ctx["shift"] = scale, shift
        return y
    out = empty_nhwc(N, OH, OW, cout, x)
    # residual + ReLU in training: a 1-bit (out > 0) mask is the backward's ReLU mask source
    # (the residual is not kept; re-reading `out` would cost 16x the bytes)
    mask = (torch.empty(out.numel() // 8, device=x.device, dtype=torch.uint8)
            if (train and residual is not None and layer.relu) else None)
    if callable(residual):  # a shortcut computed on another stream: join it here
        residual = residual()
    L.bn_apply(y, residual, scale, shift, out, layer.relu, mask=mask)
    if train and residual is not None:
        ctx["out"] = out
        ctx["mask"] = mask
    return out


def _dgrad_red(L, red_for, cfg, stride, dx, complete_s2=False):
    """conv_dgrad kwargs that reduce the consumer BN's backward sums in the dgrad epilogue
    (see convbn_bwd ``red_for``); {} when the kernel or the layer does not qualify.

    The kernels with the epilogue (``red_s1`` in csrc/conv_cfg.h: layer1's resident-weight
    kernel, the pipelined tiles of layers 3-4, layer2's halo tile) take a plain ReLU consumer
    (mask from y*scale + shift > 0), the residual block's 1-bit mask, and the fused
    identity-skip add (the consumer's output gradient is dgrad + skip).  The stem (BN + ReLU + max-pool) reduces over the pooled grid: y is its
    value at each window's argmax (ctx["yarg"]), as bn_bwd_reduce_masked does."""
    rl, rctx = red_for
    # stride 2: only a data gradient that writes dx complete in one launch (the projection's
    # 1x1/s2 segment merged in, ``complete_s2``) can reduce its consumer's sums
    kernel_ok = (_can(cfg, "red_s1", L) if stride == 1
                 else stride == 2 and complete_s2 and _can(cfg, "multi_merge_red", L))
    pool = getattr(rl, "pool_k", 0)
    y = rctx.get("yarg") if pool else rctx.get("y")
    if (not kernel_ok or not rl.relu or y is None
            or rctx.get("mean") is None or rctx.get("pre_sums") is not None
            or tuple(y.shape) != tuple(dx.shape)):
        return {}
    mask = None
    if rctx.get("has_res"):
        mask = rctx.get("mask")
        if mask is None:
            return {}
    # layer1's identity-block dgrads (res64 with the fused skip add, reducing the previous
    # block's BN): round 3 measured them 0.3% slower per step (the add/mask epilogue cost the
    # kernel ~100 us, more than the contended pass it saved: profiles/
    # dgrad_bn_reduce_ab_r3s3.txt, red9); with the round-6 packed/bit-extract reduction they
    # gained +0.26 % (profiles/res64_red_add_ab_r6.txt), so they reduce unconditionally (the
    # opt-out switch was removed).  The STEM's pooled-grid sums in the last layer-1 dgrad
    # paid too: +0.5 % (the separate pooled reduce ran next to the full-CU tail weight gradient
    # at ~2 TB/s; profiles/side_stream_sweep_r4f.txt)
    N, H, W, C = dx.shape
    rows = (L.dgrad_s2_red_rows(N, H, W, cfg) if stride == 2
            else L.conv_stats_rows(N * H * W, cfg))
    part = torch.empty(rows * 2 * C, device=dx.device, dtype=torch.float32)
    rctx["pre_sums"] = dict(pre_slab=part, pre_rows=rows)
    kw = dict(red_y=y, red_scale=rctx["scale"], red_shift=rctx["shift"],
              red_mean=rctx["mean"], red_invstd=rctx["invstd"], red_part=part)
    if mask is not None:
        kw["red_mask"] = mask
    return kw


def convbn_bwd(layer, dout, ctx, need_dx, dx_add=None, dx_into=None, fused_skip=False,
               red_for=None, phase=0, shortcut=None):
    """Returns dx (or (dx, dres) when the forward had a residual input).

    ``dx_add``  : tensor added to dx in the dgrad epilogue (identity skip gradient), or
                  ("masked", dout, mask): dout * mask added there (the fused skip below)
    ``dx_into`` : accumulate dx in place into this tensor (downsample branch)
    ``fused_skip``: with a residual input and the forward's 1-bit ReLU mask, the residual
                  gradient dres = dout * mask is NOT materialised; the returned dres is
                  ("masked", dout, mask) for the consumer's dgrad epilogue (saves writing
                  and re-reading one activation-sized tensor per identity block)
    ``red_for``  : (layer, ctx) of the ConvBN + ReLU whose output gradient dx is.  When the
                  dgrad kernel supports it (_dgrad_red), that BN's backward reduction (Σdz, Σdz·x̂)
                  runs in this dgrad's epilogue and is left in its ctx["pre_sums"], so its
                  own backward skips the pass that re-reads dx and y
    ``phase``    : 0 = the whole backward; 1 = only the BatchNorm backward (dy kept in ctx),
                  on the caller's current stream; 2 = the weight and data gradients from
                  phase 1's dy (the caller has made the current stream wait for phase 1)
    ``shortcut`` : {"join": fn} of the block's 1x1/s2 projection (a stride-2 3x3 conv only):
                  fn() orders the current stream after the projection's BatchNorm backward and
                  returns (its dy, its packed data-gradient weights); when the dgrad tile can
                  merge it, the projection's data gradient becomes a second K segment of parity
                  class (0,0) in THIS launch (dx written once, complete, so ``red_for`` applies
                  too) and shortcut["merged"] is set -- the caller then skips its dgrad"""
    L = lib()
    y = ctx["y"]
    cout = y.shape[3]
    k, s, p = layer.k, layer.stride, layer.padding
    # ("masked", dout, mask): the upstream gradient is dout * mask (a projection shortcut fed
    # the block's unmaterialised residual gradient); the BN backward's mode 4 applies exactly
    # that mask, so no ReLU of its own is involved
    in_mask = None
    if isinstance(dout, tuple):
        _, dout, in_mask = dout
        assert not layer.relu and not ctx["has_res"], "masked upstream gradient: linear BN only"
    dout = dout.contiguous()
    # 1. the BN mode
    if in_mask is not None:
        mode = 4       # dz = dout * the residual block's 1-bit mask
    elif not layer.relu:
        mode = 0
    elif ctx["has_res"]:
        # mask needs the residual: the forward's 1-bit mask (4), or the saved output (1)
        mode = 4 if ctx.get("mask") is not None else 1
    else:
        mode = 2       # mask recomputed from y (no `out` read)
    masked_res = fused_skip and ctx["has_res"] and mode == 4
    # 2. BN backward, or phase 1's
    if phase == 2:
        dy, dres = ctx.pop("_bn_out")
        # allocated on the phase-1 stream, read here and on the weight-gradient stream
        dy.record_stream(torch.cuda.current_stream())
        if dres is not None:
            dres.record_stream(torch.cuda.current_stream())
    else:
        work = torch.empty(L.bn_bwd_work(y.numel() // cout, cout), device=y.device,
                           dtype=torch.float32)
        dy, dres = bn_bwd(L, layer, ctx, mode, dout,
                          in_mask if in_mask is not None else ctx.get("mask"),
                          ctx.pop("pre_sums", None) or {}, work,
                          want_dres=ctx["has_res"] and not masked_res)
        if phase == 1:
            ctx["_bn_out"] = (dy, dres)
            return None
    # 3. weight gradient.  red_for is the stem (a pooled ConvBN) only for the first block's c1:
    # the step's last conv
    tail = red_for is not None and bool(getattr(red_for[0], "pool_k", 0))
    launch_wgrad(L, layer, ctx["x"], dy, ctx.get("pre"), k, s, p, tail=tail)
    # 4. data gradient
    dx = (_dgrad(L, layer, ctx["x"], dy, k, s, p, dx_add, dx_into, red_for, shortcut)
          if need_dx else None)
    if ctx["has_res"]:
        return dx, (("masked", dout, ctx["mask"]) if masked_res else dres)
    return dx


def bn_bwd(L, layer, ctx, mode, dout, mask, pre_sums, work, want_dres=False):
    """Shared backward step (interior layers and dmlab.ops.stem): BN backward of ``dout`` in
    ``mode`` (0 linear, 1 / 2 / 4 ReLU mask from ctx["out"] / y / ``mask``, 3: ``dout`` is the
    max-pool's output gradient, gathered through ctx["idx"]); ``pre_sums``: Σdz, Σdz·x̂ already
    reduced.  Writes dgamma / dbeta and returns (dy, dres); dres only when ``want_dres``."""
    y = ctx["y"]
    cout = y.shape[3]
    dy = empty_nhwc(*y.shape, y)
    dres = empty_nhwc(*y.shape, y) if want_dres else None
    acc = 1.0 if layer.accumulate else 0.0
    pooled = mode == 3
    bn_args = (None if pooled else dout, ctx.get("out"), y, ctx["mean"], ctx["invstd"],
               layer.bn_weight.detach(), layer.grad_slot("bn_weight"),
               layer.grad_slot("bn_bias"), acc, mode, ctx["scale"], ctx["shift"],
               dout if pooled else None, ctx.get("idx"),
               getattr(layer, "pool_k", 3), getattr(layer, "pool_s", 2),
               getattr(layer, "pool_p", 1), dy, dres, work)
    total = ctx.get("total")
    if total is None:
        L.bn_backward(*bn_args, mask=mask, **pre_sums)
    else:
        # synchronized BatchNorm.  stage "sums": this rank's Σdz, Σdz·x̂ (reduced here or taken
        # from pre_sums) -> dgamma / dbeta and a float64 row; all-reduce; stage "apply": the
        # coefficients from the global sums and count, then the same apply kernels
        sums = torch.empty(2 * cout, device=y.device, dtype=torch.float64)
        L.bn_backward(*bn_args, mask=mask, stage=1, sums=sums, **pre_sums)
        layer._sync_bn.reduce_sums(sums)
        L.bn_backward(*bn_args, mask=mask, stage=2, sums=sums, total=total)
    return dy, dres


def launch_wgrad(L, layer, x, dy, pre, k, s, p, s2d=False, tail=False):
    """Shared backward step (interior layers and dmlab.ops.stem): dW from x (``pre``: consumed
    as relu(x*scale + shift); ``s2d``: x is the stem's space-to-depth packing) and dy into the
    layer's OIHW fp32 grad slot.  On the Program's side stream when it has one (off the critical
    path; overlaps the following dgrad / BN-backward chain).  Tensors it reads that the main
    stream allocated are recorded on the side stream so the caching allocator does not hand
    their memory out again before the wgrad has read them."""
    N, OH, OW, cout = dy.shape
    C = x.shape[3]
    K = k * k * C
    same = not s2d and (OH, OW) == tuple(x.shape[1:3])
    even = OW if (not s2d and 2 * OH == x.shape[1] and 2 * OW == x.shape[2]) else 0
    wcfg, S = _wgrad_plan(N * OH * OW, cout, K, k, s, C, W=OW if same else 0,
                          rows=N * OH if same else 0, tail=tail, even=even)
    side = getattr(layer._prog, "_wgrad_stream", None)
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())
        for t in (x, dy) + (tuple(pre) if pre is not None else ()):
            t.record_stream(side)
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        slab = torch.empty(S * cout * K, device=dy.device, dtype=torch.float32)
        pre_kw = {}
        if pre is not None:
            if _can(wcfg, "pre_bn", L, wgrad=True):
                pre_kw = dict(pre_scale=pre[0], pre_shift=pre[1])
            else:
                x = _materialise(x, pre)
        L.conv_wgrad(x, dy, layer.grad_slot("weight"), slab, layer.cin, k, k, s, p,
                     1.0 if layer.accumulate else 0.0, S, wcfg, s2d, **pre_kw)


def _dgrad(L, layer, x, dy, k, s, p, dx_add, dx_into, red_for, shortcut):
    """Data gradient of an interior ConvBN (convbn_bwd documents the options); returns dx."""
    cout = dy.shape[3]
    _, wd = packed_weights(layer, need_wd=True)
    N, H, W, Cin = x.shape
    cfg = dgrad_cfg(N * H * W, Cin, k, s, cout, W)
    if dx_into is not None:
        L.conv_dgrad(dy, wd, dx_into, k, k, s, p, dx_into, cfg)
        return dx_into
    dx = empty_nhwc(N, H, W, Cin, x)
    merge_kw = {}
    if (shortcut is not None and s == 2 and k == 3 and p == 1 and dx_add is None
            and _can(cfg, "multi_merge_red", L)
            and H % 2 == 0 and W % 2 == 0):
        dy2, wd2 = shortcut["join"]()
        if (dy2.shape[:3] == dy.shape[:3] and dy2.shape[3] % 64 == 0
                and (not _can(cfg, "merge_same_c", L) or dy2.shape[3] == dy.shape[3])):
            merge_kw = dict(dy2=dy2, wd2=wd2)
            shortcut["merged"] = True
    red_kw = (_dgrad_red(L, red_for, cfg, s, dx, complete_s2=bool(merge_kw))
              if red_for is not None else {})
    if isinstance(dx_add, tuple):
        L.conv_dgrad(dy, wd, dx, k, k, s, p, dx_add[1], cfg, add_mask=dx_add[2], **red_kw)
    else:
        L.conv_dgrad(dy, wd, dx, k, k, s, p, dx_add, cfg, **red_kw, **merge_kw)
    return dx
