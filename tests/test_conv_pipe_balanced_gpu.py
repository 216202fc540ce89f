"""The balanced schedule of the pipelined conv (csrc/conv_pipe.hip, cfg 90): a persistent grid
of G workgroups splits the tiles' K steps evenly and hands partial fp32 accumulators from one
workgroup to the next.  Because the hand-off continues the same MFMA chain from the same fp32
values, every output, statistics row and reduction part row must equal the data-parallel
launch's bit for bit; on integer-valued operands (tests/exact_conv.py; preconditions asserted
in tests/test_conv_pipe_plan_cpu.py) both must also equal the float64 reference exactly.

``balance="off"`` forces the data-parallel launch, ``balance=G`` the balanced one on G
workgroups wherever it is eligible; ``conv_pipe_balance_state()`` counts the balanced launches
(and raises if a workgroup timed out waiting for its neighbour), which is how the tests know
which schedule ran."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import exact_conv as ec
import pipe_balanced_cases as pc
from dmlab.ops._native import lib
from test_exact_conv_gpu import DevCase, _stats_sum

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
CFG = 90


@functools.lru_cache(maxsize=None)
def _case(dev, geom):
    return DevCase(dev, geom)


def _launches():
    """Balanced launches so far over every workspace (synchronises; raises on a timeout)."""
    return sum(n for _, n, _ in lib().conv_pipe_balance_state())


def _expect(before, balanced):
    assert _launches() - before == (1 if balanced else 0), "which schedule ran"


def _fwd(d, balance, add=False, stats=True):
    N, H, W, Cin, Cout, k, s, p = d.geom
    OH, OW = ec.out_hw(d.geom)
    y, ychk = d.out((N, OH, OW, Cout))
    T = lib().conv_stats_rows(N * OH * OW, CFG, Cout)
    st, schk = d.out((T * 2 * Cout,), F32)
    lib().conv_fwd(d.xn, d.wf, y, st if stats else None, d.add_y if add else None, k, k, s, p, CFG,
                   balance=balance)
    ychk(f"fwd balance={balance}: y")
    if stats:
        schk(f"fwd balance={balance}: stats")
    d.check_inputs()
    return y, st, T


def _fwd_pair(d, G, balanced=True, add=False, stats=True):
    """Data-parallel and balanced forward: equal bit for bit, and equal to the reference."""
    N, H, W, Cin, Cout, k, s, p = d.geom
    n0 = _launches()
    y0, s0, T = _fwd(d, "off", add, stats)
    _expect(n0, False)
    y1, s1, _ = _fwd(d, G, add, stats)
    _expect(n0, balanced)
    assert torch.equal(y0, y1), "y differs from the data-parallel launch"
    ec.assert_exact(y1, d.r.y_add if add else d.r.y, f"fwd G={G}: y")
    if stats:
        assert torch.equal(s0, s1), "statistics slab differs from the data-parallel launch"
        ec.assert_exact(_stats_sum(s1, T, Cout), d.r.stats, f"fwd G={G}: stats")


def _dgrad(d, balance, mode="plain", red=None):
    N, H, W, Cin, Cout, k, s, p = d.geom
    dx, xchk = d.out((N, H, W, Cin))
    add, kw, part, rows = None, {}, None, 0
    if mode == "masked":
        add, kw["add_mask"] = d.add_x, d.keep_add
    elif mode == "merged":
        kw.update(dy2=d.dy2, wd2=d.wd2)
    if red:
        rows = (lib().conv_stats_rows(N * H * W, CFG, Cin) if s == 1
                else lib().dgrad_s2_red_rows(N, H, W, CFG))
        part, pchk = d.out((rows * 2 * Cin,), F32)
        kw.update(red_y=d.red_y, red_scale=d.red_scale, red_shift=d.red_shift, red_mean=d.red_mean,
                  red_invstd=d.red_invstd, red_part=part)
        if red == "bits":
            kw["red_mask"] = d.red_keep
    lib().conv_dgrad(d.dy, d.wd, dx, k, k, s, p, add, CFG, balance=balance, **kw)
    xchk(f"dgrad balance={balance} {mode} red={red}: dx")
    if red:
        pchk(f"dgrad balance={balance} {mode} red={red}: red_part")
    d.check_inputs()
    return dx, part, rows


def _dgrad_pair(d, G, mode="plain", red=None, balanced=True):
    Cin = d.geom[3]
    n0 = _launches()
    dx0, p0, rows = _dgrad(d, "off", mode, red)
    _expect(n0, False)
    dx1, p1, _ = _dgrad(d, G, mode, red)
    _expect(n0, balanced)
    assert torch.equal(dx0, dx1), "dx differs from the data-parallel launch"
    name = {"plain": "dx", "masked": "dx_masked", "merged": "dx_merged"}[mode]
    ec.assert_exact(dx1, getattr(d.r, name), f"dgrad G={G} {mode}: dx")
    if red:
        assert torch.equal(p0, p1), "red_part differs from the data-parallel launch"
        ec.assert_exact(_stats_sum(p1, rows, Cin), d.r.red[(name, red)], f"dgrad G={G} {mode}: red")


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("G", [4, 3])
@pytest.mark.parametrize("stats", [True, False])
def test_fwd_split_tiles(dev, G, stats):
    """5 tiles of 36 K steps: G = 4 ends its ranges inside tiles 1, 2 and 3 (45 steps each),
    G = 3 inside tiles 1 and 3 (60 steps each)."""
    _fwd_pair(_case(dev, pc.FWD), G, stats=stats)


def test_fwd_split_tiles_add(dev):
    _fwd_pair(_case(dev, pc.FWD), 4, add=True)


def test_fwd_aligned_ranges(dev):
    """4 tiles on 2 workgroups: every range ends on a tile boundary, no slot is exchanged."""
    _fwd_pair(_case(dev, pc.ALIGNED), 2)


@pytest.mark.parametrize("G", [4, 3])
def test_fwd_one_tap(dev, G):
    """1x1 taps, S = C / 64 = 4: ranges of 5 steps (G = 4) and 6 / 7 / 7 (G = 3)."""
    _fwd_pair(_case(dev, pc.ONE_TAP), G)


# ------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("mode,red", [("plain", None), ("masked", None), ("plain", "y"),
                                      ("masked", "bits"), ("plain", "bits"), ("masked", "y")])
def test_dgrad_layer4_like(dev, mode, red):
    """4 M tiles (the last with 16 valid rows) x 2 N tiles of 72 K steps on G = 5: ranges of
    116 / 115 steps.  ADD with the identity mask, and RED in both mask modes."""
    _dgrad_pair(_case(dev, pc.L4), 5, mode, red)


def test_dgrad_aligned_ranges(dev):
    _dgrad_pair(_case(dev, pc.ALIGNED), 2, "plain", "y")


def test_dgrad_one_tap(dev):
    _dgrad_pair(_case(dev, pc.ONE_TAP), 4, "plain", "y")


# ------------------------------------------------------------------ workspace reuse
def test_workspace_reuse_back_to_back(dev):
    """Different shapes and grids back to back on one stream reuse the slots and the flags
    (nothing is reset between launches: the flag carries the launch's sequence number)."""
    a, b = _case(dev, pc.FWD), _case(dev, pc.L4)
    want_y = _fwd(a, "off")[0].clone()
    want_dx = _dgrad(b, "off", "plain", "y")[0].clone()
    n0 = _launches()
    outs = []
    for G in (4, 3, 4):
        outs.append((want_y, _fwd(a, G)[0].clone()))
        outs.append((want_dx, _dgrad(b, 5, "plain", "y")[0].clone()))
        outs.append((want_dx, _dgrad(b, 7, "plain", "y")[0].clone()))
    assert _launches() - n0 == 9
    for want, got in outs:
        assert torch.equal(want, got)


# ------------------------------------------------------------------ ineligible requests
def test_more_workgroups_than_tiles_takes_the_old_path(dev):
    _fwd_pair(_case(dev, pc.FWD), 8, balanced=False)   # T = 5
    _fwd_pair(_case(dev, pc.FWD), 5, balanced=False)   # T == G: one round already
    _dgrad_pair(_case(dev, pc.L4), 16, "plain", "y", balanced=False)  # T = 8


@pytest.mark.parametrize("mode,red", [("plain", None), ("merged", None), ("plain", "y"),
                                      ("merged", "bits")])
def test_stride2_dgrad_takes_the_old_path(dev, mode, red):
    """Four parity classes in one launch (and the merged projection segment): never balanced."""
    _dgrad_pair(_case(dev, pc.STRIDE2), 2, mode, red, balanced=False)


def test_auto_keeps_small_grids_data_parallel(dev):
    d = _case(dev, pc.FWD)
    n0 = _launches()
    y, _, _ = _fwd(d, "auto")
    _expect(n0, False)
    ec.assert_exact(y, d.r.y, "fwd auto: y")
    with pytest.raises(RuntimeError):
        _fwd(d, "sometimes")
    with pytest.raises(RuntimeError):
        _fwd(d, 0)


# ------------------------------------------------------------------ random values
def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


def _random_operands(dev, geom, seed):
    N, H, W, Cin, Cout, k, s, p = geom
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g).bfloat16()
    w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).bfloat16()
    wf = torch.empty(Cout, k, k, Cin, device=dev, dtype=BF)
    wd = torch.empty(Cin, k, k, Cout, device=dev, dtype=BF)
    lib().pack_weights(w.float().to(dev), wf, wd, Cin)
    return x, w, wf, wd, g


def test_fwd_random_values(dev):
    """Random operands: bit for bit the data-parallel launch; the float64 reference within the
    tolerance of the pipelined tiles' tests (tests/test_native_resnet_kernels.py)."""
    N, H, W, Cin, Cout, k, s, p = pc.FWD
    x, w, wf, _, _ = _random_operands(dev, pc.FWD, 3)
    xn = x.to(dev)
    T = lib().conv_stats_rows(N * H * W, CFG, Cout)
    outs = []
    n0 = _launches()
    for balance in ("off", 4):
        y = torch.empty(N, H, W, Cout, device=dev, dtype=BF)
        st = torch.empty(T * 2 * Cout, device=dev)
        lib().conv_fwd(xn, wf, y, st, None, k, k, s, p, CFG, balance=balance)
        outs.append((y, st))
    _expect(n0, True)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, s, p).permute(0, 2, 3, 1)
    assert _rel(outs[1][0].cpu(), ref) < 6e-3


def test_dgrad_random_values(dev):
    N, H, W, Cin, Cout, k, s, p = pc.L4
    _, w, _, wd, g = _random_operands(dev, pc.L4, 4)
    dy = torch.randn(N, H, W, Cout, generator=g).bfloat16()
    red_y = torch.randn(N, H, W, Cin, generator=g).bfloat16().to(dev)
    vec = lambda lo, hi: (torch.rand(Cin, generator=g) * (hi - lo) + lo).to(dev)
    sc, sh, mu, istd = vec(0.5, 2.0), vec(-1.0, 1.0), vec(-0.5, 0.5), vec(0.5, 2.0)
    dyn = dy.to(dev)
    rows = lib().conv_stats_rows(N * H * W, CFG, Cin)
    outs = []
    n0 = _launches()
    for balance in ("off", 5):
        dx = torch.empty(N, H, W, Cin, device=dev, dtype=BF)
        part = torch.empty(rows * 2 * Cin, device=dev)
        lib().conv_dgrad(dyn, wd, dx, k, k, s, p, None, CFG, red_y=red_y, red_scale=sc, red_shift=sh,
                         red_mean=mu, red_invstd=istd, red_part=part, balance=balance)
        outs.append((dx, part))
    _expect(n0, True)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double().permute(0, 3, 1, 2), s, p)
    assert _rel(outs[1][0].cpu(), ref.permute(0, 2, 3, 1)) < 6e-3
