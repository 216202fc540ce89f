"""The cross-rank BatchNorm kernels (csrc/bn_pool.hip: bn_sync_local, bn_sync_finalize, the
two-stage bn_backward) in one process: the ranks are emulated by calling the local kernel once
per shard and stacking the rows / adding the sums, as the all-gather and all-reduce would."""
import pytest
import torch
import torch.nn.functional as F

from dmlab.ops._native import lib

pytestmark = pytest.mark.gpu

EPS = 1e-5
COUNTS = {1: [777], 2: [1, 1000], 8: [1, 5, 64, 100, 333, 1000, 2, 4099]}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


def _slab(x, T):
    """[T][2][C] fp32 partial (Σx, Σx²) rows of the elements x [n, C], dealt round-robin to
    the T rows (rows past n stay zero, as tiles without pixels do)."""
    n, C = x.shape
    rows = torch.arange(n, device=x.device) % T
    xd = x.double()
    s = torch.zeros(T, C, device=x.device, dtype=torch.float64).index_add_(0, rows, xd)
    q = torch.zeros(T, C, device=x.device, dtype=torch.float64).index_add_(0, rows, xd * xd)
    return torch.stack([s, q], 1).float().contiguous()


def _merge64(slabs, counts):
    """float64 merge of the same fp32 slabs, rank order: (mean, var, N)."""
    rows = []
    for sl, n in zip(slabs, counts):
        s, q = sl[:, 0].double().sum(0), sl[:, 1].double().sum(0)
        rows.append((s / n, (q - s * s / n).clamp_min(0), float(n)))
    N = sum(n for _, _, n in rows)
    mean = sum(n * m for m, _, n in rows) / N
    M2 = sum(m2 + n * (m - mean) ** 2 for m, m2, n in rows)
    return mean, M2 / N, N


def _sync_forward(L, slabs, counts, gamma, beta, rm, rv, nb):
    dev, C = gamma.device, gamma.numel()
    f = dict(device=dev, dtype=torch.float32)
    rows = torch.empty(len(slabs), 2 * C + 1, device=dev, dtype=torch.float64)
    for r, (sl, n) in enumerate(zip(slabs, counts)):
        L.bn_sync_local(sl.view(-1), sl.shape[0], float(n), C, rows[r], torch.empty(512 * C, **f))
    out = [torch.empty(C, **f) for _ in range(4)]  # scale, shift, mean, invstd
    total = torch.zeros(1, device=dev, dtype=torch.float64)
    L.bn_sync_finalize(rows, gamma, beta, rm, rv, 0.1, EPS, *out, nb, total)
    return out, total, rows


@pytest.mark.parametrize("C,T,ws,far", [(C, T, ws, False) for C in (64, 80, 512)
                                        for T in (1, 129, 2049) for ws in (1, 2, 8)]
                         + [(80, 129, 2, True)])
def test_sync_forward(dev, C, T, ws, far):
    """T = 2049 takes the slab_colsum pre-pass; ``far``: channel means 50 standard deviations
    from zero (Σy² - (Σy)²/n cancels 3-4 digits; the float64 rows keep the rest)."""
    L = lib()
    g = torch.Generator(device=dev).manual_seed(3)
    counts = COUNTS[ws]
    f = dict(device=dev, dtype=torch.float32)
    slabs = []
    for r, n in enumerate(counts):
        x = torch.randn(n, C, device=dev, generator=g) * (1.0 + 0.1 * r) + 0.3 * r
        if far:
            x = x + 50.0 * (1.0 + 0.1 * r)
        slabs.append(_slab(x, T))
    gamma, beta = torch.rand(C, **f) + 0.5, torch.randn(C, **f)
    rm, rv = torch.randn(C, **f), torch.rand(C, **f) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    nb = torch.zeros(1, dtype=torch.int64, device=dev)
    (scale, shift, mean, invstd), total, rows = _sync_forward(L, slabs, counts, gamma, beta, rm, rv, nb)
    mu, var, N = _merge64(slabs, counts)
    assert total.item() == float(sum(counts)) == N
    assert torch.equal(rows[:, 2 * C].cpu(), torch.tensor(counts, dtype=torch.float64))
    torch.testing.assert_close(mean.double(), mu, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(invstd.double(), 1 / torch.sqrt(var + EPS), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(scale, gamma * invstd, rtol=1e-6, atol=0)
    torch.testing.assert_close(shift, beta - mean * scale, rtol=1e-5, atol=1e-6)
    unbiased = var * N / (N - 1)
    torch.testing.assert_close(rm.double(), 0.9 * rm0.double() + 0.1 * mu, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(rv.double(), 0.9 * rv0.double() + 0.1 * unbiased, rtol=1e-3,
                               atol=1e-3)
    assert int(nb.item()) == 1
    again, _, _ = _sync_forward(L, slabs, counts, gamma, beta, rm, rv, nb)
    assert int(nb.item()) == 2  # one increment per call
    for a, b in zip(again, (scale, shift, mean, invstd)):
        assert torch.equal(a, b)
    if ws == 1:  # one rank: what the per-rank finalize gives, up to the last fp32 rounding
        ref = [torch.empty(C, **f) for _ in range(4)]
        L.bn_stats_finalize(slabs[0].view(-1), T, float(counts[0]), gamma, beta, None, None, 0.1,
                            EPS, *ref, torch.empty(512 * C, **f))
        for a, b in zip((scale, shift, mean, invstd), ref):
            torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------ backward
def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("C,shards,H", [(64, (3, 5), 6), (512, (2, 1), 2)])
@pytest.mark.parametrize("mode", [0, 1, 2, 4, 3])
def test_sync_backward(dev, C, shards, H, mode):
    """Two-stage BN backward over two shards against float64 autograd of F.batch_norm (plus
    residual / ReLU / pool per mode) over the concatenated shards; each mode with the internal
    reduction and with pre-reduced partial rows (pre_slab), gbeta 0 and 1."""
    L = lib()
    if mode == 3:
        H = 8  # the 3x3/s2/p1 pool
    relu, res = mode != 0, mode in (1, 4)
    g = torch.Generator(device=dev).manual_seed(5)
    f = dict(device=dev, dtype=torch.float32)
    bf = dict(device=dev, dtype=torch.bfloat16)
    ys = [(torch.randn(n, H, H, C, device=dev, generator=g) * (1.5 - 0.5 * r) + 0.7 * r).bfloat16()
          for r, n in enumerate(shards)]
    rs = [torch.randn(n, H, H, C, device=dev, generator=g).bfloat16() for n in shards]
    gamma = torch.rand(C, device=dev, generator=g) + 0.5
    beta = torch.randn(C, device=dev, generator=g) * 0.5
    counts = [n * H * H for n in shards]
    slabs = [_slab(y.float().view(-1, C), 1) for y in ys]
    (scale, shift, mean, invstd), total, _ = _sync_forward(L, slabs, counts, gamma, beta, None,
                                                           None, None)
    # float64 reference over the concatenated shards
    yc = _nchw(torch.cat(ys).double()).requires_grad_(True)
    g_, b_ = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.batch_norm(yc, None, None, g_, b_, True, 0.0, EPS)
    z.retain_grad()
    t = z + _nchw(torch.cat(rs).double()) if res else z
    t = F.relu(t) if relu else t
    t = F.max_pool2d(t, 3, 2, 1) if mode == 3 else t
    douts = [torch.randn(n, *t.shape[2:], C, device=dev, generator=g).bfloat16() for n in shards]
    t.backward(_nchw(torch.cat(douts).double()))
    dz_ref, dy_ref = _nhwc(z.grad), _nhwc(yc.grad)
    mu64 = yc.detach().mean((0, 2, 3))
    is64 = 1 / torch.sqrt(yc.detach().var((0, 2, 3), unbiased=False) + EPS)
    xhat = (_nhwc(yc.detach()) - mu64) * is64
    # native forward tails per shard: out / mask / pool codes
    fw = []
    for y, r in zip(ys, rs):
        if mode == 3:
            n = y.shape[0]
            out = torch.empty(n, 4, 4, C, **bf)
            idx = torch.empty(n, 4, 4, C, device=dev, dtype=torch.uint8)
            L.bn_relu_maxpool(y, scale, shift, out, idx, 3, 2, 1)
            fw.append(dict(idx=idx))
        else:
            out = torch.empty_like(y)
            mask = torch.empty(y.numel() // 8, device=dev, dtype=torch.uint8) if mode == 4 else None
            L.bn_apply(y, r if res else None, scale, shift, out, relu, mask=mask)
            fw.append(dict(out=out, mask=mask))
    lo = 0
    bounds = []
    for n in shards:
        bounds.append((lo, lo + n))
        lo += n

    def call(r, stage, dg, db, gbeta, sums, dy, dres, pre):
        y, w = ys[r], fw[r]
        work = torch.empty(L.bn_bwd_work(y.numel() // C, C), **f)
        L.bn_backward(None if mode == 3 else douts[r], w.get("out"), y, mean, invstd, gamma, dg,
                      db, gbeta, mode, scale, shift, douts[r] if mode == 3 else None,
                      w.get("idx"), 3, 2, 1, dy, dres, work, mask=w.get("mask"), stage=stage,
                      sums=sums, total=total if stage == 2 else None,
                      **(pre if stage == 1 else {}))

    for use_pre in (False, True):
        for gbeta in (0.0, 1.0):
            local, filled = [], []
            for r, (a, b) in enumerate(bounds):
                pre = {}
                if use_pre:  # 3 uneven row groups of this shard's Σdz, Σdz·x̂, as an epilogue leaves
                    dz = dz_ref[a:b].reshape(-1, C)
                    xh = xhat[a:b].reshape(-1, C)
                    cut = [0, 1, dz.shape[0] // 2, dz.shape[0]]
                    part = torch.stack([torch.cat([dz[i:j].sum(0), (dz[i:j] * xh[i:j]).sum(0)])
                                        for i, j in zip(cut[:-1], cut[1:])]).float().contiguous()
                    pre = dict(pre_slab=part.view(-1), pre_rows=3)
                dg, db = torch.randn(C, **f), torch.randn(C, **f)  # pre-filled gradient slots
                filled.append((dg.clone(), db.clone()))
                sums = torch.empty(2 * C, device=dev, dtype=torch.float64)
                dy = torch.full_like(ys[r], float("nan"))
                call(r, 1, dg, db, gbeta, sums, dy, None, pre)
                assert torch.isnan(dy.float()).all()  # stage "sums" applies nothing
                local.append((dg, db, sums))
            glob = local[0][2] + local[1][2]  # the all-reduce
            for r, (a, b) in enumerate(bounds):
                dg, db, sums = local[r]
                dz = dz_ref[a:b].reshape(-1, C)
                want_db = gbeta * filled[r][1].double() + dz.sum(0)
                want_dg = gbeta * filled[r][0].double() + (dz * xhat[a:b].reshape(-1, C)).sum(0)
                assert _rel(db, want_db) < 1e-2, (mode, use_pre, gbeta, r)
                assert _rel(dg, want_dg) < 1e-2, (mode, use_pre, gbeta, r)
                keep = (dg.clone(), db.clone())
                dy = torch.empty_like(ys[r])
                dres = torch.empty_like(ys[r]) if res else None
                call(r, 2, dg, db, gbeta, glob.clone(), dy, dres, None)
                assert torch.equal(dg, keep[0]) and torch.equal(db, keep[1])  # untouched
                assert _rel(dy, dy_ref[a:b]) < 1e-2, (mode, use_pre, gbeta, r)
                if res:
                    assert _rel(dres, dz_ref[a:b]) < 1e-2, (mode, use_pre, gbeta, r)
