"""Mixup / CutMix without a GPU: the stateless draw (dmlab/data/mix.py), its torch reference
against the loop oracle (mix_ref.py), the mixed-target cross-entropy's CPU path, the loader
and task3."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_ref as R
import mix_ref as MR
from dmlab.data import DeviceAugment, DeviceLoader, DeviceMix, TensorDataset
from dmlab.data.mix import mix_reference
from dmlab.nn import CrossEntropyLoss, MixTarget, cross_entropy

ROOT = Path(__file__).resolve().parent.parent
DTYPES = [torch.uint8, torch.float32, torch.bfloat16]
IDS = ["u8", "f32", "bf16"]


# ------------------------------------------------------------------ the draw
def test_constructor_checks():
    with pytest.raises(ValueError):
        DeviceMix()
    with pytest.raises(ValueError):
        DeviceMix(mixup_alpha=-1.0)
    with pytest.raises(ValueError):
        DeviceMix(mixup_alpha=0.2, prob=1.5)


def test_row_is_a_pure_function_of_seed_index_epoch():
    """A dataset index gets the same row at any batch position, batch size or shard (world
    size), apart from the partner column; another epoch or seed gives other rows."""
    mix = DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, seed=3)
    idx = np.arange(200)
    m0, l0 = mix.params(idx, 2, (32, 28))
    assert (m0[:, 1] < MR.ONE).any() and (m0[:, 2] != MR.EMPTY).any()  # both kinds occur
    perm = np.random.default_rng(0).permutation(200)
    for order, B in ((perm, 200), (perm, 16), (perm[1::2], 7), (idx[::4], 50)):
        for s in range(0, len(order), B):
            part = order[s: s + B]
            m, lam = mix.params(part, 2, (32, 28))
            assert torch.equal(m[:, 1:], m0[part][:, 1:]) and torch.equal(lam, l0[part])
    for other in (DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, seed=4).params(idx, 2, (32, 28)),
                  mix.params(idx, 3, (32, 28))):
        assert not torch.equal(other[0][:, 1:], m0[:, 1:])
        assert not torch.equal(other[1], l0)


def test_partner_column_through_the_loader():
    """n = 40 at batch 16: partners B-1-b with B = 16, 16, 8 (the partial batch has its own);
    the target's second label is the partner's."""
    n = 40
    im = torch.zeros(n, 6, 6, 1, dtype=torch.uint8)
    ds = TensorDataset(im, torch.arange(n) % 10)
    mix = DeviceMix(mixup_alpha=1.0, seed=1)
    loader = DeviceLoader(ds, 16, shuffle=True, seed=2, transform=DeviceAugment.pad_crop(0),
                          mix=mix)
    idx, par, tab, lam = loader._host_tables()
    sizes = [16, 16, 8]
    want = torch.cat([torch.arange(B - 1, -1, -1) for B in sizes]).int()
    assert torch.equal(tab[:, 0], want)
    seen = 0
    for (x, t), B in zip(loader, sizes):
        assert isinstance(t, MixTarget) and x.shape[0] == B
        assert torch.equal(t.partner_labels, t.labels.flip(0))
        assert torch.equal(t.lam, lam[seen: seen + B]) and t.lam.dtype == torch.float32
        seen += B
    assert seen == n
    with pytest.raises(ValueError):
        DeviceLoader(ds, 16, mix=mix)


def _sup_distance(x, cdf):
    x = np.sort(x)
    n = x.size
    c = cdf(x)
    return max(np.abs(c - np.arange(n) / n).max(), np.abs(c - np.arange(1, n + 1) / n).max())


@pytest.mark.parametrize("alpha,cdf", [
    (0.5, lambda x: 2.0 / math.pi * np.arcsin(np.sqrt(x))),
    (1.0, lambda x: x),
    (2.0, lambda x: 3 * x ** 2 - 2 * x ** 3),
], ids=["a0.5", "a1", "a2"])
def test_lambda_distribution(alpha, cdf):
    """Kolmogorov distance to the closed-form Beta(α, α) CDF over 20 000 indices below
    2/sqrt(n): a 0.07 % chance bound for a correct sampler, and the seed is fixed."""
    n = 20000
    lam, mixed, cut = DeviceMix(mixup_alpha=alpha, seed=5).lambdas(np.arange(n), 1)
    lam = lam[mixed]
    assert not cut.any() and lam.size > 0.99 * n
    d = _sup_distance(lam, cdf)
    print(f"alpha {alpha}: accepted {lam.size}, sup-distance {d:.5f}, bound {2 / math.sqrt(n):.5f}")
    assert d < 2 / math.sqrt(n)


def test_lambda_distribution_small_alpha():
    """α = 0.2 (Jöhnk): the mean within 4 standard errors of ½ and the variance within 5 % of
    1 / (4 (2α + 1))."""
    n, alpha = 20000, 0.2
    lam, mixed, _ = DeviceMix(cutmix_alpha=alpha, seed=5).lambdas(np.arange(n), 0)
    lam = lam[mixed]
    var = 1.0 / (4 * (2 * alpha + 1))
    print(f"accepted {lam.size}, mean {lam.mean():.5f}, var {lam.var():.5f} (exact {var:.5f})")
    assert lam.size > 0.99 * n
    assert abs(lam.mean() - 0.5) < 4 * math.sqrt(var / n)
    assert abs(lam.var() - var) < 0.05 * var


def test_cutmix_rows():
    OH, OW = 24, 20
    mix = DeviceMix(cutmix_alpha=1.0, seed=7)
    tab, lam = mix.params(np.arange(4000), 0, (OH, OW))
    tab = tab.numpy().astype(np.int64)
    x1, x2 = tab[:, 2] & 0xFFFF, (tab[:, 2] >> 16) + 1
    y1, y2 = tab[:, 3] & 0xFFFF, (tab[:, 3] >> 16) + 1
    mixed = x2 > x1
    assert mixed.sum() > 3000 and (~mixed).sum() > 0  # a tiny λ0 side rounds to an empty box
    assert (tab[:, 1] == MR.ONE).all()
    assert (x1[mixed] >= 0).all() and (x2[mixed] <= OW).all() and (y2[mixed] > y1[mixed]).all()
    assert (y1[mixed] >= 0).all() and (y2[mixed] <= OH).all()
    area = np.where(mixed, (x2 - x1) * (y2 - y1), 0)
    want = (1.0 - area.astype(np.float64) / (OH * OW)).astype(np.float32)
    assert np.array_equal(lam.numpy(), want)
    # the unmixed rows are exactly the unmixed row
    um = tab[~mixed]
    assert (um[:, 0] == np.nonzero(~mixed)[0]).all() and (um[:, 2:] == MR.EMPTY).all()
    assert (lam.numpy()[~mixed] == 1.0).all()


def test_mixup_rows():
    tab, lam = DeviceMix(mixup_alpha=0.8, seed=7).params(np.arange(1000), 0, (8, 8))
    assert (tab[:, 2:] == MR.EMPTY).all()
    assert torch.equal(lam, tab[:, 1].float() / 65536)  # the label weight IS the pixel weight
    assert 0 <= int(tab[:, 1].min()) and int(tab[:, 1].max()) <= MR.ONE
    assert torch.equal(tab[:, 0], torch.arange(999, -1, -1).int())


def _loader(ds, mix, dev=None):
    aug = DeviceAugment.random_resized_crop((10, 9), flip=0.5, seed=2)
    return DeviceLoader(ds if dev is None else ds.to(dev), 16, shuffle=True, seed=1,
                        transform=aug, mix=mix)


def test_prob_zero_is_the_unmixed_loader():
    tab, lam = DeviceMix(mixup_alpha=0.3, cutmix_alpha=1.0, prob=0.0).params(np.arange(64), 0,
                                                                          (8, 8))
    assert torch.equal(tab, torch.tensor([MR.unmixed_row(b) for b in range(64)]).int())
    assert bool((lam == 1).all())
    n = 40
    g = torch.Generator().manual_seed(3)
    im = torch.randint(0, 256, (n, 12, 11, 3), generator=g, dtype=torch.uint8)
    ds = TensorDataset(im, torch.arange(n))
    for (xm, t), (x, y) in zip(_loader(ds, DeviceMix(cutmix_alpha=1.0, prob=0.0)),
                               _loader(ds, None)):
        assert torch.equal(xm, x) and torch.equal(t.labels, y)
        assert torch.equal(t.partner_labels, y) and bool((t.lam == 1).all())


# ------------------------------------------------------------------ torch reference vs the loop oracle
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("src,out,B,C", MR.CASES, ids=MR.CASE_IDS)
def test_mix_reference_equals_loop_oracle(src, out, B, C, dtype):
    im, batches = MR.case(src, out, B, C)
    x = R.torch_images(im, dtype)
    for idx, par, mix, S in batches:
        got = mix_reference(x, torch.tensor(idx), torch.tensor(par, dtype=torch.int32),
                            torch.tensor(mix, dtype=torch.int32), out[0], out[1])
        want = MR.expected(S, mix, dtype)
        assert got.dtype == dtype and torch.equal(got, want), (idx, mix)


def test_oracle_unmixed_is_the_augmentation_oracle():
    (src, out), B, C = MR.SHAPES[0], 5, 3
    _, batches = MR.case(src, out, B, C)
    for dtype in DTYPES:
        for idx, par, _, S in batches:
            mix = [MR.unmixed_row(b) for b in range(B)]
            assert torch.equal(MR.expected(S, mix, dtype), R.expected(S, dtype))


# ------------------------------------------------------------------ mixed cross-entropy, CPU path
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C", [(1, 10), (5, 10), (13, 65)])
def test_mixed_cross_entropy_cpu(B, C, eps):
    g = torch.Generator().manual_seed(B + C)
    x = (torch.randn(B, C, generator=g) * 3).requires_grad_(True)
    ya, yb, lam = MR.mixed_ce_rows(B, C)
    loss = CrossEntropyLoss(eps)(x, MixTarget(ya, yb, lam))
    loss.backward()
    xr = x.detach().double().requires_grad_(True)
    ref = MR.mixed_ce_reference(xr, ya, yb, lam, eps)
    ref.backward()
    torch.testing.assert_close(loss, ref.float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(x.grad, xr.grad.float(), rtol=1e-5, atol=1e-6)
    if B >= 5:
        assert not x.grad[2:5].any()  # invalid rows: zero gradient
    # lam = 1 everywhere is the one-label loss
    one = cross_entropy(x.detach(), MixTarget(ya.clamp(0, C - 1), yb.clamp(0, C - 1),
                                              torch.ones(B)), eps)
    torch.testing.assert_close(one, cross_entropy(x.detach(), ya.clamp(0, C - 1), eps))


# ------------------------------------------------------------------ task3
def _task3(args, tmp_path):
    env = dict(os.environ, PYTHONPATH=str(ROOT), OMP_NUM_THREADS="2")
    return subprocess.run([sys.executable, "-m", "dmlab.tasks.task3", "--device", "cpu",
                           "--synthetic", "--train-samples", "256", "--epochs", "1", "--no-test"]
                          + args, cwd=tmp_path, env=env, capture_output=True, text=True,
                          timeout=300)


@pytest.mark.slow
def test_task3_mixing_runs_and_reports(tmp_path):
    js = tmp_path / "r.json"
    r = _task3(["--mixup", "0.2", "--cutmix", "1.0", "--max-steps", "3", "--json", str(js)],
               tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    st = json.loads(js.read_text())
    assert st["mixup"] == 0.2 and st["cutmix"] == 1.0 and st["mix_prob"] == 1.0
    assert st["steps"] == 3 and "fused" not in st


@pytest.mark.slow
def test_task3_fused_with_mixing_exits(tmp_path):
    r = _task3(["--fused", "1", "--mixup", "0.2"], tmp_path)
    assert r.returncode != 0
    assert "--mixup and --cutmix need the layer-wise loop" in r.stderr
