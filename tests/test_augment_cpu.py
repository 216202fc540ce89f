"""The augmentation's host side (dmlab/data/augment.py): Philox known answers, the parameter
tables, the torch CPU path against the per-pixel loop oracle (augment_ref.py) and against torch
ops, the loader with a transform, and the task3 flags."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as R
from dist_helpers import free_port
from dmlab.data import DeviceAugment, DeviceLoader, MySampler, TensorDataset, philox4x32

DTYPES = [torch.uint8, torch.float32, torch.bfloat16]


# ------------------------------------------------------------------ Philox4x32-10
@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    got = philox4x32(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert " ".join(f"{int(v):08x}" for v in got) == want
    # vectorised: the same row inside a batch of counters
    many = philox4x32(np.array([[1, 2, 3, 4], ctr, [5, 6, 7, 8]], dtype=np.uint64),
                      np.array(key, dtype=np.uint64))
    assert " ".join(f"{int(v):08x}" for v in many[1]) == want


# ------------------------------------------------------------------ parameters
def _unpack(tab):
    t = tab.numpy().astype(np.int64)
    return dict(X0=t[:, 0], Y0=t[:, 1], DX=t[:, 2], DY=t[:, 3], flags=t[:, 4],
                xlo=t[:, 5] & 0xFFFF, xhi=(t[:, 5] >> 16) & 0xFFFF,
                ylo=t[:, 6] & 0xFFFF, yhi=(t[:, 6] >> 16) & 0xFFFF, last=t[:, 7])


AUGS = [
    lambda **kw: DeviceAugment.pad_crop(4, flip=0.5, **kw),
    lambda **kw: DeviceAugment.random_resized_crop((24, 20), flip=0.5, **kw),
    lambda **kw: DeviceAugment.center(24, **kw),
]


@pytest.mark.parametrize("make", AUGS)
@pytest.mark.parametrize("size", [(32, 32), (13, 11), (40, 200)])
def test_boxes_inside_image(make, size):
    H, W = size
    aug = make(size=size, seed=3)
    tab = aug.params(torch.arange(3000), epoch=2)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (3000, 8)
    p = _unpack(tab)
    assert (p["xlo"] <= p["xhi"]).all() and (p["xhi"] < W).all()   # w >= 1, inside
    assert (p["ylo"] <= p["yhi"]).all() and (p["yhi"] < H).all()
    assert (p["last"] == 0).all() and (p["DX"] > 0).all() and (p["DY"] > 0).all()


@pytest.mark.parametrize("make", AUGS)
def test_params_stateless_and_keyed_by_index(make):
    aug = make(size=(32, 28), seed=11)
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, 1 << 40, (500,), generator=g)
    a, b = aug.params(idx, 3), aug.params(idx, 3)
    assert torch.equal(a, b)
    perm = torch.randperm(500, generator=g)
    assert torch.equal(a[perm], aug.params(idx[perm], 3))
    # a sub-batch, another batch size: the rows are the same
    assert torch.equal(a[100:137], aug.params(idx[100:137], 3))
    if aug.mode != "center":
        assert not torch.equal(a, aug.params(idx, 4))
        assert not torch.equal(a, make(size=(32, 28), seed=12).params(idx, 3))
        assert not torch.equal(a, make(size=(32, 28), seed=11 + (1 << 32)).params(idx, 3))


def test_flip_probability():
    idx = torch.arange(4096)
    count = lambda p: int((DeviceAugment.pad_crop(2, flip=p, size=(8, 8), seed=5)
                           .params(idx, 0)[:, 4] & 1).sum())
    n = count(0.5)
    print("flips at p = 0.5:", n)
    assert abs(n - 2048) <= 160  # 5 sigma, sigma = sqrt(4096) / 2 = 32
    assert count(0.0) == 0 and count(1.0) == 4096


def test_rrc_full_image_and_fallback_boxes():
    idx = torch.arange(512)
    full = DeviceAugment.random_resized_crop(16, scale=(1, 1), ratio=(1, 1), size=(32, 32))
    x0, y0, w, h = full.boxes(idx, 0)
    assert (x0 == 0).all() and (y0 == 0).all() and (w == 32).all() and (h == 32).all()
    p = _unpack(full.params(idx, 0))
    assert (p["xlo"] == 0).all() and (p["xhi"] == 31).all() and (p["yhi"] == 31).all()
    assert (p["DX"] == (32 << 16) // 16).all() and (p["X0"] == 65536 - 32768).all()
    # ratio 2 at full area never fits a square image (w = round(sqrt(2) * 32) > 32):
    # torchvision's fallback is w = W, h = round(W / ratio), centred
    fb = DeviceAugment.random_resized_crop(16, scale=(1, 1), ratio=(2, 2), size=(32, 32))
    x0, y0, w, h = fb.boxes(idx, 0)
    assert (w == 32).all() and (h == 16).all() and (x0 == 0).all() and (y0 == 8).all()


def test_rrc_matches_a_scalar_reimplementation():
    """get_params written out per index with Python floats, fed the same uniforms."""
    import math

    from dmlab.data.augment import _uniform

    H, W = 37, 50
    aug = DeviceAugment.random_resized_crop(8, size=(H, W), seed=9)
    idx = np.arange(300)
    bx = aug.boxes(idx, 1)
    accepted_late = 0
    for j, i in enumerate(idx):
        want = None
        for t in range(1, 11):
            u = _uniform(9, np.array([i]), 1, t)[0]
            area = H * W * (0.08 + u[0] * (1.0 - 0.08))
            ar = math.exp(math.log(3 / 4) + u[1] * (math.log(4 / 3) - math.log(3 / 4)))
            w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
            if 0 < w <= W and 0 < h <= H:
                want = (int(u[2] * (W - w + 1)), int(u[3] * (H - h + 1)), w, h)
                accepted_late += t > 1
                break
        assert want is not None
        assert tuple(int(v[j]) for v in bx) == want
    assert accepted_late > 0  # some index needed more than one try


def test_pad_crop_offsets_cover_the_range():
    P = 3
    p = _unpack(DeviceAugment.pad_crop(P, size=(10, 12), seed=1).params(torch.arange(2000), 0))
    assert set((p["X0"] >> 16).tolist()) == set(range(-P, P + 1))
    assert set((p["Y0"] >> 16).tolist()) == set(range(-P, P + 1))
    assert (p["X0"] & 0xFFFF == 0).all() and (p["DX"] == 65536).all() and (p["DY"] == 65536).all()
    assert (p["flags"] & 2 == 2).all()  # zero fill
    assert (p["xlo"] == 0).all() and (p["xhi"] == 11).all() and (p["yhi"] == 9).all()


def test_eval_transform_is_deterministic():
    rrc = DeviceAugment.random_resized_crop(24, flip=0.5, size=(32, 32))
    ev = rrc.eval()
    idx = torch.arange(64)
    assert ev.mode == "center" and ev.out == (24, 24)
    assert torch.equal(ev.params(idx, 0), ev.params(idx.flip(0), 7))  # the same row everywhere
    pc = DeviceAugment.pad_crop(4, flip=0.5, size=(8, 8)).eval()
    t = pc.params(idx, 3)
    assert (t[:, 0] == 0).all() and (t[:, 1] == 0).all() and (t[:, 4] & 1 == 0).all()


# ------------------------------------------------------------------ torch path vs the oracle
def _layouts(t_nhwc):
    """The same pixels as (N,H,W,C) and as channels_last (N,C,H,W)."""
    yield t_nhwc, lambda o: o
    yield t_nhwc.permute(0, 3, 1, 2), lambda o: o.permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32", "bf16"])
@pytest.mark.parametrize("src,out,B,C,ks", R.CASES, ids=R.CASE_IDS)
def test_torch_path_equals_loop_oracle(src, out, B, C, ks, dtype):
    im, batches = R.case(src, out, B, C, ks)
    x = R.torch_images(im, dtype)
    aug = DeviceAugment.center(out)  # apply() takes the output size from the transform
    for idx, par, S in batches:
        want = R.expected(S, dtype)
        for xin, back in _layouts(x):
            got = back(aug.apply(xin, torch.tensor(idx), torch.tensor(par, dtype=torch.int32)))
            assert got.dtype == dtype and tuple(got.shape) == (B,) + tuple(out) + (C,)
            assert torch.equal(got, want)


def test_oracle_identity_flip_and_shift():
    """The oracle itself on the cases that have a closed form."""
    im = R.images_u8(2, 6, 5, 3)
    full = [R.box(0, 5), R.box(0, 6), 0]
    ident = R.to_u8(R.ref_sums(im, [1], [[0, 0, 65536, 65536, 0] + full], 6, 5))
    assert (ident[0] == im[1]).all()
    flipped = R.to_u8(R.ref_sums(im, [0], [[0, 0, 65536, 65536, 1] + full], 6, 5))
    assert (flipped[0] == im[0][:, ::-1]).all()
    sh = R.to_u8(R.ref_sums(im, [0], [[2 << 16, -(1 << 16), 65536, 65536, 2] + full], 6, 5))
    pad = np.pad(im[0], ((3, 3), (3, 3), (0, 0)))
    assert (sh[0] == pad[3 - 1: 3 - 1 + 6, 3 + 2: 3 + 2 + 5]).all()


# ------------------------------------------------------------------ against torch ops
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32", "bf16"])
@pytest.mark.parametrize("C", [1, 3])
def test_pad_crop_equals_pad_and_slice(dtype, C):
    N, H, W, P = 6, 9, 11, 3
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (N, C, H, W), generator=g).to(dtype)
    x = x.contiguous(memory_format=torch.channels_last)
    aug = DeviceAugment.pad_crop(P, flip=0.0, size=(H, W), seed=2)
    idx = torch.tensor([5, 0, 3, 3, 1, 2, 4, 0])
    par = aug.params(idx, 1)
    got = aug.apply(x, idx, par)
    assert tuple(got.shape) == (8, C, H, W)
    padded = F.pad(x, (P, P, P, P))
    for b in range(8):
        tx, ty = int(par[b, 0]) >> 16, int(par[b, 1]) >> 16
        want = padded[idx[b], :, P + ty: P + ty + H, P + tx: P + tx + W]
        assert torch.equal(got[b], want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32", "bf16"])
def test_flip_equals_torch_flip(dtype):
    N, H, W = 4, 7, 10
    x = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(2)).to(dtype)
    aug = DeviceAugment.pad_crop(0, flip=1.0, size=(H, W))
    idx = torch.tensor([3, 1, 1, 0])
    got = aug.apply(x, idx, aug.params(idx, 0))
    assert torch.equal(got, torch.flip(x[idx], dims=[2]))


def test_resized_crop_close_to_interpolate():
    """uint8 noise, 60 random boxes: within 3 grey levels of float64 bilinear interpolation
    of the crop (8-bit fractions cost at most 2 * 255/256, rounding 0.5, the DX floor drift
    at most OW / 65536 px)."""
    N, H, W, OH, OW = 4, 13, 11, 9, 8
    x = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(3),
                      dtype=torch.uint8)
    aug = DeviceAugment.random_resized_crop((OH, OW), size=(H, W), seed=4)
    keys = torch.arange(60)
    idx = keys % N
    par = aug.params(keys, 0)
    x0, y0, w, h = aug.boxes(keys, 0)
    got = aug.apply(x, idx, par).double()
    worst = 0.0
    for b in range(60):
        crop = x[idx[b], y0[b]: y0[b] + h[b], x0[b]: x0[b] + w[b]].permute(2, 0, 1)[None].double()
        want = F.interpolate(crop, size=(OH, OW), mode="bilinear", align_corners=False)
        worst = max(worst, float((got[b].permute(2, 0, 1) - want[0]).abs().max()))
    print("max |ours - interpolate| =", worst)
    assert worst <= 3.0


def test_apply_rejects_bad_layouts():
    aug = DeviceAugment.pad_crop(1, size=(8, 8))
    idx = torch.tensor([0])
    with pytest.raises(ValueError):
        aug.apply(torch.zeros(2, 3, 8, 8), idx, aug.params(idx, 0))  # NCHW, not channels_last
    with pytest.raises(ValueError):
        DeviceAugment("rrc")  # no output size
    with pytest.raises(ValueError):
        DeviceAugment.pad_crop(1).params(idx, 0)  # no source size


# ------------------------------------------------------------------ loader
def _dataset(n=48, C=1, H=12, W=10, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    im = torch.randint(0, 256, (n, C, H, W), generator=g).to(dtype)
    return TensorDataset(im.contiguous(memory_format=torch.channels_last), torch.arange(n))


def _epoch(loader, epoch):
    loader.set_epoch(epoch)
    return [(x.clone(), y.clone()) for x, y in loader]


def test_loader_epochs():
    ds = _dataset(C=3)
    aug = DeviceAugment.pad_crop(2, flip=0.5, seed=1)
    loader = DeviceLoader(ds, 16, shuffle=False, transform=aug)
    e0, e1, e0b = _epoch(loader, 0), _epoch(loader, 1), _epoch(loader, 0)
    assert len(e0) == 3 and tuple(e0[0][0].shape) == (16, 3, 12, 10)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(e0, e0b))
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(e0, e1))
    # iter_gathered yields the augmented tensor too (no Gathered object)
    loader.set_epoch(0)
    for (xg, yg), (x, y) in zip(loader.iter_gathered(), e0):
        assert isinstance(xg, torch.Tensor) and torch.equal(xg, x) and torch.equal(yg, y)


def test_loader_without_transform_is_unchanged():
    ds = _dataset()
    plain = DeviceLoader(ds, 16, shuffle=True, seed=3)
    assert plain.transform is None
    idx = plain._indices()
    for k, (x, y) in enumerate(plain):
        assert torch.equal(x, ds.images[idx[16 * k: 16 * k + 16]])
    assert plain.cursor().nbatch == 3


def test_same_pixels_on_any_rank():
    """A 2-way partition and the 1-rank run augment a dataset row identically."""
    ds = _dataset(n=50, C=3)
    aug = DeviceAugment.random_resized_crop((12, 10), flip=0.5, seed=7)

    def rows(ws, rank, bs):
        sampler = MySampler(ds, ws, rank, shuffle=True, seed=0, mode="partition")
        loader = DeviceLoader(ds, bs, sampler=sampler, transform=aug)
        loader.set_epoch(2)
        return {int(i): x[j].clone() for x, y in loader for j, i in enumerate(y)}

    one = rows(1, 0, 16)
    assert len(one) == 50
    seen = 0
    for rank in (0, 1):
        for i, img in rows(2, rank, 7).items():
            assert torch.equal(img, one[i])
            seen += 1
    assert seen >= 50


def test_cursor_raises_with_transform():
    loader = DeviceLoader(_dataset(), 16, transform=DeviceAugment.pad_crop(2))
    with pytest.raises(ValueError, match="transform"):
        loader.cursor()


def test_second_batch_leaves_the_first_alone():
    loader = DeviceLoader(_dataset(), 16, transform=DeviceAugment.pad_crop(2, seed=3))
    it = iter(loader)
    x0, _ = next(it)
    keep = x0.clone()
    x1, _ = next(it)
    assert x1.data_ptr() != x0.data_ptr() and torch.equal(x0, keep)


# ------------------------------------------------------------------ task3
def test_task3_augment_flag(tmp_path, monkeypatch):
    from dmlab.tasks import task3

    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    js = tmp_path / "aug.json"
    args = ["--device", "cpu", "--model", "lenet", "--synthetic", "--train-samples", "320",
            "--max-steps", "5", "--no-test"]
    stats = task3.main(args + ["--augment", "pad-crop", "--aug-seed", "3", "--json", str(js)])
    assert stats["steps"] == 5 and np.isfinite(stats["samples_per_s"])
    rec = json.loads(js.read_text())
    assert rec["augment"] == "pad-crop" and rec["aug_seed"] == 3 and rec["aug_flip"] == 0.0
    assert "fused" not in rec  # --fused auto resolved to the layer-wise loop
    with pytest.raises(SystemExit):
        task3.main(args + ["--augment", "pad-crop", "--fused", "1"])
    js2 = tmp_path / "plain.json"
    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    task3.main(args + ["--json", str(js2)])
    plain = json.loads(js2.read_text())
    assert not any(k.startswith("aug") for k in plain)
    assert set(rec) - set(plain) == {"augment", "aug_seed", "aug_flip"}


def test_task3_rrc_evaluates_on_the_centre_crop(monkeypatch):
    from dmlab.tasks import task3

    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    stats = task3.main(["--device", "cpu", "--model", "lenet", "--synthetic", "--train-samples",
                        "160", "--max-steps", "3", "--augment", "rrc", "--aug-scale", "0.5", "1",
                        "--aug-flip", "0.5"])
    assert stats["augment"] == "rrc" and stats["aug_flip"] == 0.5 and 0 <= stats["accuracy"] <= 1
