"""The mixing augmentation kernel (csrc/augment_mix.hip) against the loop oracle (mix_ref.py)
and the unmixed kernel, its guards and graph capture; the mixed-target cross-entropy kernel
(csrc/loss.hip) against a float64 reference; the loader and one ResNet-18 step."""
import numpy as np
import pytest
import torch

import augment_ref as R
import mix_ref as MR
from dmlab.data import DeviceAugment, DeviceLoader, DeviceMix, TensorDataset
from dmlab.nn import MixTarget, cross_entropy
from dmlab.ops._native import lib
from loss_metrics_ref import SHAPES as LOSS_SHAPES

pytestmark = pytest.mark.gpu

DTYPES = [torch.uint8, torch.float32, torch.bfloat16]
IDS = ["u8", "f32", "bf16"]


def _i32(rows, dev):
    return torch.tensor(rows, dtype=torch.int32, device=dev)


def _run(x, idx, par, mix, out_hw):
    """The native kernel on an (N,H,W,C) device tensor -> (B,OH,OW,C)."""
    out = torch.empty((idx.numel(),) + tuple(out_hw) + (x.shape[3],), device=x.device,
                      dtype=x.dtype)
    lib().augment_mix_apply(x, idx, par, mix, out)
    return out


def _plain(x, idx, par, out_hw):
    out = torch.empty((idx.numel(),) + tuple(out_hw) + (x.shape[3],), device=x.device,
                      dtype=x.dtype)
    lib().augment_apply(x, idx, par, out)
    return out


# ------------------------------------------------------------------ kernel vs the loop oracle
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("src,out,B,C", MR.CASES, ids=MR.CASE_IDS)
def test_kernel_equals_loop_oracle(dev, src, out, B, C, dtype):
    """Bit-equal on integer-valued pixels: there every fp32 product and sum of a sample's blend
    is exact (255 * 65536 < 2^24), and the oracle evaluates the mix in numpy float32, one
    rounded operation at a time."""
    im, batches = MR.case(src, out, B, C)
    x = R.torch_images(im, dtype, dev)
    for idx, par, mix, S in batches:
        got = _run(x, torch.tensor(idx, device=dev), _i32(par, dev), _i32(mix, dev), out).cpu()
        want = MR.expected(S, mix, dtype)
        bad = (got.float() != want.float()).sum().item()
        print(f"idx {idx} mix {mix}: {bad} of {got.numel()} values differ")
        assert torch.equal(got, want)
    # the channels_last (N,C,H,W) view of the same memory is accepted as it is
    idx, par, mix, S = batches[-1]
    out_t = torch.empty((B, C) + tuple(out), device=dev, dtype=dtype).contiguous(
        memory_format=torch.channels_last)
    lib().augment_mix_apply(x.permute(0, 3, 1, 2), torch.tensor(idx, device=dev), _i32(par, dev),
                            _i32(mix, dev), out_t)
    assert torch.equal(out_t.permute(0, 2, 3, 1).cpu(), MR.expected(S, mix, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [1, 3])
def test_unmixed_table_equals_the_augmentation_kernel(dev, dtype, C):
    (N, H, W), (OH, OW) = (3, 13, 11), (17, 19)
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(N, H, W, C, generator=g) * 40 + 128).clamp(0, 255).to(dtype).to(dev)
    rows = [r for _, r in R.planted(H, W, OH, OW)]
    B = len(rows)
    idx = torch.tensor([(N - 1 - k) % N for k in range(B)], device=dev)
    mix = _i32([MR.unmixed_row(b) for b in range(B)], dev)
    got = _run(x, idx, _i32(rows, dev), mix, (OH, OW))
    assert torch.equal(got, _plain(x, idx, _i32(rows, dev), (OH, OW)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 3])
def test_real_valued_noise(dev, dtype, C):
    """Within 10 * 2^-24 * max|tap| of a float64 evaluation; bf16 storage adds 2^-8 * |value|.
    With u = 2^-24 and M the largest |tap| of either sample: each sample's unrounded blend a',
    p' is within 7 u M of its exact value (the augmentation test's bound); the weights L and
    65536 - L are integers <= 2^16, exact in fp32, and sum to 2^16, so the inherited error of
    L a' + (65536 - L) p' is at most 7 u M * 2^16; the two products are each rounded once, by
    at most u L M and u (65536 - L) M, together u M * 2^16; their sum is below 2^16 M and
    rounded once, u M * 2^16; the 2^-16 scale is exact.  9 u M in all, 10 with the second-order
    terms."""
    (N, H, W), (OH, OW) = (3, 13, 11), (17, 19)
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(N, H, W, C, generator=g) * 3).to(dtype)
    rows = [r for _, r in R.planted(H, W, OH, OW)]
    B = len(rows)
    idx = [(N - 1 - k) % N for k in range(B)]
    mix = MR.mix_rows(OH, OW, B, 0)
    S, M = R.ref_sums(x.double().numpy(), idx, rows, OH, OW, tapmax=True)
    want, tap = (torch.from_numpy(v) for v in MR.expected_real(S, M, mix))
    got = _run(x.to(dev), torch.tensor(idx, device=dev), _i32(rows, dev), _i32(mix, dev),
               (OH, OW)).cpu().double()
    tol = 10 * 2.0 ** -24 * tap
    if dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * want.abs()
    err = (got - want).abs()
    print(f"max err {err.max().item():.3e}, max err / tol {(err / tol.clamp_min(1e-30)).max():.3f}")
    assert bool((err <= tol).all())


# ------------------------------------------------------------------ guards
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cutmix_does_not_read_the_partner_outside_the_box(dev, dtype):
    """A partner sample of NaNs with L = 65536: outside the box the output is the augmentation
    kernel's, and finite; inside the box it is the partner's NaN."""
    N, H, W, C, OH, OW = 2, 13, 11, 3, 12, 10
    x = R.torch_images(R.images_u8(N, H, W, C, seed=8), dtype, dev)
    x[1] = float("nan")
    rows = [R.resize_row(1, 1, W - 2, H - 3, OH, OW), R.resize_row(0, 0, W, H, OH, OW, flags=1)]
    idx = torch.tensor([0, 1], device=dev)
    mix = _i32([[1, MR.ONE, MR.box(2, 5), MR.box(3, 7)], MR.unmixed_row(1)], dev)
    got = _run(x, idx, _i32(rows, dev), mix, (OH, OW))
    plain = _plain(x, idx, _i32(rows, dev), (OH, OW))
    inbox = torch.zeros(OH, OW, dtype=torch.bool, device=dev)
    inbox[3:8, 2:6] = True
    assert bool(torch.isfinite(got[0][~inbox]).all())
    assert torch.equal(got[0][~inbox], plain[0][~inbox])
    assert bool(torch.isnan(got[0][inbox]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_partner_idx_outside_the_dataset_contributes_zeros(dev, dtype):
    N, H, W, C = 3, 13, 11, 3
    im = R.images_u8(N, H, W, C, seed=3)
    x = R.torch_images(im, dtype, dev)
    rows = [r for _, r in R.planted(H, W, H, W)][:5]
    idx = [2, -1, 0, N, 1]
    mix = [[4 - b, 32768, MR.box(0, 3), MR.box(0, 2)] for b in range(5)]
    S = R.ref_sums(im, idx, rows, H, W)
    assert not S[1].any() and not S[3].any()
    for use in (idx, [2, -(1 << 62), 0, (1 << 62), 1]):
        got = _run(x, torch.tensor(use, device=dev), _i32(rows, dev), _i32(mix, dev), (H, W))
        assert torch.equal(got.cpu(), MR.expected(S, mix, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("offset", [0, 16, 5])
def test_out_view_inside_a_larger_buffer(dev, dtype, offset):
    """``out`` as a view (16-byte aligned or not): the bytes before and after it stay."""
    N, H, W, C, B = 3, 13, 11, 3, 5
    im = R.images_u8(N, H, W, C, seed=4)
    x = R.torch_images(im, dtype, dev)
    rows = [r for _, r in R.planted(H, W, H, W)][4:4 + B]
    idx = [2, 2, 1, 0, 0]
    mix = MR.mix_rows(H, W, B, 2)  # box_and_blend, two bad partners, two clamped L
    n = B * H * W * C
    pad = 64
    buf = torch.full((pad + offset + n + pad,), 77, device=dev, dtype=dtype)
    out = buf[pad + offset: pad + offset + n].view(B, H, W, C)
    lib().augment_mix_apply(x, torch.tensor(idx, device=dev), _i32(rows, dev), _i32(mix, dev), out)
    host = buf.cpu()
    assert bool((host[: pad + offset] == 77).all()) and bool((host[pad + offset + n:] == 77).all())
    want = MR.expected(R.ref_sums(im, idx, rows, H, W), mix, dtype)
    assert torch.equal(host[pad + offset: pad + offset + n].view(B, H, W, C), want)


def test_binding_checks(dev):
    x = torch.zeros(3, 8, 8, 3, device=dev, dtype=torch.uint8)
    idx = torch.zeros(2, device=dev, dtype=torch.long)
    par = torch.zeros(2, 8, device=dev, dtype=torch.int32)
    mix = _i32([MR.unmixed_row(0), MR.unmixed_row(1)], dev)
    out = torch.empty(2, 8, 8, 3, device=dev, dtype=torch.uint8)
    f = lib().augment_mix_apply
    f(x, idx, par, mix, out)
    with pytest.raises(RuntimeError):
        f(x, idx, par, mix, out.float())                       # dtype of out
    with pytest.raises(RuntimeError):
        f(x.to(torch.int16), idx, par, mix, out)               # dtype of images
    with pytest.raises(RuntimeError):
        f(x, idx.int(), par, mix, out)                         # idx int64
    with pytest.raises(RuntimeError):
        f(x, idx, par[:, :7].contiguous(), mix, out)           # params [B,8]
    with pytest.raises(RuntimeError):
        f(x, idx, par, mix.long(), out)                        # mix int32
    with pytest.raises(RuntimeError):
        f(x, idx, par, mix[:, :3].contiguous(), out)           # mix [B,4]
    with pytest.raises(RuntimeError):
        f(x, idx, par, mix[:1], out)                           # batch of mix
    with pytest.raises(RuntimeError):
        f(x, idx, par, torch.cat([mix, mix], 1)[:, :4], out)   # strided mix
    with pytest.raises(RuntimeError):
        f(x, idx, par, mix.cpu(), out)                         # host mix
    with pytest.raises(RuntimeError):
        f(x, idx, par, mix, out[:1])                           # batch of out
    with pytest.raises(RuntimeError):
        f(x.permute(0, 2, 1, 3), idx, par, mix, out)           # strided images
    with pytest.raises(RuntimeError):
        f(x, idx, par, mix, x[:2])                             # out aliases images
    with pytest.raises(RuntimeError):
        f(x.cpu(), idx, par, mix, out)                         # host tensor
    ce = lib().cross_entropy_mix
    lg = torch.zeros(2, 10, device=dev)
    y = torch.zeros(2, device=dev, dtype=torch.long)
    lam = torch.ones(2, device=dev)
    rl, ls, dl = torch.empty(2, device=dev), torch.empty((), device=dev), torch.empty_like(lg)
    ce(lg, y, y, lam, rl, ls, dl, 0.5, 0.0)
    with pytest.raises(RuntimeError):
        ce(lg, y, y.int(), lam, rl, ls, dl, 0.5, 0.0)          # labels int64
    with pytest.raises(RuntimeError):
        ce(lg, y, y[:1], lam, rl, ls, dl, 0.5, 0.0)            # one label per row
    with pytest.raises(RuntimeError):
        ce(lg, y, y, lam.double(), rl, ls, dl, 0.5, 0.0)       # lam float32
    with pytest.raises(RuntimeError):
        ce(lg, y, y, lam.cpu(), rl, ls, dl, 0.5, 0.0)          # host lam
    with pytest.raises(RuntimeError):
        ce(lg, y, y, lam, rl, ls, dl, 0.5, 1.5)                # eps
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_graph_replay_with_two_tables(dev, dtype):
    """One captured launch replayed on two different idx / params / mix inputs equals eager."""
    from dmlab.utils.graph import CapturedStep

    N, H, W, C, B, OH, OW = 6, 20, 24, 3, 5, 16, 18
    g = torch.Generator().manual_seed(6)
    x = torch.randint(0, 256, (N, H, W, C), generator=g).to(dtype).to(dev)
    aug = DeviceAugment.random_resized_crop((OH, OW), flip=0.5, size=(H, W), seed=8)
    mixer = DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, seed=8)
    idx_a, idx_b = torch.tensor([5, 3, 3, 1, 0]), torch.tensor([0, 4, 2, 2, 5])
    ins = {"a": (idx_a, aug.params(idx_a, 0), mixer.params(idx_a, 0, (OH, OW))[0]),
           "b": (idx_b, aug.params(idx_b, 1), mixer.params(idx_b, 1, (OH, OW))[0])}
    assert not torch.equal(ins["a"][2], ins["b"][2])
    ins = {k: tuple(t.to(dev) for t in v) for k, v in ins.items()}
    out = torch.empty(B, OH, OW, C, device=dev, dtype=dtype)

    def step(idx, par, mix):
        lib().augment_mix_apply(x, idx, par, mix, out)
        return out

    eager = {k: _run(x, *v, (OH, OW)) for k, v in ins.items()}
    assert not torch.equal(eager["a"], eager["b"])
    runner = CapturedStep(step, list(ins["a"]), warmup=1)
    assert torch.equal(runner(*ins["b"]), eager["b"])
    assert torch.equal(runner(*ins["a"]), eager["a"])
    assert runner.replays == 2


# ------------------------------------------------------------------ the loss kernel
def _logits(dev, B, C, dtype, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed + 1000 * B + C)
    return (torch.randn(B, C, device=dev, generator=g) * 3).to(dtype)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,C", LOSS_SHAPES)
def test_mixed_cross_entropy_kernel(dev, dtype, B, C, eps):
    """Against float64 F.cross_entropy on the explicit probability targets, with the
    smoothed-loss test's tolerances; lam = 1 agrees with the one-label loss."""
    x = _logits(dev, B, C, dtype, seed=3).requires_grad_(True)
    ya, yb, lam = MR.mixed_ce_rows(B, C, device=dev)
    l1 = cross_entropy(x, MixTarget(ya, yb, lam), label_smoothing=eps)
    l1.backward(torch.tensor(2.0, device=dev))
    xr = x.detach().double().requires_grad_(True)
    l2 = MR.mixed_ce_reference(xr, ya, yb, lam, eps)
    (2 * l2).backward()
    print(f"loss {l1.item():.7f} ref {l2.item():.7f} "
          f"max grad err {(x.grad.double() - xr.grad).abs().max().item():.3e}")
    torch.testing.assert_close(l1, l2.float(), rtol=1e-4, atol=1e-4)
    tol = 1e-6 if dtype == torch.float32 else 2e-3
    torch.testing.assert_close(x.grad.float(), xr.grad.float(), rtol=tol, atol=tol)
    if B >= 5:
        assert not x.grad[2:5].any()  # an invalid label in either slot: zero gradient
    # lam = 1: the one-label loss of ya
    yv = ya.clamp(0, C - 1)
    xa, xb = (x.detach().clone().requires_grad_(True) for _ in range(2))
    la = cross_entropy(xa, MixTarget(yv, yb.clamp(0, C - 1), torch.ones(B, device=dev)), eps)
    lb = cross_entropy(xb, yv, eps)
    la.backward()
    lb.backward()
    print(f"lam = 1 bit-equal to the one-label kernel: loss {torch.equal(la, lb)}, "
          f"gradient {torch.equal(xa.grad, xb.grad)}")
    torch.testing.assert_close(la, lb, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(xa.grad.float(), xb.grad.float(), rtol=tol, atol=tol)


# ------------------------------------------------------------------ loader and model
@pytest.mark.parametrize("mode", ["pad_crop", "rrc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_loader_on_gpu_equals_cpu_path(dev, dtype, mode):
    n, C, H, W = 40, 3, 20, 18
    g = torch.Generator().manual_seed(9)
    im = torch.randint(0, 256, (n, C, H, W), generator=g).to(dtype).contiguous(
        memory_format=torch.channels_last)
    ds = TensorDataset(im, torch.arange(n) % 7)
    aug = (DeviceAugment.pad_crop(3, flip=0.5, seed=2) if mode == "pad_crop"
           else DeviceAugment.random_resized_crop((16, 14), flip=0.5, seed=2))
    mix = DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.9, seed=4)
    host = DeviceLoader(ds, 16, shuffle=True, seed=1, transform=aug, mix=mix)
    gpu = DeviceLoader(ds.to(dev), 16, shuffle=True, seed=1, transform=aug, mix=mix)
    kinds = np.zeros(3, int)
    for epoch in (0, 1):
        host.set_epoch(epoch)
        gpu.set_epoch(epoch)
        tab = host._host_tables()[2]
        kinds += [int((tab[:, 1] < 65536).sum()), int((tab[:, 2] != MR.EMPTY).sum()),
                  int(((tab[:, 1] == 65536) & (tab[:, 2] == MR.EMPTY)).sum())]
        nb = 0
        for (xh, th), (xg, tg) in zip(host, gpu):
            assert xg.is_cuda and xg.shape == xh.shape
            assert torch.equal(xg.cpu(), xh)
            for fh, fg in zip(th, tg):
                assert fg.is_cuda and fg.dtype == fh.dtype and torch.equal(fg.cpu(), fh)
            nb += 1
        assert nb == 3
    assert (kinds > 0).all(), kinds  # mixup, CutMix and unmixed rows all went through


def test_resnet18_step_through_the_mixing_loader(dev):
    """One ResNet-18 training step at batch 8 on 64 x 64 uint8 through the mixing loader: the
    loss is finite and every gradient equals the one from a clone of the same batch and
    target."""
    import copy

    from dmlab.models import ResNet18

    n, side = 32, 64
    g = torch.Generator().manual_seed(12)
    im = torch.randint(0, 256, (n, 3, side, side), generator=g, dtype=torch.uint8).contiguous(
        memory_format=torch.channels_last)
    ds = TensorDataset(im, torch.randint(0, 10, (n,), generator=g)).to(dev)
    aug = DeviceAugment.random_resized_crop(side, flip=0.5, seed=5)
    loader = DeviceLoader(ds, 8, shuffle=True, seed=3, transform=aug,
                          mix=DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, seed=5))
    torch.manual_seed(0)
    model = ResNet18(num_classes=10).to(dev)
    twin = copy.deepcopy(model)
    x, t = next(iter(loader))
    assert x.dtype == torch.uint8 and tuple(x.shape) == (8, 3, side, side)
    assert isinstance(t, MixTarget) and bool((t.lam < 1).any())
    loss = cross_entropy(model(x), t, 0.1)
    loss.backward()
    loss2 = cross_entropy(twin(x.clone()), MixTarget(*(f.clone() for f in t)), 0.1)
    loss2.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and torch.equal(loss, loss2)
    grads = 0
    for (name, p), q in zip(model.named_parameters(), twin.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert torch.equal(p.grad, q.grad), name
        grads += 1
    assert grads > 20
