"""The augmentation kernel (csrc/augment.hip) against the per-pixel loop oracle
(augment_ref.py), its guards, graph capture, and the loader / ResNet-18 level."""
import pytest
import torch

import augment_ref as R
from dmlab.data import DeviceAugment, DeviceLoader, TensorDataset
from dmlab.ops._native import lib

pytestmark = pytest.mark.gpu

DTYPES = [torch.uint8, torch.float32, torch.bfloat16]
IDS = ["u8", "f32", "bf16"]


def _par(rows, dev):
    return torch.tensor(rows, dtype=torch.int32, device=dev)


def _run(x, idx, par, out_hw):
    """The native kernel on an (N,H,W,C) device tensor -> (B,OH,OW,C)."""
    out = torch.empty((idx.numel(),) + tuple(out_hw) + (x.shape[3],), device=x.device,
                      dtype=x.dtype)
    lib().augment_apply(x, idx, par, out)
    return out


# ------------------------------------------------------------------ kernel vs the loop oracle
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("src,out,B,C,ks", R.CASES, ids=R.CASE_IDS)
def test_kernel_equals_loop_oracle(dev, src, out, B, C, ks, dtype):
    """Bit-equal: uint8 always; fp32 / bf16 on integer-valued pixels, where every product
    and sum is exact (255 * 65536 < 2^24)."""
    im, batches = R.case(src, out, B, C, ks)
    x = R.torch_images(im, dtype, dev)
    for idx, par, S in batches:
        got = _run(x, torch.tensor(idx, device=dev), _par(par, dev), out).cpu()
        want = R.expected(S, dtype)
        bad = (got.float() != want.float()).sum().item()
        print(f"idx {idx}: {bad} of {got.numel()} values differ")
        assert torch.equal(got, want)
    # the channels_last (N,C,H,W) view of the same memory is accepted as it is
    idx, par, S = batches[0]
    out_t = torch.empty((B, C) + tuple(out), device=dev, dtype=dtype).contiguous(
        memory_format=torch.channels_last)
    lib().augment_apply(x.permute(0, 3, 1, 2), torch.tensor(idx, device=dev), _par(par, dev), out_t)
    assert torch.equal(out_t.permute(0, 2, 3, 1).cpu(), R.expected(S, dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 3])
def test_real_valued_noise(dev, dtype, C):
    """Within 8 * 2^-24 * max|tap| of a float64 evaluation of the same weights; bf16 storage
    adds 2^-8 * |value|.  (The weights are integers <= 2^16, exact in fp32; the four products
    and the three sums are each below 2^16 * max|tap| and rounded once, the 2^-16 scale is
    exact: at most 7 * 2^-24 * max|tap|.)"""
    (N, H, W), (OH, OW) = (3, 13, 11), (17, 19)
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(N, H, W, C, generator=g) * 3).to(dtype)
    rows = [r for _, r in R.planted(H, W, OH, OW)]
    idx = [(N - 1 - k) % N for k in range(len(rows))]
    S, M = R.ref_sums(x.double().numpy(), idx, rows, OH, OW, tapmax=True)
    want = torch.from_numpy(R.to_real(S))
    got = _run(x.to(dev), torch.tensor(idx, device=dev), _par(rows, dev), (OH, OW)).cpu().double()
    tol = 8 * 2.0 ** -24 * torch.from_numpy(M)
    if dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * want.abs()
    err = (got - want).abs()
    print(f"max err {err.max().item():.3e}, max err / tol {(err / tol.clamp_min(1e-30)).max():.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (1, 1, 2), (2, 1, 1)])
def test_smallest_tensors(dev, dtype, N, H, W):
    """3-channel taps are 4-element loads: the tap that ends the tensor, and a tensor too small
    for one such load (a single 1 x 1 image)."""
    im = R.images_u8(N, H, W, 3, seed=5)
    x = R.torch_images(im, dtype, dev)
    rows = [R.resize_row(0, 0, W, H, 2, 3), R.resize_row(W - 1, 0, 1, 1, 2, 3, flags=1)]
    idx = [N - 1, N - 1]
    # H = 1: handed over as the channels_last (N,3,H,W) view, the reading that wins when a
    # shape fits both layouts
    got = torch.empty(2, 2, 3, 3, device=dev, dtype=dtype)
    lib().augment_apply(x.permute(0, 3, 1, 2), torch.tensor(idx, device=dev), _par(rows, dev), got)
    assert torch.equal(got.cpu(), R.expected(R.ref_sums(im, idx, rows, 2, 3), dtype))


# ------------------------------------------------------------------ guards
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_idx_outside_the_dataset_gives_zero_rows(dev, dtype):
    N, H, W, C = 3, 13, 11, 3
    im = R.images_u8(N, H, W, C, seed=3)
    x = R.torch_images(im, dtype, dev)
    rows = [r for _, r in R.planted(H, W, H, W)][:5]
    idx = [2, -1, 0, N, 1]
    got = _run(x, torch.tensor(idx, device=dev), _par(rows, dev), (H, W)).cpu()
    S = R.ref_sums(im, idx, rows, H, W)
    assert not S[1].any() and not S[3].any() and S[0].any() and S[2].any() and S[4].any()
    assert torch.equal(got, R.expected(S, dtype))
    huge = [2, -(1 << 62), 0, (1 << 62), 1]
    got = _run(x, torch.tensor(huge, device=dev), _par(rows, dev), (H, W)).cpu()
    assert torch.equal(got, R.expected(S, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("offset", [0, 16, 5])
def test_out_view_inside_a_larger_buffer(dev, dtype, offset):
    """``out`` as a view (16-byte aligned or not): the bytes before and after it stay."""
    N, H, W, C, B = 3, 13, 11, 3, 5
    im = R.images_u8(N, H, W, C, seed=4)
    x = R.torch_images(im, dtype, dev)
    rows = [r for _, r in R.planted(H, W, H, W)][4:4 + B]
    idx = [2, 2, 1, 0, 0]
    n = B * H * W * C
    pad = 64
    buf = torch.full((pad + offset + n + pad,), 77, device=dev, dtype=dtype)
    out = buf[pad + offset: pad + offset + n].view(B, H, W, C)
    lib().augment_apply(x, torch.tensor(idx, device=dev), _par(rows, dev), out)
    host = buf.cpu()
    assert bool((host[: pad + offset] == 77).all()) and bool((host[pad + offset + n:] == 77).all())
    want = R.expected(R.ref_sums(im, idx, rows, H, W), dtype)
    assert torch.equal(host[pad + offset: pad + offset + n].view(B, H, W, C), want)


def test_binding_checks(dev):
    x = torch.zeros(3, 8, 8, 3, device=dev, dtype=torch.uint8)
    idx = torch.zeros(2, device=dev, dtype=torch.long)
    par = torch.zeros(2, 8, device=dev, dtype=torch.int32)
    out = torch.empty(2, 8, 8, 3, device=dev, dtype=torch.uint8)
    f = lib().augment_apply
    f(x, idx, par, out)
    with pytest.raises(RuntimeError):
        f(x, idx, par, out.float())                       # dtype of out
    with pytest.raises(RuntimeError):
        f(x.to(torch.int16), idx, par, out)               # dtype of images
    with pytest.raises(RuntimeError):
        f(x, idx.int(), par, out)                         # idx int64
    with pytest.raises(RuntimeError):
        f(x, idx, par[:, :7].contiguous(), out)           # params [B,8]
    with pytest.raises(RuntimeError):
        f(x, idx, par.long(), out)                        # params int32
    with pytest.raises(RuntimeError):
        f(x, idx, par, out[:1])                           # batch of out
    with pytest.raises(RuntimeError):
        f(x, idx, par, torch.empty(2, 8, 8, 1, device=dev, dtype=torch.uint8))  # channels
    with pytest.raises(RuntimeError):
        f(x.permute(0, 2, 1, 3), idx, par, out)           # strided images
    with pytest.raises(RuntimeError):
        f(x, idx, par, x[:2])                             # out aliases images
    with pytest.raises(RuntimeError):
        f(x.cpu(), idx, par, out)                         # host tensor
    with pytest.raises(RuntimeError):
        f(torch.zeros(3, 8, 8, 2, device=dev, dtype=torch.uint8), idx, par,
          torch.empty(2, 8, 8, 2, device=dev, dtype=torch.uint8))              # C = 2
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_runs_bit_equal_and_graph_replay(dev, dtype):
    """Two eager runs agree, and a captured launch replayed on two different idx / params
    inputs equals eager (no host sync, no allocation inside the call)."""
    from dmlab.utils.graph import CapturedStep

    N, H, W, C, B, OH, OW = 6, 20, 24, 3, 5, 16, 18
    g = torch.Generator().manual_seed(6)
    x = torch.randint(0, 256, (N, H, W, C), generator=g).to(dtype).to(dev)
    aug = DeviceAugment.random_resized_crop((OH, OW), flip=0.5, size=(H, W), seed=8)
    idx_a, idx_b = torch.tensor([5, 3, 3, 1, 0]), torch.tensor([0, 4, 2, 2, 5])
    par_a, par_b = aug.params(idx_a, 0), aug.params(idx_b, 1)
    assert not torch.equal(par_a, par_b)
    out = torch.empty(B, OH, OW, C, device=dev, dtype=dtype)

    def step(idx, par):
        lib().augment_apply(x, idx, par, out)
        return out

    eager = {}
    for name, (i, p) in {"a": (idx_a, par_a), "b": (idx_b, par_b)}.items():
        first = _run(x, i.to(dev), p.to(dev), (OH, OW))
        again = _run(x, i.to(dev), p.to(dev), (OH, OW))
        assert torch.equal(first, again)
        eager[name] = first
    assert not torch.equal(eager["a"], eager["b"])
    runner = CapturedStep(step, [idx_a.to(dev), par_a.to(dev)], warmup=1)
    assert torch.equal(runner(idx_b.to(dev), par_b.to(dev)), eager["b"])
    assert torch.equal(runner(idx_a.to(dev), par_a.to(dev)), eager["a"])
    assert runner.replays == 2


# ------------------------------------------------------------------ loader and model
@pytest.mark.parametrize("mode", ["pad_crop", "rrc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_loader_on_gpu_equals_cpu_path(dev, dtype, mode):
    n, C, H, W = 40, 3, 20, 18
    g = torch.Generator().manual_seed(9)
    im = torch.randint(0, 256, (n, C, H, W), generator=g).to(dtype).contiguous(
        memory_format=torch.channels_last)
    ds = TensorDataset(im, torch.arange(n))
    aug = (DeviceAugment.pad_crop(3, flip=0.5, seed=2) if mode == "pad_crop"
           else DeviceAugment.random_resized_crop((16, 14), flip=0.5, seed=2))
    host = DeviceLoader(ds, 16, shuffle=True, seed=1, transform=aug)
    gpu = DeviceLoader(ds.to(dev), 16, shuffle=True, seed=1, transform=aug)
    for epoch in (0, 1):
        host.set_epoch(epoch)
        gpu.set_epoch(epoch)
        nb = 0
        for (xh, yh), (xg, yg) in zip(host, gpu):
            assert xg.is_cuda and xg.shape == xh.shape
            assert torch.equal(xg.cpu(), xh) and torch.equal(yg.cpu(), yh)
            nb += 1
        assert nb == 3


def test_resnet18_step_through_the_loader(dev):
    """One ResNet-18 training step at batch 8 on 64 x 64 uint8 through the rrc loader: the
    fused stem takes the augmented batch, the loss is finite and every gradient equals the one
    from feeding a clone of the same augmented batch as a plain tensor."""
    import copy

    from dmlab.models import ResNet18
    from dmlab.nn import cross_entropy
    from dmlab.ops.stem import stem_fused_ok

    n, side = 32, 64
    g = torch.Generator().manual_seed(12)
    im = torch.randint(0, 256, (n, 3, side, side), generator=g, dtype=torch.uint8).contiguous(
        memory_format=torch.channels_last)
    ds = TensorDataset(im, torch.randint(0, 10, (n,), generator=g)).to(dev)
    aug = DeviceAugment.random_resized_crop(side, flip=0.5, seed=5)
    loader = DeviceLoader(ds, 8, shuffle=True, seed=3, transform=aug)
    torch.manual_seed(0)
    model = ResNet18(num_classes=10).to(dev)
    twin = copy.deepcopy(model)
    x, y = next(iter(loader))
    assert x.dtype == torch.uint8 and tuple(x.shape) == (8, 3, side, side)
    assert stem_fused_ok(model.stem, x)
    plain = x.clone()
    loss = cross_entropy(model(x), y)
    loss.backward()
    loss2 = cross_entropy(twin(plain), y)
    loss2.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and torch.equal(loss, loss2)
    grads = 0
    for (name, p), q in zip(model.named_parameters(), twin.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert torch.equal(p.grad, q.grad), name
        grads += 1
    assert grads > 20
