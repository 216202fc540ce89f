"""The q8 codec's HIP kernels (csrc/gradq.hip) against the float64 reference
(tests/gradq_ref.py) and against the torch path of dmlab.parallel.compress: every shape on a
16-byte aligned slice and on a view one element into its storage, with and without the
residual, with sentinel bytes behind every output."""
import numpy as np
import pytest
import torch

import gradq_ref as R

pytestmark = pytest.mark.gpu
SIZES = [1, 4, 255, 256, 257, 1027, 300001]
GUARD = 64


def _lib():
    from dmlab.ops._native import lib

    return lib()


def _dev_view(x, mis, dev, guard_value):
    """x (numpy fp32) as a device view: 16-B aligned, or starting one element (4 B) into its
    storage; GUARD sentinel elements follow it.  Returns (view, whole storage)."""
    n = x.shape[0]
    store = torch.full((n + 4 + GUARD,), guard_value, dtype=torch.float32, device=dev)
    off = 1 if mis else 0
    view = store[off:off + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert (view.data_ptr() % 16 == 0) == (not mis)
    return view, store


def kernel_encode(g, r, mis, dev, max_blocks=0):
    """Run q8_encode; returns (scales, codes, payload bytes, new residual or None) as numpy,
    after checking that nothing behind the payload, the residual or the gradient changed."""
    n = g.shape[0]
    pb = R.payload_bytes(n)
    gv, gstore = _dev_view(g, mis, dev, 9.0)
    g_before = gstore.clone()
    rv = rstore = None
    if r is not None:
        rv, rstore = _dev_view(r, mis, dev, 5.0)
    pstore = torch.full((pb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    _lib().q8_encode(gv, rv, pstore[:pb], max_blocks)
    torch.cuda.synchronize()
    # the gradient is read only (compared as bits: it may hold NaN)
    assert torch.equal(gstore.view(torch.int32), g_before.view(torch.int32))
    used = 4 * R.n_blocks(n) + n
    assert (pstore[used:] == 0xA5).all()  # padding and the guard behind the payload
    r_new = None
    if r is not None:
        off = 1 if mis else 0
        assert (rstore[:off] == 5.0).all() and (rstore[off + n:] == 5.0).all()
        r_new = rv.cpu().numpy()
    payload = pstore[:pb].cpu().numpy()
    s, q = R.split_payload(payload, n)
    return s, q, payload, r_new


def torch_encode(g, r):
    from dmlab.parallel.compress import encode_torch

    n = g.shape[0]
    payload = torch.full((R.payload_bytes(n),), 0xA5, dtype=torch.uint8)
    rt = None if r is None else torch.from_numpy(r.copy())
    encode_torch(torch.from_numpy(g.copy()), rt, payload)
    s, q = R.split_payload(payload.numpy(), n)
    return s, q, payload.numpy(), (None if rt is None else rt.numpy())


def _same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()


cases = pytest.mark.parametrize("n", SIZES)
align = pytest.mark.parametrize("mis", [False, True], ids=["aligned", "offset4"])
resid = pytest.mark.parametrize("ef", [True, False], ids=["ef", "noef"])


def test_bindings_present_and_checked(dev):
    lib = _lib()
    assert lib.q8_payload_bytes(51902) == R.payload_bytes(51902)
    g = torch.zeros(300, device=dev)
    with pytest.raises(RuntimeError, match="payload"):
        lib.q8_encode(g, None, torch.zeros(R.payload_bytes(300) + 16, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="float32"):
        lib.q8_encode(g.double(), None,
                      torch.zeros(R.payload_bytes(300), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="residual"):
        lib.q8_encode(g, torch.zeros(299, device=dev),
                      torch.zeros(R.payload_bytes(300), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="payload_bytes"):
        lib.q8_decode_mean(torch.zeros((2, 64), dtype=torch.uint8, device=dev), g, 1.0)


@cases
@align
@resid
def test_exact_integer_blocks(n, mis, ef, dev):
    for k in (-20, 0, 7):
        g, ints = R.exact_ints(n, k, seed=n)
        r0 = np.zeros(n, np.float32) if ef else None
        s, q, payload, r = kernel_encode(g, r0, mis, dev)
        assert (s == np.float32(2.0 ** k)).all() and (q == ints).all()
        if ef:
            assert (r == 0).all()
        assert _same_bits(payload, torch_encode(g, r0)[2])  # the torch path, bit for bit


@cases
@align
def test_half_integer_blocks_round_to_even(n, mis, dev):
    for k in (-20, 0, 7):
        g, odd = R.half_ints(n, k, seed=n)
        r0 = np.zeros(n, np.float32)
        s, q, payload, r = kernel_encode(g, r0, mis, dev)
        want = R.half_int_codes(odd)
        assert (s == np.float32(2.0 * 2.0 ** k)).all() and (q == want).all()
        assert (r.astype(np.float64) == (odd - 2 * want) * 2.0 ** k).all()
        ts, tq, tp, tr = torch_encode(g, r0)
        assert _same_bits(payload, tp) and _same_bits(r, tr)


@cases
@align
@resid
def test_random_normal_properties_and_torch_path(n, mis, ef, dev):
    g, r0 = R.random_pair(n)
    r0 = r0 if ef else None
    for max_blocks in ((0, 8) if n >= 1027 else (0,)):  # 8 workgroups: several grid passes
        s, q, _, r = kernel_encode(g, r0, mis, dev, max_blocks)
        ref = R.check_encode_properties(g, r0, s, q, r)
        ts, tq, _, tr = torch_encode(g, r0)
        assert _same_bits(s, ts)
        keep = R.tie_free(ref["x"])
        left_out = 1.0 - keep.mean()
        print(f"n={n} left out of the code comparison: {left_out:.5%}; codes differing from "
              f"the torch path anywhere: {(q != tq).sum()}")
        assert left_out <= 1e-3
        assert (q[keep] == tq[keep]).all() and (q[keep] == ref["q"][keep]).all()


@align
def test_special_blocks(mis, dev):
    n = 6 * 256 + 10
    g = R.random_normal(n, seed=9)
    g[0:512] = 0.0
    g[300] = -3.5
    g[512:768] = np.float32(1e-44) * np.where(g[512:768] < 0, -1, 1).astype(np.float32)
    g[800] = np.inf
    g[1100] = np.nan
    r0 = np.zeros(n, np.float32)
    r0[1024:1280] = 0.25
    s, q, payload, r = kernel_encode(g, r0, mis, dev)
    assert s[0] == 0 and (q[:256] == 0).all() and (r[:256] == 0).all()
    assert s[1] == np.float32(3.5) / np.float32(127) and q[300] == -127
    assert (np.delete(q[256:512], 44) == 0).all()
    assert s[2] == 0 and (q[512:768] == 0).all() and _same_bits(r[512:768], g[512:768])
    for b in (3, 4):
        assert np.isnan(s[b]) and (q[b * 256:(b + 1) * 256] == 0).all()
        assert (r[b * 256:(b + 1) * 256] == 0).all()
    R.check_encode_properties(g[1280:], r0[1280:], s[5:], q[1280:], r[1280:])
    ts, tq, _, tr = torch_encode(g, r0)
    assert (tq == q).all() and _same_bits(np.nan_to_num(s), np.nan_to_num(ts)) and _same_bits(r, tr)
    out = kernel_decode(np.stack([payload, payload]), n, 0.5, mis, dev)
    assert np.isnan(out[768:1280]).all() and np.isfinite(out[:768]).all()
    assert np.isfinite(out[1280:]).all()


# ------------------------------------------------------------------ decode-mean
def kernel_decode(rows, n, c, mis, dev, max_blocks=0):
    gathered = torch.full((rows.shape[0] * rows.shape[1] + GUARD,), 0x5A, dtype=torch.uint8,
                          device=dev)
    gv = gathered[:rows.size].view(rows.shape[0], rows.shape[1])
    gv.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
    before = gathered.clone()
    out, store = _dev_view(np.full(n, 7.0, np.float32), mis, dev, 3.0)
    _lib().q8_decode_mean(gv, out, c, max_blocks)
    torch.cuda.synchronize()
    off = 1 if mis else 0
    assert (store[:off] == 3.0).all() and (store[off + n:] == 3.0).all()  # guard behind out
    assert torch.equal(gathered, before)
    return out.cpu().numpy()


_rows_cache = {}


def _rows(n, ws, kind):
    """ws payloads of n elements, encoded once on the CPU and shared by the decode cases."""
    key = (n, kind)
    if key not in _rows_cache:
        rows, total = [], np.zeros(n)
        for rk in range(8):
            if kind == "ints":
                g, ints = R.exact_ints(n, rk - 3, seed=10 + rk)
                total = total + ints * 2.0 ** (rk - 3)
                rows.append((torch_encode(g, None)[2], total.copy()))
            else:
                rows.append((torch_encode(R.random_normal(n, 20 + rk) * (1 + rk), None)[2], None))
        _rows_cache[key] = rows
    rows = _rows_cache[key][:ws]
    return np.stack([p for p, _ in rows]), rows[-1][1]


@pytest.mark.parametrize("ws", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [257, 300001])
@align
def test_decode_mean(n, ws, mis, dev):
    from dmlab.parallel.compress import decode_mean_torch

    ints, total = _rows(n, ws, "ints")
    rand, _ = _rows(n, ws, "rand")
    s, q = R.split_payload(rand, n)
    for c in (1.0, 1.0 / ws):
        c32 = np.float64(np.float32(c))
        # exact inputs: sums of small integers times powers of two, then one fp32 rounding
        assert (kernel_decode(ints, n, c, mis, dev) == (total * c32).astype(np.float32)).all()
        for max_blocks in ((0, 8) if n > 1000 else (0,)):
            got = kernel_decode(rand, n, c, mis, dev, max_blocks)
            want = R.decode_mean_ref(s, q, c32)
            assert np.abs(got - want).max() <= ws * 2.0 ** -23 * np.abs(want).max()
            cpu = torch.empty(n)
            decode_mean_torch(torch.from_numpy(rand), cpu, c)
            assert _same_bits(got, cpu.numpy())  # the torch path adds in the same order


def test_compressor_on_device_matches_cpu(dev):
    """Q8Compressor on the GPU (kernels) and on the CPU (torch path) over three steps of one
    bucket inside a larger buffer: payloads, residuals and decoded gradients bit for bit."""
    from dmlab.parallel.compress import Q8Compressor, payload_bytes

    total, lo, n = 4096, 1280, 1027
    comps = [Q8Compressor(total, d) for d in (dev, "cpu")]
    for t in range(3):
        g = R.random_normal(n, seed=50 + t)
        outs = []
        for comp in comps:
            d = comp.device
            payload = torch.zeros(payload_bytes(n), dtype=torch.uint8, device=d)
            out = torch.zeros(n, device=d)
            comp.encode(torch.from_numpy(g).to(d), lo, payload)
            comp.decode_mean(payload.view(1, -1), out, 1.0)
            outs.append((payload.cpu(), out.cpu(), comp.residual.cpu()))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
    assert comps[0].residual[:lo].abs().max() == 0 and comps[0].residual[lo + n:].abs().max() == 0
