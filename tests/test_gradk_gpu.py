"""The topk codec's HIP kernels (csrc/gradk.hip) against the numpy reference
(tests/gradk_ref.py) and against the torch path of dmlab.parallel.compress, bit for bit: every
shape on a 16-byte aligned slice and on a view one element into its storage, with and without
the residual, with sentinel bytes behind every output.  Selection is on integer keys with a
defined tie order, so nothing is left out of any comparison."""
import numpy as np
import pytest
import torch

import gradk_ref as R

pytestmark = pytest.mark.gpu
SIZES = [1, 33, 2047, 2048, 2049, 3 * 2048 + 5, 300001]
KEEPS = [1, 32, 256]
GUARD = 64
FILL = 0xA5


def _lib():
    from dmlab.ops._native import lib

    return lib()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and (_bits(a) == _bits(b)).all()


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


def kernel_encode(g, r, keep, mis, dev, max_blocks=0):
    """Run topk_encode; returns (payload bytes, new residual or None) as numpy, after checking
    that nothing behind the payload, the residual or the gradient changed."""
    n = g.shape[0]
    pb = R.payload_bytes(n, keep)
    gv, gstore = _dev_view(g, mis, dev, 9.0)
    g_before = gstore.clone()
    rv = rstore = None
    if r is not None:
        rv, rstore = _dev_view(r, mis, dev, 5.0)
    pstore = torch.full((pb + GUARD,), FILL, dtype=torch.uint8, device=dev)
    _lib().topk_encode(gv, rv, pstore[:pb], keep, max_blocks)
    torch.cuda.synchronize()
    # the gradient is read only (compared as bits: it may hold NaN)
    assert torch.equal(gstore.view(torch.int32), g_before.view(torch.int32))
    used = 6 * R.n_blocks(n) * keep
    assert (pstore[used:] == FILL).all()  # padding and the guard behind the payload
    r_new = None
    if r is not None:
        off = 1 if mis else 0
        assert (rstore[:off] == 5.0).all() and (rstore[off + n:] == 5.0).all()
        r_new = rv.cpu().numpy()
    return pstore[:pb].cpu().numpy(), r_new


def torch_encode(g, r, keep):
    from dmlab.parallel.compress import topk_encode_torch

    n = g.shape[0]
    payload = torch.full((R.payload_bytes(n, keep),), FILL, dtype=torch.uint8)
    rt = None if r is None else torch.from_numpy(r.copy())
    topk_encode_torch(torch.from_numpy(g.copy()), rt, payload, keep)
    return payload.numpy(), (None if rt is None else rt.numpy())


_want_cache = {}


def want_encode(g, r, keep, key):
    """The reference and the torch mirror (checked equal), computed once per case and shared by
    the alignments and grid caps."""
    if key not in _want_cache:
        vals, idx, rn = R.encode_ref(g, r, keep)
        p = R.join_payload(vals, idx, g.shape[0], FILL)
        tp, tr = torch_encode(g, r, keep)
        assert _same_bits(p, tp) and (r is None or _same_bits(rn, tr))
        _want_cache[key] = (p, rn)
    return _want_cache[key]


align = pytest.mark.parametrize("mis", [False, True], ids=["aligned", "offset4"])
resid = pytest.mark.parametrize("ef", [True, False], ids=["ef", "noef"])


def test_bindings_present_and_checked(dev):
    lib = _lib()
    assert lib.topk_payload_bytes(51902, 32) == R.payload_bytes(51902, 32)
    g = torch.zeros(3000, device=dev)
    pb = R.payload_bytes(3000, 32)
    ok = torch.zeros(pb, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="payload"):
        lib.topk_encode(g, None, torch.zeros(pb + 16, dtype=torch.uint8, device=dev), 32)
    with pytest.raises(RuntimeError, match="float32"):
        lib.topk_encode(g.double(), None, ok, 32)
    with pytest.raises(RuntimeError, match="uint8"):
        lib.topk_encode(g, None, torch.zeros(pb, dtype=torch.int8, device=dev), 32)
    with pytest.raises(RuntimeError, match="residual"):
        lib.topk_encode(g, torch.zeros(2999, device=dev), ok, 32)
    for keep in (0, 257):
        with pytest.raises(RuntimeError, match="keep"):
            lib.topk_encode(g, None, ok, keep)
        with pytest.raises(RuntimeError, match="keep"):
            lib.topk_decode_mean(ok.view(1, -1), g, keep, 1.0)
        with pytest.raises(RuntimeError, match="keep"):
            lib.topk_payload_bytes(3000, keep)
    with pytest.raises(RuntimeError, match="payload_bytes"):
        lib.topk_decode_mean(torch.zeros((2, 64), dtype=torch.uint8, device=dev), g, 32, 1.0)
    with pytest.raises(RuntimeError, match="float32"):
        lib.topk_decode_mean(ok.view(1, -1), g.double(), 32, 1.0)
    with pytest.raises(RuntimeError):
        lib.topk_encode(g.cpu(), None, ok, 32)


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("n", SIZES)
@align
@resid
def test_encode_equals_reference_and_torch_path(n, keep, mis, ef, dev):
    g, r0 = R.random_pair(n, seed=n + keep)
    r0 = r0 if ef else None
    want_p, want_r = want_encode(g, r0, keep, (n, keep, ef))
    for max_blocks in ((0, 8) if n > 100000 else (0,)):  # 8 workgroups: several grid passes
        p, r = kernel_encode(g, r0, keep, mis, dev, max_blocks)
        assert _same_bits(p, want_p)  # values, indices, untouched padding
        if ef:
            assert _same_bits(r, want_r)


@pytest.mark.parametrize("keep", KEEPS)
@align
def test_special_blocks(keep, mis, dev):
    """Ties with mixed signs, fewer than K non-zeros, NaN and Inf, denormals, m < K."""
    g, d = R.special_blocks()
    n = d["n"]
    r0 = np.zeros(n, np.float32)
    want_p, want_r = want_encode(g, r0, keep, ("special", keep))
    p, r = kernel_encode(g, r0, keep, mis, dev)
    assert _same_bits(p, want_p) and _same_bits(r, want_r)
    vals, idx = R.split_payload(p, n, keep)
    assert (idx[d["ties"]] == np.arange(keep)).all()
    sent = idx[d["nonfinite"]].tolist()
    assert 100 in sent and (keep == 1 or 1900 in sent)
    assert 77 in idx[d["denormal"]].tolist()
    k5 = min(keep, 5)
    assert (idx[d["tail"]][k5:] == R.UNUSED).all() and (_bits(vals[d["tail"]][k5:]) == 0).all()
    nz = [5, 700, 2047]  # the non-zeros, then the lowest-index zeros; K = 1: the largest
    want = sorted((nz + [i for i in range(R.B) if i not in nz])[:keep]) if keep >= 3 else [700]
    assert idx[d["zeros"]].tolist() == want
    # without the residual: the same payload from e = g (-0.0 stays -0.0)
    want_p2, _ = want_encode(g, None, keep, ("special-noef", keep))
    p2, _ = kernel_encode(g, None, keep, mis, dev)
    assert _same_bits(p2, want_p2)
    out = kernel_decode(np.stack([p, p]), n, keep, 0.5, mis, dev)
    assert np.isnan(out[2 * R.B + 100]) and np.isfinite(out[:2 * R.B]).all()


# ------------------------------------------------------------------ decode-mean
def kernel_decode(rows, n, keep, c, mis, dev, max_blocks=0):
    gathered = torch.full((rows.shape[0] * rows.shape[1] + GUARD,), 0x5A, dtype=torch.uint8,
                          device=dev)
    gv = gathered[:rows.size].view(rows.shape[0], rows.shape[1])
    gv.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
    before = gathered.clone()
    out, store = _dev_view(np.full(n, 7.0, np.float32), mis, dev, 3.0)
    _lib().topk_decode_mean(gv, out, keep, c, max_blocks)
    torch.cuda.synchronize()
    off = 1 if mis else 0
    assert (store[:off] == 3.0).all() and (store[off + n:] == 3.0).all()  # guard behind out
    assert torch.equal(gathered, before)
    return out.cpu().numpy()


_rows_cache = {}


def _rows(n, ws, keep, kind):
    """ws payloads of n elements, encoded once on the CPU and shared by the decode cases; for
    the integer rows also the exact running sum of what each rank sends."""
    key = (n, keep, kind)
    if key not in _rows_cache:
        rows, total = [], np.zeros(n)
        for rk in range(8):
            if kind == "ints":
                g, _ = R.small_ints(n, rk - 3, seed=10 + rk)
                vals, idx, _ = R.encode_ref(g, None, keep)
                sent = np.zeros(n)
                for b in range(R.n_blocks(n)):
                    used = idx[b] != R.UNUSED
                    sent[b * R.B + idx[b][used].astype(np.int64)] = vals[b][used]
                total = total + sent
                rows.append((R.join_payload(vals, idx, n), total.copy()))
            else:
                vals, idx, _ = R.encode_ref(R.random_normal(n, 20 + rk) * (1 + rk), None, keep)
                rows.append((R.join_payload(vals, idx, n), None))
        _rows_cache[key] = rows
    rows = _rows_cache[key][:ws]
    return np.stack([p for p, _ in rows]), rows[-1][1]


@pytest.mark.parametrize("ws", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [2049, 300001])
@align
def test_decode_mean(n, ws, mis, dev):
    from dmlab.parallel.compress import topk_decode_mean_torch

    keep = 32
    ints, total = _rows(n, ws, keep, "ints")
    rand, _ = _rows(n, ws, keep, "rand")
    v, i = R.split_payload(rand, n, keep)
    for c in (1.0, 1.0 / ws):
        c32 = np.float64(np.float32(c))
        # exact inputs: sums of small integers times powers of two, then one fp32 rounding
        got = kernel_decode(ints, n, keep, c, mis, dev)
        assert (got == (total * c32).astype(np.float32)).all()
        for max_blocks in ((0, 8) if n > 100000 else (0,)):
            got = kernel_decode(rand, n, keep, c, mis, dev, max_blocks)
            want = R.decode_mean_ref(v, i, n, c32)
            assert np.abs(got - want).max() <= ws * 2.0 ** -23 * np.abs(want).max()
            cpu = torch.empty(n)
            topk_decode_mean_torch(torch.from_numpy(rand), cpu, c, keep)
            assert _same_bits(got, cpu.numpy())  # the torch path adds in the same order


@pytest.mark.parametrize("keep", [1, 256])
def test_decode_mean_other_keeps_and_unused_slots(keep, dev):
    """K = 1 and K = 256 (every thread of the workgroup adds), with a 5-element last block whose
    unused slots must be skipped."""
    n, ws = 2 * 2048 + 5, 3
    rows = np.stack([R.join_payload(*R.encode_ref(R.random_normal(n, 40 + rk), None, keep)[:2], n)
                     for rk in range(ws)])
    v, i = R.split_payload(rows, n, keep)
    want = R.decode_mean_ref(v, i, n, 1.0)
    for mis in (False, True):
        got = kernel_decode(rows, n, keep, 1.0, mis, dev)
        assert np.abs(got - want).max() <= ws * 2.0 ** -23 * np.abs(want).max()
        assert (got[want == 0] == 0).all()


@align
def test_decode_order_is_rank_order(mis, dev):
    """Three ranks list one element with 2^24, 1, -2^24: rank order gives 0 in fp32, not 1."""
    n, keep = 2049, 1
    rows = []
    for val in (2.0 ** 24, 1.0, -2.0 ** 24):
        g = np.zeros(n, np.float32)
        g[1234] = val
        g[2048] = val
        rows.append(R.join_payload(*R.encode_ref(g, None, keep)[:2], n))
    out = kernel_decode(np.stack(rows), n, keep, 1.0, mis, dev)
    assert (out == 0).all()
    out = kernel_decode(np.stack([rows[0], rows[2], rows[1]]), n, keep, 1.0, mis, dev)
    assert out[1234] == 1.0 and out[2048] == 1.0


def test_compressor_on_device_matches_cpu(dev):
    """TopKCompressor on the GPU (kernels) and on the CPU (torch path) over three steps of one
    bucket inside a larger buffer: payloads, residuals and decoded gradients bit for bit."""
    from dmlab.parallel.compress import TopKCompressor

    total, lo, n = 3 * 4096, 1280, 2 * 2048 + 1027
    comps = [TopKCompressor(total, d, keep=32) for d in (dev, "cpu")]
    for t in range(3):
        g = R.random_normal(n, seed=50 + t)
        outs = []
        for comp in comps:
            d = comp.device
            payload = torch.zeros(comp.payload_bytes(n), dtype=torch.uint8, device=d)
            out = torch.zeros(n, device=d)
            comp.encode(torch.from_numpy(g).to(d), lo, payload)
            comp.decode_mean(payload.view(1, -1), out, 1.0)
            outs.append((payload.cpu(), out.cpu(), comp.residual.cpu()))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
    assert comps[0].residual[:lo].abs().max() == 0 and comps[0].residual[lo + n:].abs().max() == 0
    assert comps[0].residual.abs().max() > 0
