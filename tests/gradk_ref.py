"""numpy reference of the topk gradient codec: the reference of the gradk tests.  Written from
the codec's definition (blocks of 2048 from the slice's start, key = |e| as an integer, the K
largest keys with ties in ascending index, emitted in ascending index, payload = values +
uint16 indices + padding, decode in rank order); it shares no code with dmlab and never calls
the code under test.  Also the input generators that the CPU and the GPU tests both use."""
import numpy as np

B = 2048
UNUSED = 0xFFFF


def n_blocks(n):
    return -(-n // B)


def payload_bytes(n, keep):
    return -(-(6 * n_blocks(n) * keep) // 16) * 16


def split_payload(payload, n, keep):
    """uint8 array [..., payload_bytes(n, keep)] -> (fp32 values [..., nb, keep], uint16
    indices [..., nb, keep])."""
    p = np.ascontiguousarray(np.asarray(payload, dtype=np.uint8))
    nb = n_blocks(n)
    assert p.shape[-1] == payload_bytes(n, keep), (p.shape, payload_bytes(n, keep))
    v = np.ascontiguousarray(p[..., :4 * nb * keep]).view(np.float32)
    i = np.ascontiguousarray(p[..., 4 * nb * keep:6 * nb * keep]).view(np.uint16)
    return v.reshape(p.shape[:-1] + (nb, keep)), i.reshape(p.shape[:-1] + (nb, keep))


def join_payload(vals, idx, n, fill=0):
    """The inverse of split_payload for one rank; the padding bytes are ``fill``."""
    vals = np.ascontiguousarray(vals, np.float32)
    idx = np.ascontiguousarray(idx, np.uint16)
    nb, keep = vals.shape
    assert nb == n_blocks(n)
    out = np.full(payload_bytes(n, keep), fill, np.uint8)
    out[:4 * nb * keep] = vals.reshape(-1).view(np.uint8)
    out[4 * nb * keep:6 * nb * keep] = idx.reshape(-1).view(np.uint8)
    return out


def keys_of(e):
    return np.ascontiguousarray(e, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def encode_ref(g, r, keep):
    """g, r (or None): fp32 arrays [n].  Returns (values [nb, keep] fp32, indices [nb, keep]
    uint16, new residual [n] fp32 or None)."""
    g = np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        e = g.copy() if r is None else (g + np.asarray(r, np.float32)).astype(np.float32)
    n = e.shape[0]
    nb = n_blocks(n)
    vals = np.zeros((nb, keep), np.float32)
    idx = np.full((nb, keep), UNUSED, np.uint16)
    rn = e.copy()
    for b in range(nb):
        eb = e[b * B:(b + 1) * B]
        m = eb.shape[0]
        k = keys_of(eb).astype(np.int64)
        # primary: key descending; secondary: index ascending (lexsort: the last key is primary)
        order = np.lexsort((np.arange(m), -k))
        sel = np.sort(order[:min(keep, m)])
        vals[b, :sel.size] = eb[sel]
        idx[b, :sel.size] = sel
        rn[b * B + sel] = 0.0
    return vals, idx, (None if r is None else rn)


def decode_mean_ref(vals, idx, n, c):
    """vals [ws, nb, keep] fp32, idx [ws, nb, keep] uint16 -> float64 c * sum over ranks."""
    vals = np.asarray(vals, np.float64)
    ws, nb, keep = vals.shape
    acc = np.zeros(nb * B)
    with np.errstate(all="ignore"):
        for rk in range(ws):
            for b in range(nb):
                used = idx[rk, b] != UNUSED
                np.add.at(acc, b * B + idx[rk, b][used].astype(np.int64), vals[rk, b][used])
        return c * acc[:n]


# ------------------------------------------------------------------ inputs
def random_normal(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32)


def random_pair(n, seed=0):
    """(gradient, small carried residual)."""
    return random_normal(n, seed), (0.01 * random_normal(n, seed + 1)).astype(np.float32)


def small_ints(n, k, seed=0, lo=-50, hi=51):
    """Integers in [lo, hi) times 2^k: sums of a few of them are exact in fp32."""
    rng = np.random.default_rng(seed)
    v = rng.integers(lo, hi, size=n)
    return (v * 2.0 ** k).astype(np.float32), v


def special_blocks():
    """Six blocks and a 5-element tail, one property each.  Returns (g, description dict)."""
    n = 6 * B + 5
    g = random_normal(n, seed=9)
    rng = np.random.default_rng(10)
    # block 0: equal magnitudes, mixed signs
    g[0:B] = 0.75 * np.where(rng.integers(0, 2, B) == 0, -1.0, 1.0)
    # block 1: three non-zeros, zeros of both signs elsewhere
    g[B:2 * B] = 0.0
    g[B + 1::2][:B // 2] = -0.0
    g[B + 700], g[B + 5], g[B + 2047] = -3.5, 1e-30, 2.0
    # block 2: a NaN and an Inf among ordinary data
    g[2 * B + 100] = np.nan
    g[2 * B + 1900] = -np.inf
    # block 3: denormals only
    g[3 * B:4 * B] = np.float32(1e-44) * np.where(g[3 * B:4 * B] < 0, -1, 1).astype(np.float32)
    g[3 * B + 77] = np.float32(3e-44)
    # blocks 4, 5: ordinary; the tail block has m = 5
    return g, dict(n=n, ties=0, zeros=1, nonfinite=2, denormal=3, tail=6)
