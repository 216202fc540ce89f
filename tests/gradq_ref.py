"""float64 numpy reference of the q8 gradient codec: the reference of the gradq tests.
Written from the codec's definition (blocks of 256 from the slice's start, s = a/127,
q = clamp(rint(e/s)), r = e - q*s, payload = scales + codes + padding); it shares no code
with dmlab and never calls the code under test.  Also the input generators and the property
checks that the CPU and the GPU tests both use."""
import numpy as np

B = 256


def n_blocks(n):
    return -(-n // B)


def payload_bytes(n):
    return -(-(4 * n_blocks(n) + n) // 16) * 16


def split_payload(payload, n):
    """uint8 array [..., payload_bytes(n)] -> (fp32 scales [..., nb], int8 codes [..., n])."""
    p = np.ascontiguousarray(np.asarray(payload, dtype=np.uint8))
    nb = n_blocks(n)
    assert p.shape[-1] == payload_bytes(n), (p.shape, payload_bytes(n))
    s = np.ascontiguousarray(p[..., :4 * nb]).view(np.float32)
    q = np.ascontiguousarray(p[..., 4 * nb:4 * nb + n]).view(np.int8)
    return s, q


def join_payload(s, q):
    """The inverse of split_payload for one rank (padding bytes zero)."""
    n = q.shape[-1]
    out = np.zeros(payload_bytes(n), np.uint8)
    out[:4 * n_blocks(n)] = np.asarray(s, np.float32).view(np.uint8)
    out[4 * n_blocks(n):4 * n_blocks(n) + n] = np.asarray(q, np.int8).view(np.uint8)
    return out


def _blocks(x):
    n = x.shape[0]
    xp = np.zeros(n_blocks(n) * B, x.dtype)
    xp[:n] = x
    return xp.reshape(-1, B)


def encode_ref(g, r=None):
    """g, r: fp32 arrays [n].  Returns a dict, everything beyond ``e`` in float64:
    e [n] fp32 (the one fp32 addition the definition asks for), a [nb], s [nb] = a/127
    (NaN for a non-finite block), x [n] = e/s (NaN where the block is dead), q [n] codes,
    r [n] = e - q*s (e where s == 0, 0 in a non-finite block), live [nb]."""
    g = np.asarray(g, np.float32)
    e = g if r is None else (g + np.asarray(r, np.float32)).astype(np.float32)
    n = e.shape[0]
    eb = _blocks(e.astype(np.float64))
    with np.errstate(all="ignore"):
        absb = np.abs(eb)
        a = np.where(np.isnan(absb).any(1), np.nan, absb.max(1))
        finite = np.isfinite(a)
        s = np.where(finite, a / 127.0, np.nan)
        s32 = s.astype(np.float32).astype(np.float64)  # what fp32 can hold of a/127
        live = finite & (s32 != 0)
        sd = np.where(live, s32, 1.0)[:, None]
        x = np.where(live[:, None], eb / sd, np.nan)
        q = np.where(live[:, None], np.clip(np.rint(eb / sd), -127, 127), 0.0)
        rn = np.where(live[:, None], eb - q * sd, np.where(finite[:, None], eb, 0.0))
    return dict(e=e, a=a, s=s, s32=s32, live=live, x=x.reshape(-1)[:n],
                q=q.reshape(-1)[:n], r=rn.reshape(-1)[:n])


def decode_mean_ref(scales, codes, c):
    """scales [ws, nb] fp32, codes [ws, n] int8 -> float64 c * sum over ranks of q*s."""
    scales = np.asarray(scales, np.float64)
    codes = np.asarray(codes, np.float64)
    n = codes.shape[1]
    with np.errstate(all="ignore"):
        return c * (codes * np.repeat(scales, B, axis=1)[:, :n]).sum(0)


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


# ------------------------------------------------------------------ inputs
def exact_ints(n, k, seed=0):
    """Every block: integers in [-127, 127] times 2^k with at least one +-127, so s == 2^k,
    the codes are the integers and the residual is exactly 0.  Returns (g fp32, ints)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-127, 128, size=n)
    for b0 in range(0, n, B):
        v[b0 + rng.integers(0, min(B, n - b0))] = 127 if (b0 // B) % 2 == 0 else -127
    return (v * 2.0 ** k).astype(np.float32), v


def half_ints(n, k, seed=0):
    """Every block: maximum 254 * 2^k (s == 2 * 2^k), every other entry an odd multiple of
    2^k below it, so every e/s is a half-integer: ties to even decide each code and the
    residual is exactly +-2^k (0 at the maximum).  Needs n >= 1.  Returns (g fp32, odd ints)."""
    rng = np.random.default_rng(seed)
    v = 2 * rng.integers(-126, 126, size=n) + 1  # odd, |v| <= 251
    for b0 in range(0, n, B):
        v[b0 + rng.integers(0, min(B, n - b0))] = 254 if (b0 // B) % 2 == 0 else -254
    return (v * 2.0 ** k).astype(np.float32), v


def half_int_codes(v):
    """Codes of half_ints: v/2 rounded half to even (+-127 at the maximum)."""
    return np.rint(v / 2.0).astype(np.int64)


def random_normal(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32)


# seeds at which at most 0.1 % of the elements lie within 2^-12 of a tie (tie_free below), with
# and without the residual: found with this reference alone, rechecked by
# test_gradq_cpu.py::test_tie_margin_share_of_the_seeds (normal data puts about 0.05 % there,
# so a short slice needs a seed with none)
SEEDS = {1: 0, 4: 0, 255: 1, 256: 1, 257: 1, 1027: 0, 300001: 0}


def random_pair(n):
    """(gradient, small carried residual) for the random-input checks at size n."""
    return random_normal(n, SEEDS[n]), (0.01 * random_normal(n, SEEDS[n] + 1)).astype(np.float32)


def tie_free(x):
    """Elements whose code is decided far enough from a tie for fp32 arithmetic to agree with
    float64: |x - round(x)| < 0.5 - 2^-12 (x = e/s in float64)."""
    return np.abs(x - np.rint(x)) < 0.5 - 2.0 ** -12


# ------------------------------------------------------------------ property checks
def check_encode_properties(g, r_old, s_got, q_got, r_new):
    """The derived bounds on an encode of ordinary (finite, normal-range) data:
    s within 1 ulp of fp32(a/127); |q| <= 127; |e - q*s| <= 0.5*s*(1 + 2^-10) with the scale
    and codes the implementation produced; |r_new - (e - q*s)| <= 2^-22 * a in float64 (one
    fp32 rounding of q*s, about 2^-24 a, plus one of the difference)."""
    ref = encode_ref(g, r_old)
    n = np.asarray(g).shape[0]
    s_got = np.asarray(s_got, np.float64)
    q_got = np.asarray(q_got, np.float64)
    assert (np.abs(s_got - ref["s32"]) <= ulp32(ref["s32"])).all()
    assert (np.abs(q_got) <= 127).all()
    se = np.repeat(s_got, B)[:n]
    ae = np.repeat(ref["a"], B)[:n]
    err = ref["e"].astype(np.float64) - q_got * se
    assert (np.abs(err) <= 0.5 * se * (1 + 2.0 ** -10)).all(), np.abs(err / se).max()
    if r_new is not None:
        d = np.abs(np.asarray(r_new, np.float64) - err)
        assert (d <= 2.0 ** -22 * ae).all(), (d / ae).max()
    return ref
