"""References shared by test_loss_metrics_cpu.py and test_loss_metrics_gpu.py: the label-rank
rule of ``dmlab.nn.EvalMetrics`` written out in torch, float64 NLL, and planted labels."""
import torch
import torch.nn.functional as F

SHAPES = [(1, 10), (5, 10), (7, 63), (6, 65), (300, 1000)]

# Ranks planted per period of 8 rows: every rank 0..7 once, rank 0 again on every fourth row
# (in place of rank 4).  The order inside the period is chosen so that already the first five
# rows hold both hits and misses at k = 1 and at k = 5.
_PERIOD = (0, 5, 1, 6, 0, 7, 2, 3)


def ref_rank(x, y):
    """rank = #{c : x_c > x_y} + #{c < y : x_c == x_y}, on the logit values as stored."""
    xf = x.float()
    xy = xf.gather(1, y[:, None])
    cols = torch.arange(xf.shape[1], device=xf.device)[None, :]
    return ((xf > xy) | ((xf == xy) & (cols < y[:, None]))).sum(1)


def ref_counts(x, y, k):
    """(n, top-1 hits, top-k hits) by the rank rule."""
    r = ref_rank(x, y)
    return [x.shape[0], int((r < 1).sum()), int((r < k).sum())]


def ref_nll_sum(x, y):
    return F.cross_entropy(x.double(), y, reduction="sum")


def planted_labels(x, shift=0, mult=1):
    """Row i's label is the column at position ``mult * _PERIOD[(i + shift) % 8]`` of the row's
    stable descending order, i.e. the column whose rank under the rule is that position."""
    B, C = x.shape
    order = x.float().argsort(dim=1, descending=True, stable=True)
    i = torch.arange(B, device=x.device)
    pos = torch.tensor(_PERIOD, device=x.device)[(i + shift) % 8] * mult
    assert int(pos.max()) < C
    return order[i, pos]


def assert_mixed(x, y, k):
    """The reference itself has at least a quarter of the rows hitting and a quarter missing
    at k: a kernel that reports all-hit or all-miss cannot pass."""
    B = x.shape[0]
    hits = int((ref_rank(x, y) < k).sum())
    assert 4 * hits >= B and 4 * (B - hits) >= B, (B, k, hits)
