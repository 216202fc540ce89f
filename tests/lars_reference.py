"""float64 per-tensor LARS loop: the reference of the LARS tests.  Written from the
formulas of the optimiser's definition; it never calls the code under test."""
import math

import torch


def lars_ref_step(ws, gs, bs, adapted, *, lr, eta=0.001, wd=0.0, mu=0.9, eps=1e-9,
                  grad_scale=1.0, nesterov=False, max_grad_norm=None):
    """One step from the given state (any dtype/device; computed on the CPU in float64).
    Returns (new_w, new_b, stats [n,3] = (|w|, |g'|, r), G)."""
    ws = [w.detach().double().cpu().reshape(-1) for w in ws]
    gs = [g.detach().double().cpu().reshape(-1) for g in gs]
    bs = [b.detach().double().cpu().reshape(-1) for b in bs]
    G = math.sqrt(sum(float((grad_scale * g).square().sum()) for g in gs))
    c = 1.0 if max_grad_norm is None else min(1.0, max_grad_norm / (G + 1e-6))
    new_w, new_b, stats = [], [], []
    for w, g, b, ad in zip(ws, gs, bs, adapted):
        gp = c * grad_scale * g
        wn, gn = float(w.norm()), float(gp.norm())
        r = 1.0
        if ad:
            if wn > 0 and gn > 0:
                r = eta * wn / (gn + wd * wn + eps)
            d = r * (gp + wd * w)
        else:
            d = gp
        b2 = mu * b + d
        w2 = w - lr * (d + mu * b2 if nesterov else b2)
        new_w.append(w2)
        new_b.append(b2)
        stats.append((wn, gn, r))
    return new_w, new_b, torch.tensor(stats, dtype=torch.float64).reshape(-1, 3), G


def rel_l2(a, ref):
    """|a - ref| / |ref| in float64 (0 when both are zero)."""
    a, ref = a.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    den = float(ref.norm())
    num = float((a - ref).norm())
    return num / den if den > 0 else num
