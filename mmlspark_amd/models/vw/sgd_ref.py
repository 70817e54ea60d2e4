"""Torch CPU reference for the VW sparse-SGD kernels (minibatch/hogwild
semantics matching vw_kernels.hip; numerics reference for GPU tests)."""
from __future__ import annotations

import torch

EPS = 1e-10


def _dloss(loss: str, pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    if loss == "squared":
        return pred - y
    if loss == "logistic":  # y in {-1, +1}
        return -y * torch.sigmoid(-y * pred)
    if loss == "hinge":
        return torch.where(y * pred < 1.0, -y, torch.zeros_like(y))
    raise ValueError(loss)


def vw_predict(indices, values, offsets, w_tbl):
    n_ex = offsets.numel() - 1
    counts = offsets[1:] - offsets[:-1]
    seg = torch.repeat_interleave(torch.arange(n_ex, device=indices.device),
                                  counts)
    contrib = w_tbl[indices.long()] * values
    out = torch.zeros(n_ex, dtype=torch.float32, device=indices.device)
    out.index_add_(0, seg, contrib)
    return out


def _invariant_dp(loss: str, pred, y, h_eta):
    """Prediction-space move of the importance-weight-invariant update
    (Karampatziakis & Langford, VW --invariant): integrate the per-example
    gradient flow dp/dh = -eta * dloss(p) exactly over importance weight h,
    so a weight-h update equals h sequential weight-1 updates in the small-h
    limit and NEVER overshoots the label/margin for any h."""
    if loss == "squared":  # p(h) = y + (p0-y) exp(-h eta)
        return (y - pred) * (-torch.expm1(-h_eta))
    if loss == "logistic":
        # q = y*p obeys e^q + q = e^{q0} + q0 + h*eta; solve d = q-q0 >= 0,
        # the root of g(d) = A expm1(d) + d - h_eta with A = e^{q0}.  g is
        # convex and increasing, so Newton started at or right of the root
        # descends onto it and never passes it.  Both h_eta (g = A expm1)
        # and log1p(h_eta/A) (g = d) are right of it; the smaller is within
        # a few Newton steps for every (q0, h_eta).
        q0 = y * pred
        A = torch.exp(q0)
        # where A underflows, log1p(h_eta/A) = log(h_eta) - q0
        start = torch.where(q0 > -40.0, torch.log1p(h_eta / A),
                            torch.log(h_eta) - q0)
        d = torch.minimum(h_eta, start.clamp_min(0.0))
        for _ in range(8):
            # A e^d as e^{q0+d} (<= A + h_eta: no overflow) and A expm1(d)
            # as that times (1 - e^{-d}): finite for every q0 and d
            E = torch.exp(q0 + d)
            g = E * (-torch.expm1(-d)) + d - h_eta
            d = (d - g / (E + 1.0)).clamp_min(0.0)
        # A >= e^30: the linear term is below float32 resolution
        return y * torch.where(q0 > 30.0, h_eta * torch.exp(-q0), d)
    if loss == "hinge":  # move to the margin, never past it
        q0 = y * pred
        d = torch.minimum(h_eta, (1.0 - q0).clamp_min(0.0))
        return y * d
    raise ValueError(loss)


def vw_sgd_minibatch(indices, values, offsets, labels, w_tbl, g_tbl, lr, l2,
                     power_t, loss: str, ex_weight=None, s_tbl=None,
                     invariant=False):
    """One pass over the minibatch: adaptive (AdaGrad) sparse updates.
    Collisions accumulate like the GPU kernel's atomics (index_add).
    invariant=True applies VW's importance-weight-aware closed-form update
    (safe for large importance weights).

    Like the kernel (and VW), an example whose update is zero leaves the
    tables alone, l2 decay included: on the plain path one whose weighted
    loss gradient is 0, on the invariant path one whose sensitivity is 0."""
    n_ex = offsets.numel() - 1
    counts = offsets[1:] - offsets[:-1]
    seg = torch.repeat_interleave(torch.arange(n_ex, device=indices.device),
                                  counts)
    il = indices.long()
    preds = vw_predict(indices, values, offsets, w_tbl)
    gl0 = _dloss(loss, preds, labels)
    gl = gl0 * ex_weight if ex_weight is not None else gl0
    g = gl[seg] * values + l2 * w_tbl[il]

    def normalized(scale):  # --normalized: divide by the running max|x|
        sn = s_tbl[il]
        return torch.where(sn > 0.0, scale / sn, scale)

    if invariant:
        if s_tbl is not None:
            s_tbl.scatter_reduce_(0, il, values.abs(), reduce="amax")
        # per-coordinate scale with G-before-update + x^2 proxy (VW's
        # pred_per_update sensitivity), then a prediction-space solve
        Gp = g_tbl[il] + values * values
        scale = torch.rsqrt(Gp + EPS) if power_t == 0.5 \
            else (Gp + EPS) ** (-power_t)
        if s_tbl is not None:
            scale = normalized(scale)
        xs2 = values * values * scale
        x_norm = torch.zeros(n_ex, dtype=torch.float32,
                             device=indices.device)
        x_norm.index_add_(0, seg, xs2)  # sensitivity sum x_i^2 s_i
        h = ex_weight if ex_weight is not None else torch.ones_like(labels)
        dp = _invariant_dp(loss, preds, labels, h * lr * x_norm)
        live = x_norm > 0.0
        k = torch.where(live, dp / x_norm, torch.zeros_like(dp))[seg]
        live = live[seg]
        zero = torch.zeros_like(g)
        g_tbl.index_add_(0, il, torch.where(live, g * g, zero))
        w_tbl.index_add_(0, il, torch.where(
            live, (k * values - lr * l2 * w_tbl[il]) * scale, zero))
        return preds
    live = (gl != 0.0)[seg]
    zero = torch.zeros_like(g)
    g = torch.where(live, g, zero)
    if s_tbl is not None:
        s_tbl.scatter_reduce_(0, il, torch.where(live, values.abs(), zero),
                              reduce="amax")
    g_tbl.index_add_(0, il, g * g)
    G = g_tbl[il]
    if power_t == 0.5:
        scale = torch.rsqrt(G + EPS)
    else:
        scale = (G + EPS) ** (-power_t)
    if s_tbl is not None:
        scale = normalized(scale)
    w_tbl.index_add_(0, il, -lr * g * scale)
    return preds
