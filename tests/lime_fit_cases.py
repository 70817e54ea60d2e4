"""Cases, float64 reference and yardstick shared by test_gpu_lime_fit.py and
test_lime_fit_ref.py.

The reference is lasso_regression's coordinate descent (residual form, same
order and stopping rule) in float64 numpy with no float32 step.  The
yardstick of a case is how far the existing lasso_regression's coefficients
are from that reference: the noise users of the host fit already have.  It
is computed on the CPU from the reference side alone; lime_fit's
coefficients, intercepts and r2 each have to stay inside it, and its sweep
counts have to equal the reference's."""
import functools

import numpy as np
import torch

from mmlspark_amd.explainers.regression import lasso_regression
from mmlspark_amd.ops import backend

WIDTH = 0.75
# (n, m, C, alpha, {column: forced value}, rows)
CASES = [
    (64, 1, 1, 0.0, {}, 2),              # single coordinate
    (64, 5, 2, 0.0, {}, 2),              # sub-tile m, two classes, one Gram
    (200, 33, 3, 0.0, {}, 2),            # a bit past a word and two tiles
    (200, 33, 3, 0.01, {}, 2),           # the same with thresholding
    (65, 64, 1, 0.005, {3: 1, 40: 0}, 2),   # constant columns, max_iter cap
    (130, 128, 8, 0.0, {77: 0}, 1),      # LDS limit, a class per wave
    (96, 129, 1, 0.01, {}, 2),           # first shape with the Gram in global
    (512, 196, 2, 0.0, {}, 1),           # ImageLIME at cellSize 16
]


def reference(S, y, w, alpha, max_iter=200, tol=1e-6):
    w = w / w.sum()
    xm, ym = (S * w[:, None]).sum(0), (y * w).sum()
    Xc, resid = S - xm, y - ym
    xs = np.maximum(np.sqrt((Xc * Xc * w[:, None]).sum(0)), 1e-12)
    Xs = Xc / xs
    wX = w[:, None] * Xs
    z = np.maximum((wX * Xs).sum(0), 1e-12)
    var = (w * resid * resid).sum()
    beta, sweeps = np.zeros(S.shape[1]), 0
    for _ in range(max_iter):
        sweeps, max_delta = sweeps + 1, 0.0
        for j in range(S.shape[1]):
            bj = beta[j]
            rho = (wX[:, j] * (resid + Xs[:, j] * bj)).sum()
            bnew = np.sign(rho) * max(abs(rho) - alpha, 0.0) / z[j]
            if bnew != bj:
                resid = resid + Xs[:, j] * (bj - bnew)
                beta[j] = bnew
                max_delta = max(max_delta, abs(bnew - bj))
        if max_delta < tol:
            break
    coef = beta / xs
    return (coef, ym - (coef * xm).sum(),
            1.0 - (w * resid * resid).sum() / max(var, 1e-12), sweeps)


@functools.lru_cache(maxsize=None)
def case(idx):
    """(states (R, n, m), scores (R, n, C), reference outputs, yardstick)."""
    n, m, C, alpha, forced, R = CASES[idx]
    rng = np.random.default_rng(100 + idx)
    S = (rng.random((R, n, m)) < 0.5).astype(np.float64)
    for col, v in forced.items():
        S[:, :, col] = v
    B = rng.normal(size=(m, C)) * 2
    Y = S @ B + 0.3 * np.sin(S @ rng.normal(size=(m, C))) \
        + 0.05 * rng.normal(size=(R, n, C))
    coef, icpt = np.zeros((R, C, m)), np.zeros((R, C))
    r2, sweeps = np.zeros((R, C)), np.zeros((R, C), dtype=np.int32)
    yard = 0.0
    free = [j for j in range(m) if j not in forced]
    for r in range(R):
        d = np.sqrt((1.0 - S[r]).sum(1)) / np.sqrt(m)
        w = np.sqrt(np.exp(-(d / WIDTH) ** 2))
        for c in range(C):
            coef[r, c], icpt[r, c], r2[r, c], sweeps[r, c] = reference(
                S[r], Y[r, :, c], w, alpha)
        # the host fit is slow: its first class alone sets the yardstick,
        # which can only make the bound tighter
        host = lasso_regression(
            torch.from_numpy(S[r]), torch.from_numpy(Y[r, :, 0]), alpha,
            sample_weight=torch.from_numpy(w)).coefficients.numpy()
        yard = max(yard, np.abs(host - coef[r, 0])[free].max())
    return S, Y, (coef, icpt, r2, sweeps), yard


def max_yardstick():
    return max(case(i)[3] for i in range(len(CASES)))


def check(idx, device):
    """backend.lime_fit on `device` against case idx."""
    n, m, C, alpha, forced, R = CASES[idx]
    S, Y, (coef, icpt, r2, sweeps), yard = case(idx)
    bits = torch.stack([backend.pack_states(s) for s in S]).to(device)
    got = [t.cpu().numpy() for t in backend.lime_fit(
        bits, m, torch.from_numpy(Y).to(device), WIDTH, alpha)]
    devs = [np.abs(g - e).max() for g, e in zip(got, (coef, icpt, r2))]
    print("case", CASES[idx][:4], "yardstick %.3g" % yard,
          "coef %.3g intercept %.3g r2 %.3g" % tuple(devs),
          "sweeps", sweeps.ravel().tolist())
    assert yard > 0
    assert np.array_equal(got[3], sweeps)
    assert got[3].dtype == np.int32
    for col in forced:
        assert (got[0][:, :, col] == 0).all()
    assert max(devs) <= yard, (devs, yard)
