"""vw_sgd_k / vw_predict_k on MI355X against the float64 per-example oracle
of vw_kernel_cases: the full configuration grid, the zero-update rules, the
launch shapes, the logistic --invariant solve in isolation and a colliding
batch whose result is order-independent by construction."""
import numpy as np
import pytest
import torch

from . import vw_kernel_cases as cases
from .test_vw_oracle import _torch_batch, check_case

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")


def _backend():
    from mmlspark_amd.ops import backend
    return backend.vw_sgd_minibatch, backend.vw_predict


def _check(case):
    check_case(case, *_backend(), cases.GPU_MARGIN[case.family], "cuda")


@requires_gpu
@pytest.mark.parametrize("params", cases.GRID_PARAMS, ids=cases.grid_id)
def test_kernel_matches_oracle_on_grid(params):
    _check(cases.grid_case(*params))


@requires_gpu
@pytest.mark.parametrize("params", cases.EDGE_PARAMS, ids=cases.edge_id)
def test_kernel_matches_oracle_on_zero_update_rules(params):
    _check(cases.edge_case(*params))


@requires_gpu
@pytest.mark.parametrize("config", cases.SHAPE_CONFIGS, ids=cases.grid_id)
@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_kernel_matches_oracle_on_launch_shapes(shape, config):
    _check(cases.shape_case(shape, config))


@requires_gpu
@pytest.mark.parametrize("invariant", [False, True])
def test_no_examples(invariant):
    sgd, predict = _backend()
    w0, g0 = cases.warm_tables(42, 1 << 10)
    w, g = torch.from_numpy(w0).cuda(), torch.from_numpy(g0).cuda()
    s = torch.full((1 << 10,), 0.5, device="cuda")
    idx = torch.zeros(0, dtype=torch.int32, device="cuda")
    val = torch.zeros(0, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    y = torch.zeros(0, device="cuda")
    out = sgd(idx, val, off, y, w, g, cases.LR, cases.L2, 0.5, "logistic", y,
              s, invariant)
    assert out.shape == (0,) and out.is_cuda
    assert predict(idx, val, off, w).shape == (0,)
    assert np.array_equal(w.cpu().numpy().view(np.int32), w0.view(np.int32))
    assert np.array_equal(g.cpu().numpy().view(np.int32), g0.view(np.int32))
    assert bool((s == 0.5).all())


def _check_predict(batch, w):
    """vw_predict against sum w x in float64.  The kernel adds at most
    ceil(n/64) products per lane and then 6 tree levels, so its error is
    within (that depth + 1 for the product) * eps/2 of sum|w x|."""
    _, predict = _backend()
    b = _torch_batch(batch, "cuda")
    got = predict(b["idx"], b["val"], b["off"],
                  torch.from_numpy(w.copy()).cuda())
    assert got.shape == (batch.n_ex,) and got.dtype == torch.float32
    p, p_abs = cases.predict_oracle(batch, w)
    depth = -(-np.diff(batch.off) // 64) + 6 + 1
    tol = depth * 0.5 * cases.F32_EPS * p_abs
    err = np.abs(got.cpu().numpy().astype(np.float64) - p)
    print("PREDICT worst err/tol %.3f" % float(
        (err / np.maximum(tol, 1e-300)).max()))
    assert bool((err <= tol).all()), (err.max(), tol[err.argmax()])
    return p, p_abs


@requires_gpu
@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_predict_on_launch_shapes(shape):
    case = cases.shape_case(shape, cases.SHAPE_CONFIGS[0])
    assert bool(case.w0.any())
    _check_predict(case.batch, case.w0)


@requires_gpu
def test_predict_with_cancellation():
    batch, w = cases.cancelling_predict_case()
    p, p_abs = _check_predict(batch, w)
    big = np.diff(batch.off) >= 64
    assert bool((np.abs(p[big]) < 0.05 * p_abs[big]).all())


@requires_gpu
def test_logistic_invariant_solve_on_device():
    """One feature per example with x = 1, power_t 0, no normalisation, no
    l2, lr 1: scale = x_norm = 1, h_eta = h, q0 = y*w and the kernel's only
    arithmetic after the solve is w += y*d.  So y*(w_new - w) is the solve's
    d up to the rounding of that one add, eps/2 * max(|w|, |w_new|)."""
    sgd, _ = _backend()
    grid = cases.root_grid()
    n = len(grid)
    tol = cases.ROOT_TOL
    for ysign in (1.0, -1.0):
        q0 = np.array([q for q, _, _ in grid])
        w0 = (ysign * q0).astype(np.float32)
        w = torch.from_numpy(w0.copy()).cuda()
        g = torch.zeros(n, device="cuda")
        out = sgd(torch.arange(n, dtype=torch.int32, device="cuda"),
                  torch.ones(n, device="cuda"),
                  torch.arange(n + 1, dtype=torch.int64, device="cuda"),
                  torch.full((n,), ysign, device="cuda"), w, g, 1.0, 0.0,
                  0.0, "logistic",
                  torch.tensor([h for _, h, _ in grid], device="cuda"), None,
                  True)
        assert np.array_equal(out.cpu().numpy(), w0)
        w1 = w.cpu().numpy().astype(np.float64)
        assert np.isfinite(w1).all()
        worst = 0.0
        for k, (q, h, root) in enumerate(grid):
            d = ysign * (w1[k] - float(w0[k]))
            slack = 0.5 * cases.F32_EPS * max(abs(float(w0[k])), abs(w1[k]))
            worst = max(worst, (abs(d - root) - slack) / root)
            assert -slack <= d <= root * (1.0 + tol) + slack, (q, h, d, root)
            assert abs(d - root) <= tol * root + slack, (q, h, d, root)
        print("ROOT y=%+.0f worst (|d-root|-slack)/root = %.3e (tol %.3e)"
              % (ysign, worst, tol))


@requires_gpu
def test_colliding_updates_add_up():
    """Atomics under contention: every slot of a 64-slot table takes about
    940 updates from different waves.  The case is built so that the result
    is a plain sum in some order (see collision_case).

    w: the terms have random signs, so partial sums stay near sqrt(n) terms
    and the rounding error of any order is a fraction of eps * sum|term|;
    4 eps * sum|term| is asserted.  G: all terms are positive, partial sums
    grow to the full sum and the error of a random order is already about
    sqrt(n)/6 eps * sum (5 eps for n = 940), so the bound is the one that
    holds for every order, (n + 4) eps/2 * sum (4 for the roundings inside
    a term).  A lost or doubled update moves a slot by sum/n, about 20 times
    that.  Measured on MI355X: w 0.23 of its bound, G 9.2 eps * sum."""
    sgd, _ = _backend()
    c = cases.collision_case()
    n = cases.COLLISION_SLOTS
    w, g = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    preds = sgd(*(torch.from_numpy(c[k]).cuda()
                  for k in ("idx", "val", "off", "y")), w, g,
                cases.COLLISION_LR, 0.0, 0.0, "hinge",
                torch.from_numpy(c["h"]).cuda(), None, False)
    assert float(preds.abs().max()) < 1.0
    eps = cases.F32_EPS
    w_err = np.abs(w.cpu().numpy().astype(np.float64) - c["w"])
    g_err = np.abs(g.cpu().numpy().astype(np.float64) - c["g"])
    w_tol = 4 * eps * c["w_abs"]
    g_tol = (c["count"] + 4) * 0.5 * eps * c["g"]
    print("COLLISION worst err/tol w %.3f g %.3f; g err/(eps*sum) %.2f" % (
        float((w_err / w_tol).max()), float((g_err / g_tol).max()),
        float((g_err / (eps * c["g"])).max())))
    assert bool((w_err <= w_tol).all())
    assert bool((g_err <= g_tol).all())
