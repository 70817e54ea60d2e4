"""The float32 torch reference of the VW sparse-SGD kernels against the
float64 per-example oracle of vw_kernel_cases: the full loss x path x power_t
x normalized x l2 grid over three successive calls, the rules on which the
kernel and a naive vectorised reference part ways, and the logistic
--invariant solve against its exact root.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from . import vw_kernel_cases as cases


def _torch_batch(batch, device="cpu"):
    # copies: the case's arrays are read-only and shared between tests
    t = {k: torch.from_numpy(getattr(batch, k).copy()).to(device)
         for k in ("idx", "val", "off", "y")}
    t["h"] = None if batch.h is None else torch.from_numpy(
        batch.h.copy()).to(device)
    return t


def run_case(case, sgd, predict, device="cpu", report=None):
    """Drive sgd/predict through the case's calls and compare every tensor
    with the oracle after each one.  Returns the worst relative error per
    tensor; the caller asserts its own bound.  Exact properties (s, untouched
    entries, finiteness) are asserted here."""
    b = _torch_batch(case.batch, device)
    w = torch.from_numpy(case.w0.copy()).to(device)
    g = torch.from_numpy(case.g0.copy()).to(device)
    s = torch.zeros(case.table, device=device) if case.normalized else None
    touched = case.batch.touched()
    untouched = np.ones(case.table, dtype=bool)
    untouched[touched] = False
    worst = {"w": 0.0, "g": 0.0, "preds": 0.0}
    for lr, (preds, _, w64, g64, s64) in zip(case.lrs, case.steps):
        got = sgd(b["idx"], b["val"], b["off"], b["y"], w, g, lr, case.l2,
                  case.power_t, case.loss, b["h"], s, case.invariant)
        assert got.shape == (case.batch.n_ex,)
        wn, gn = w.cpu().numpy(), g.cpu().numpy()
        assert np.isfinite(wn).all() and np.isfinite(gn).all()
        for key, a, ref in (("preds", got.cpu().numpy(), preds),
                            ("w", wn[touched], w64[touched]),
                            ("g", gn[touched], g64[touched])):
            worst[key] = max(worst[key], cases.rel_err(a, ref))
        # entries that no example names: bit-equal to where they started
        assert np.array_equal(wn[untouched].view(np.int32),
                              case.w0[untouched].view(np.int32))
        assert np.array_equal(gn[untouched].view(np.int32),
                              case.g0[untouched].view(np.int32))
        if s is not None:  # copies of |x|: exact
            assert np.array_equal(s.cpu().numpy().astype(np.float64), s64)
    # scoring with the trained table, against the oracle's table
    got = predict(b["idx"], b["val"], b["off"], w).cpu().numpy()
    worst["preds"] = max(worst["preds"], cases.rel_err(
        got, cases.predict_oracle(case.batch, case.steps[-1][2])[0]))
    if report is not None:
        report(case, worst)
    return worst


def _print_errors(case, worst):
    print("ERR %-40s %-6s w=%.2e g=%.2e preds=%.2e" % (
        case.name, case.family, worst["w"], worst["g"], worst["preds"]))


def check_case(case, sgd, predict, margin, device="cpu"):
    worst = run_case(case, sgd, predict, device, _print_errors)
    for key, err in worst.items():
        tol = margin * cases.FLOOR[case.family][key]
        assert tol <= cases.MAX_TOL
        assert err <= tol, (case.name, key, err, tol)


def _ref():
    from mmlspark_amd.models.vw import sgd_ref
    return sgd_ref.vw_sgd_minibatch, sgd_ref.vw_predict


@pytest.mark.parametrize("params", cases.GRID_PARAMS, ids=cases.grid_id)
def test_reference_matches_oracle_on_grid(params):
    check_case(cases.grid_case(*params), *_ref(), cases.CPU_MARGIN)


@pytest.mark.parametrize("params", cases.EDGE_PARAMS, ids=cases.edge_id)
def test_reference_matches_oracle_on_zero_update_rules(params):
    case = cases.edge_case(*params)
    check_case(case, *_ref(), cases.CPU_MARGIN)
    # what the rules mean, read off the oracle itself
    b, (_, _, w1, g1, _) = case.batch, case.steps[0]
    loss, invariant = params[0], params[1]

    def unchanged(ex):
        i = b.idx[b.off[ex]:b.off[ex + 1]]
        return (np.array_equal(w1[i], case.w0[i].astype(np.float64))
                and np.array_equal(g1[i], case.g0[i].astype(np.float64)))

    if not invariant:
        assert unchanged(cases.EDGE_H0)
        assert unchanged(cases.EDGE_BEYOND) == (loss == "hinge")
    else:
        assert unchanged(cases.EDGE_ZEROS)
        assert not unchanged(cases.EDGE_H0)  # l2 still decays it
    assert not unchanged(cases.EDGE_PLAIN)


@pytest.mark.parametrize("config", cases.SHAPE_CONFIGS, ids=cases.grid_id)
@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_reference_matches_oracle_on_launch_shapes(shape, config):
    check_case(cases.shape_case(shape, config), *_ref(), cases.CPU_MARGIN)


@pytest.mark.parametrize("loss", cases.LOSSES)
def test_invariant_move_float32_against_exact(loss):
    from mmlspark_amd.models.vw.sgd_ref import _invariant_dp
    grid = cases.root_grid()
    q0 = torch.tensor([q for q, _, _ in grid], dtype=torch.float32)
    h_eta = torch.tensor([h for _, h, _ in grid], dtype=torch.float32)
    tol = cases.ROOT_TOL
    for y in (1.0, -1.0):
        yt = torch.full_like(q0, y)
        # for squared and hinge q0 is read as the prediction p itself
        pred = q0 * y if loss == "logistic" else q0
        dp = _invariant_dp(loss, pred, yt, h_eta)
        assert dp.dtype == torch.float32
        dp = dp.double().numpy()
        assert np.isfinite(dp).all()
        for k, (q, h, root) in enumerate(grid):
            p = float(pred[k])
            exact = cases.invariant_move(loss, p, y, h)
            if loss == "logistic":
                assert exact == y * root
            # along the direction of the exact move: never backwards, never
            # past it, and within tol of it
            d, e = dp[k] * np.sign(exact or 1.0), abs(exact)
            assert 0.0 <= d <= e * (1.0 + tol), (loss, y, q, h, d, e)
            assert abs(d - e) <= tol * e, (loss, y, q, h, d, e)
            if loss == "squared":   # never passes the label
                assert abs(dp[k]) <= abs(y - p)
            if loss == "hinge":     # never passes the margin
                assert y * (p + dp[k]) <= max(1.0, y * p)


def test_logistic_root_solves_its_equation():
    """The oracle's own root: residual of e^q0 (e^d - 1) + d = h_eta at the
    float64 neighbours of d straddles zero."""
    import math
    for q0, h_eta, d in cases.root_grid():
        a = math.exp(q0)

        def f(v):
            return a * math.expm1(v) + v - h_eta
        assert 0.0 < d <= h_eta
        assert f(np.nextafter(d, 0.0)) <= 0.0 <= f(np.nextafter(d, np.inf))


def test_oracle_by_hand():
    """One squared-loss example on each path, worked out by hand."""
    idx, x = np.array([3, 5]), np.array([2.0, -1.0])
    b = cases.Batch(idx, x, [0, 2], [1.0], [2.0])
    w, g = np.zeros(8), np.zeros(8)
    w[3], w[5], g[3] = 0.5, 1.0, 1.0
    wp, gp = w.copy(), g.copy()
    preds, _ = cases.oracle_step(b, wp, gp, None, 0.25, 0.0, 0.5, "squared",
                                 False)
    assert preds[0] == 0.0                  # 0.5*2 - 1*1
    gl = (0.0 - 1.0) * 2.0                  # (p - y) h
    G3, G5 = 1.0 + (gl * 2.0) ** 2, (gl * -1.0) ** 2
    np.testing.assert_allclose(gp[[3, 5]], [G3, G5], rtol=1e-15)
    np.testing.assert_allclose(
        wp[[3, 5]], [0.5 - 0.25 * gl * 2.0 / np.sqrt(G3 + 1e-10),
                     1.0 - 0.25 * gl * -1.0 / np.sqrt(G5 + 1e-10)],
        rtol=1e-15)
    wi, gi, s = w.copy(), g.copy(), np.zeros(8)
    cases.oracle_step(b, wi, gi, s, 0.25, 0.0, 0.0, "squared", True)
    assert s[3] == 2.0 and s[5] == 1.0
    x_norm = 4.0 / 2.0 + 1.0 / 1.0          # x^2 * 1 / s
    dp = (1.0 - 0.0) * (1.0 - np.exp(-2.0 * 0.25 * x_norm))
    np.testing.assert_allclose(
        wi[[3, 5]], [0.5 + dp / x_norm * 2.0 / 2.0,
                     1.0 + dp / x_norm * -1.0 / 1.0], rtol=1e-15)
    np.testing.assert_allclose(gi[[3, 5]], [G3, G5], rtol=1e-15)
    # the move lands the prediction where the closed form says
    assert abs(wi[3] * 2.0 - wi[5] - dp) < 1e-15
