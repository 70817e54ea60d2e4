"""als_kernels.hip against the float64 oracle of tests/als_cases.py."""
import numpy as np
import pytest
import torch

from mmlspark_amd.models import cyber
from mmlspark_amd.models.cyber import AccessAnomaly
from mmlspark_amd.ops import backend

from . import als_cases as ac

pytestmark = pytest.mark.gpu

HEAVY = 40
# 70 rows: more than one block, no multiple of 3 or 4 waves.  Degrees around
# the 32-entry tile, an empty row, and row 7 alone above the heavy threshold.
DEGREES = [0, 1, 31, 32, 33, 17, 40, 2 * HEAVY + 3] + [0, 1, 31, 32, 33, 9] * 10 \
    + [5, 12]


def _dev(*ts):
    return [t.cuda() for t in ts]


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("k", [1, 10, 31, 32, 33, 64])
def test_half_step_matches_oracle(k, implicit):
    assert len(DEGREES) == 70
    indptr, col, val = ac.csr(DEGREES, 50, k, implicit)
    Y = ac.factors(50, k, 100 + k)
    x = backend.als_half_step(*_dev(indptr, col, val, Y), 0.1, 1.5, implicit,
                              heavy=HEAVY)
    ac.check_half_step(x, indptr, col, val, Y, 0.1, 1.5, implicit)


@pytest.mark.parametrize("k", [1, 32, 33, 64])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_gram(n, k):
    Y = ac.factors(n, k, n + k)
    G = backend.als_gram(Y.cuda()).cpu().double()
    Yd = Y.double()
    bound = (n + 2) * ac.U32 * (Yd.abs().t() @ Yd.abs())
    assert bool(((G - Yd.t() @ Yd).abs() <= bound).all())
    assert torch.equal(G, G.t())


@pytest.mark.parametrize("implicit", [False, True])
def test_repeatable_and_blind_to_a_threshold_no_row_crosses(implicit):
    args = _dev(*ac.csr(DEGREES, 50, 3, implicit), ac.factors(50, 33, 4))
    x = backend.als_half_step(*args, 0.1, 1.5, implicit, heavy=HEAVY)
    again = backend.als_half_step(*args, 0.1, 1.5, implicit, heavy=HEAVY)
    moved = backend.als_half_step(*args, 0.1, 1.5, implicit, heavy=HEAVY + 20)
    assert torch.equal(x, again) and torch.equal(x, moved)
    G = backend.als_gram(args[3])
    assert torch.equal(G, backend.als_gram(args[3]))


@pytest.mark.parametrize("n", [1, 257])
def test_score_pairs(n):
    k = 10
    U, V = ac.factors(7 + 30, k, 1), ac.factors(5 + 40, k, 2)
    u_off, v_off = torch.tensor([0, 7, 37]), torch.tensor([0, 5, 45])
    mean = torch.tensor([0.3, -1.2], dtype=torch.float64)
    std = torch.tensor([0.7, 2.5], dtype=torch.float64)
    rng = np.random.default_rng(n)
    tenant = rng.integers(0, 2, n).astype(np.int32)
    user = rng.integers(0, np.array([7, 30])[tenant]).astype(np.int32)
    res = rng.integers(0, np.array([5, 40])[tenant]).astype(np.int32)
    bad = np.zeros(n, dtype=bool)
    if n > 1:       # out of range on either side, and an unknown tenant
        user[3], res[4], user[5], tenant[6] = 7 + 30, -1, -1, -1
        tenant[3], res[7], tenant[7] = 0, 5, 0
        bad[3:8] = True
    got = backend.als_score_pairs(*_dev(
        U, V, *map(torch.from_numpy, (user, res, tenant)), u_off, v_off, mean,
        std)).cpu().numpy()
    assert np.isnan(got[bad]).all()
    t = tenant[~bad]
    a = U.double().numpy()[u_off.numpy()[t] + user[~bad]]
    b = V.double().numpy()[v_off.numpy()[t] + res[~bad]]
    want = (-(a * b).sum(1) - mean.numpy()[t]) / std.numpy()[t]
    tol = (k + 2) * ac.U32 * ((np.abs(a) * np.abs(b)).sum(1)
                              + np.abs(mean.numpy()[t])) / std.numpy()[t]
    assert (np.abs(got[~bad] - want) <= tol).all()


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("implicit", [False, True])
def test_access_anomaly_on_the_gpu(implicit, fused, monkeypatch):
    monkeypatch.setenv("MMLSPARK_AMD_ALS_FUSED", fused)
    df, normal, anomalous = ac.indexed_access_log()
    model = AccessAnomaly(maxIter=8, rankParam=8, device="cuda",
                          applyImplicitCf=implicit).fit(df)
    assert ac.separates(model, normal, anomalous)
    # the one-launch scoring agrees with the per-row loop, NaN rows included
    probe = anomalous.assign(user_idx=[-1, 20] + list(anomalous["user_idx"])[2:])
    got = model.transform(probe)["anomaly_score"].to_numpy()
    model.set("device", "cpu")
    want = model.transform(probe)["anomaly_score"].to_numpy()
    assert np.isnan(want[:2]).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4, equal_nan=True)


@pytest.mark.parametrize("implicit", [False, True])
def test_fit_tracks_the_float64_fit(implicit):
    df, _, _ = ac.indexed_access_log()
    args = (20, 20, df["user_idx"].to_numpy(), df["res_idx"].to_numpy(),
            np.ones(len(df)))
    kw = dict(rank=8, reg=0.1, iters=3, seed=0, implicit=implicit, alpha=1.0)
    want = np.concatenate(ac.oracle_fit(*args, **kw))
    ref = torch.cat(cyber._als_csr(*args, device="cpu", **kw)).numpy()
    got = torch.cat(cyber._als_csr(*args, device="cuda", **kw)).cpu().numpy()
    ref_dev = np.abs(ref - want).max()
    dev = np.abs(got - want).max()
    print("implicit=%s cpu_ref deviation %.3e fused deviation %.3e"
          % (implicit, ref_dev, dev))
    # Measured on an MI355X host: the float32 torch fit is 2.03e-3 (explicit)
    # and 9.1e-4 (implicit) from the float64 fit on this data, factors up to
    # 3.9 in size; the fused fit may be 4x that away (8.1e-3, 3.6e-3) for MFMA
    # tile sums and Cholesky against torch's order and LU.  It measured
    # 4.7e-3 and 4.8e-4.
    assert dev <= 4 * ref_dev
