"""ALS half step in ops/cpu_ref.py against the float64 oracle, and the
AccessAnomaly options built on it (implicit feedback, likelihood ratings)."""
import numpy as np
import pytest
import torch

from mmlspark_amd.models import cyber
from mmlspark_amd.models.cyber import AccessAnomaly, ComplementAccessTransformer
from mmlspark_amd.ops import backend

from . import als_cases as ac


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("k", [1, 10, 33])
def test_half_step_matches_oracle(k, implicit):
    indptr, col, val = ac.csr([3, 0, 5, 1, 40, 17], 12, k, implicit)
    Y = ac.factors(12, k, 100 + k)
    x = backend.als_half_step(indptr, col, val, Y, 0.1, 1.5, implicit)
    ac.check_half_step(x, indptr, col, val, Y, 0.1, 1.5, implicit)


def test_implicit_separates_groups_without_complement(monkeypatch):
    def no_sampling(self, df):
        raise AssertionError("implicit mode must not draw a complement set")
    monkeypatch.setattr(ComplementAccessTransformer, "_transform", no_sampling)
    df, normal, anomalous = ac.indexed_access_log()
    model = AccessAnomaly(maxIter=8, rankParam=8, applyImplicitCf=True).fit(df)
    assert ac.separates(model, normal, anomalous)


def test_likelihood_is_scaled_before_the_solver(monkeypatch):
    df, _, _ = ac.indexed_access_log()
    df = df.drop_duplicates(["user_idx", "res_idx"]).copy()
    df["likelihood"] = np.random.default_rng(1).uniform(3.0, 900.0, len(df))
    seen = []
    real = backend.als_half_step

    def spy(indptr, col, val, *a, **kw):
        seen.append(val)
        return real(indptr, col, val, *a, **kw)
    monkeypatch.setattr(backend, "als_half_step", spy)
    AccessAnomaly(maxIter=1, applyImplicitCf=True, likelihoodCol="likelihood",
                  lowValue=5.0, highValue=10.0).fit(df)
    assert len(seen) == 2
    for v in seen:      # the extremes of the column land on the two ends
        assert v.numel() == len(df)
        assert float(v.min()) == 5.0 and float(v.max()) == 10.0


def test_default_fit_is_the_parent_als():
    df, _, _ = ac.indexed_access_log()
    model = AccessAnomaly(maxIter=3).fit(df)
    neg = ComplementAccessTransformer(complementsetFactor=2, seed=0).transform(df)
    u = np.concatenate([df["user_idx"], neg["user_idx"]])
    r = np.concatenate([df["res_idx"], neg["res_idx"]])
    y = np.concatenate([np.ones(len(df)), np.zeros(len(neg))])
    U, V = cyber._als(20, 20, u, r, y, rank=10, reg=0.1, iters=3, seed=0)
    assert np.array_equal(model.get("userFactors")["t0"], U.numpy())
    assert np.array_equal(model.get("resFactors")["t0"], V.numpy())
    assert model.get("device") == "cpu"


@pytest.mark.parametrize("breakage", ["dtype", "stride", "decreasing", "end",
                                      "column", "rank"])
def test_bad_inputs_raise(breakage):
    indptr, col, val = ac.csr([3, 2, 4], 6, 0, False)
    Y = ac.factors(6, 65 if breakage == "rank" else 4, 1)
    if breakage == "dtype":
        col = col.long()
    elif breakage == "stride":
        val = val.repeat_interleave(2)[::2]
    elif breakage == "decreasing":
        indptr = torch.tensor([0, 5, 3, 9])
    elif breakage == "end":
        indptr = torch.tensor([0, 3, 5, 8])
    elif breakage == "column":
        col[4] = 6
    with pytest.raises(ValueError):
        backend.als_half_step(indptr, col, val, Y, 0.1, 1.0, False)
