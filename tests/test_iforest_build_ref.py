"""cpu_ref.iforest_build, the definition of the fused isolation-forest build:
structure on the shared cases, the distributions of its draws, and
IsolationForest(fusedBuild=True) through the public estimator on the CPU."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from mmlspark_amd.models.iforest import IsolationForest, IsolationForestModel
from mmlspark_amd.ops import cpu_ref

from . import iforest_cases as ic


@pytest.mark.parametrize("name", list(ic.CASES))
def test_definition_passes_the_checker(name):
    X, sub_n, n_feat, boot = ic.case(name)
    out = ic.build(name, "cpu")
    ic.check_forest(X, sub_n, n_feat, boot, out)
    if name == "all-constant":
        assert np.array_equal(out[7], np.arange(ic.N_TREES + 1))
        assert (out[5] == 128).all() and (out[1] == -1).all()


def test_draw_distributions():
    """4000 single-level trees (sub_n = 2) over X = arange in 8 identical
    columns: u = (thr - lo) / (hi - lo) is uniform, the root's feature is
    uniform over 8, and every row is sampled with probability 2 / n."""
    n, T = 64, 4000
    X = np.repeat(np.arange(n, dtype=np.float32)[:, None], 8, axis=1)
    rows, feat, thr, *_ = (t.numpy() for t in cpu_ref.iforest_build(
        torch.from_numpy(X), T, 2, 8, False, 5))
    lo, hi = rows.min(1).astype(np.float64), rows.max(1).astype(np.float64)
    u = (thr[0::3] - lo) / (hi - lo)          # every tree: root, two leaves
    assert abs(u.mean() - 0.5) <= 4 / np.sqrt(12 * T)
    share = np.bincount(feat[0::3], minlength=8) / T
    assert (np.abs(share - 1 / 8) <= 4 * np.sqrt(1 / 8 * 7 / 8 / T)).all()
    p = 2 / n
    incl = np.bincount(rows.reshape(-1), minlength=n)
    assert (np.abs(incl - T * p) <= 5 * np.sqrt(T * p * (1 - p))).all()


def _outlier_frame():
    rng = np.random.default_rng(0)
    inliers = rng.normal(size=(500, 4)).astype(np.float32)
    outliers = rng.normal(size=(20, 4)).astype(np.float32) * 6 + 10
    return pd.DataFrame({"features": list(np.concatenate([inliers,
                                                          outliers]))})


def test_fused_estimator_finds_outliers_and_round_trips(tmp_path):
    df = _outlier_frame()
    m = IsolationForest(numEstimators=50, contamination=0.04, randomSeed=3,
                        fusedBuild=True).fit(df)
    out = m.transform(df)
    scores = out["outlierScore"].to_numpy()
    assert scores[500:].mean() > scores[:500].mean() + 0.1
    pred = out["predictedLabel"].to_numpy()
    assert pred[500:].mean() > 0.7
    assert pred[:500].mean() < 0.05
    m.save(os.path.join(tmp_path, "if"))
    m2 = IsolationForestModel.load(os.path.join(tmp_path, "if"))
    np.testing.assert_array_equal(
        m2.transform(df)["outlierScore"].to_numpy(), scores)


def test_host_builder_is_unchanged():
    """fusedBuild=False is the builder from before the option: the node
    count, first nodes and four scores below were recorded from it."""
    df = _outlier_frame()
    m = IsolationForest(numEstimators=5, randomSeed=3,
                        fusedBuild=False).fit(df)
    f = m.get("forestArrays")
    assert len(f["feature"]) == 385
    assert f["feature"][:6].tolist() == [1, 3, 1, -1, -1, 1]
    assert f["threshold"][:3].view(np.int32).tolist() == [
        -1087313887, -1073607769, -1082244268]
    scores = m.transform(df)["outlierScore"].to_numpy()
    np.testing.assert_allclose(
        scores[[0, 1, 510, 519]],
        [0.34673998, 0.3756682, 0.7226997, 0.7226997], rtol=1e-6)
