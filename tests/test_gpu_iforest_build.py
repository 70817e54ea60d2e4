"""iforest_build_k + iforest_compact_k on MI355X: bit-for-bit against the numpy
definition (cpu_ref.iforest_build) on the shared cases, the checker on the
device result alone, the public estimator on both paths, and agreement of
the fused forest's scores with the host builder's."""
import numpy as np
import pandas as pd
import pytest

from mmlspark_amd.models.iforest import IsolationForest

from . import iforest_cases as ic

pytestmark = pytest.mark.gpu

NAMES = ("sample_rows", "feature", "threshold", "left", "right", "size",
         "depth", "offsets")


@pytest.mark.parametrize("name", list(ic.CASES))
def test_kernel_equals_definition(name):
    X, sub_n, n_feat, boot = ic.case(name)
    got, want = ic.build(name, "cuda"), ic.build(name, "cpu")
    for what, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        if what == "threshold":
            g, w = g.view(np.int32), w.view(np.int32)
        assert np.array_equal(g, w), what
    ic.check_forest(X, sub_n, n_feat, boot, got)


def _outlier_frame():
    rng = np.random.default_rng(0)
    inliers = rng.normal(size=(500, 4)).astype(np.float32)
    outliers = rng.normal(size=(20, 4)).astype(np.float32) * 6 + 10
    return pd.DataFrame({"features": list(np.concatenate([inliers,
                                                          outliers]))})


def test_estimator_same_model_on_both_paths(monkeypatch):
    df = _outlier_frame()
    est = IsolationForest(numEstimators=50, contamination=0.04, randomSeed=3,
                          fusedBuild=True)
    m_gpu = est.fit(df)
    monkeypatch.setenv("MMLSPARK_AMD_IFOREST_FUSED", "0")
    m_ref = est.fit(df)
    fa, fb = m_gpu.get("forestArrays"), m_ref.get("forestArrays")
    assert set(fa) == set(fb)
    for k in fa:
        assert fa[k].dtype == fb[k].dtype and np.array_equal(fa[k], fb[k]), k
    assert m_gpu.get("scoreThreshold") == m_ref.get("scoreThreshold")
    out = m_gpu.transform(df)
    scores = out["outlierScore"].to_numpy()
    assert np.array_equal(scores, m_ref.transform(df)["outlierScore"]
                          .to_numpy())
    assert scores[500:].mean() > scores[:500].mean() + 0.1
    pred = out["predictedLabel"].to_numpy()
    assert pred[500:].mean() > 0.7
    assert pred[:500].mean() < 0.05


def test_fused_forest_agrees_with_host_forests():
    """Scores of 300-tree forests on 500 held-out points.  Two host forests
    with different seeds differ by at most `ref` (reference against
    reference); the fused forest, a third independent draw of the same
    estimator, may differ from the first host forest by twice that.
    Measured on MI355X: ref = 0.03437, fused = 0.02847."""
    rng = np.random.default_rng(4)
    train = pd.DataFrame({"features": list(
        rng.normal(size=(2000, 6)).astype(np.float32))})
    held = rng.normal(size=(500, 6)).astype(np.float32)
    held[:25] = held[:25] * 4 + 6
    held = pd.DataFrame({"features": list(held)})

    def scores(**kw):
        m = IsolationForest(numEstimators=300, **kw).fit(train)
        return m.transform(held)["outlierScore"].to_numpy()

    host = scores(randomSeed=1)
    ref = np.abs(host - scores(randomSeed=2)).max()
    fused = np.abs(host - scores(randomSeed=1, fusedBuild=True)).max()
    print("host vs host %.5f, fused vs host %.5f" % (ref, fused))
    assert fused <= 2 * ref
