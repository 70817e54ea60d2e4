"""GPU tests for the stream pool of the native GBDT grower: with
MMLSPARK_AMD_GROWER_STREAMS at 1, 2 and 3 the independent split chains run on
one, two and three streams, and every array `grow_tree_native` hands back —
node arrays, concatenated leaf rows, offsets — must be the same, and the
model must equal the Python grower's.

One fit per setting: a race that needs repeated runs to show is not what
these tests look for; they pin the result of each path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

N_ROWS = 30_000
ENV = "MMLSPARK_AMD_GROWER_STREAMS"


def _dataset(nf, seed, n_cat=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N_ROWS, nf)).astype(np.float32)
    logit = (X[:, n_cat] * 0.5 + X[:, nf - 1]
             + 0.3 * np.sin(3 * X[:, min(n_cat + 2, nf - 1)]))
    if n_cat:
        cats = rng.integers(0, 24, size=(N_ROWS, n_cat))
        X[:, :n_cat] = cats
        # non-monotone in the category id: needs one-vs-rest set splits
        logit = logit + 1.5 * ((cats[:, 0] % 3 == 0) ^ (cats[:, 1] % 5 == 0))
    y = (logit + 0.3 * rng.normal(size=N_ROWS) > 0.4 * bool(n_cat))
    return X, y.astype(np.float32)


def _fit(X, y, monkeypatch, n_cat, streams=None, python_grower=False):
    """Fit once; returns (model string, list of per-tree result dicts)."""
    import pandas as pd
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    from mmlspark_amd.ops import _hip_grower
    df = pd.DataFrame({"features": list(X), "label": y})
    kw = dict(numIterations=4, numLeaves=63, minDataInLeaf=1,
              featureFraction=0.8, device="cuda")
    if n_cat:
        kw["categoricalSlotIndexes"] = list(range(n_cat))
    grown = []
    real = _hip_grower.grow_tree_native

    def recording(*a, **k):
        d = real(*a, **k)
        grown.append({key: v.cpu().numpy() for key, v in d.items()})
        return d

    with monkeypatch.context() as mp:
        mp.setattr(_hip_grower, "grow_tree_native", recording)
        if streams is not None:
            mp.setenv(ENV, str(streams))
        if python_grower:
            mp.setenv("MMLSPARK_AMD_NO_NATIVE_GROWER", "1")
        model = LightGBMClassifier(**kw).fit(df)
    return model.booster, grown


def _check_streams(X, y, monkeypatch, n_cat=0):
    b_py, none = _fit(X, y, monkeypatch, n_cat, python_grower=True)
    assert not none, "the Python grower must not call the native one"
    b1, trees1 = _fit(X, y, monkeypatch, n_cat, streams=1)
    assert len(trees1) == 4
    assert max(len(t["feature"]) for t in trees1) == 2 * 63 - 1
    assert b1.save_to_string() == b_py.save_to_string()
    for streams in (2, 3):
        b, trees = _fit(X, y, monkeypatch, n_cat, streams=streams)
        assert len(trees) == len(trees1)
        for t, (got, want) in enumerate(zip(trees, trees1)):
            assert got.keys() == want.keys()
            for key in want:
                assert got[key].dtype == want[key].dtype, (streams, t, key)
                assert np.array_equal(got[key], want[key]), (streams, t, key)
        assert b.save_to_string() == b_py.save_to_string(), streams
    return b1


@requires_gpu
@pytest.mark.parametrize("nf", [5, 100])
def test_grower_streams_identical_trees(nf, monkeypatch):
    monkeypatch.delenv("MMLSPARK_AMD_FORCE_DIST_GROWER", raising=False)
    X, y = _dataset(nf, seed=40 + nf)
    _check_streams(X, y, monkeypatch)


@requires_gpu
@pytest.mark.parametrize("nf", [5, 100])
def test_grower_streams_identical_trees_categorical(nf, monkeypatch):
    monkeypatch.delenv("MMLSPARK_AMD_FORCE_DIST_GROWER", raising=False)
    X, y = _dataset(nf, seed=50 + nf, n_cat=4)
    b = _check_streams(X, y, monkeypatch, n_cat=4)
    assert any((t.cat_offset >= 0).any() for t in b.trees), \
        "no categorical split was taken"


@requires_gpu
@pytest.mark.parametrize("nf", [5, 100])
def test_grower_streams_identical_trees_dist_codepath(nf, monkeypatch):
    """The distributed code path without a process group: child ranges come
    from the device left count, of which every stream keeps its own."""
    monkeypatch.setenv("MMLSPARK_AMD_FORCE_DIST_GROWER", "1")
    X, y = _dataset(nf, seed=60 + nf)
    _check_streams(X, y, monkeypatch)


@requires_gpu
def test_grower_streams_env_is_validated(monkeypatch):
    X, y = _dataset(5, seed=1)
    for bad in ("0", "4", "many"):
        with pytest.raises(RuntimeError, match=ENV):
            _fit(X, y, monkeypatch, 0, streams=bad)
