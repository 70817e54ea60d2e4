"""The two ends of a tree in the native GBDT grower: the root read in place
from the static bin planes (rows_identity), the single wait for the root
split, and the prediction update launched by the grower.  Each has an
environment switch, and nothing that `grow_tree_native` hands back, no model
and no score may depend on it.

30 000 rows; 5, 9 and 100 features give 1, 2 and 13 bin planes with 5, 1 and
4 valid bytes in the last one.  num_leaves 2: the root split is the only
split; 3: the first write into arena buffer 0, the smallest tree in which
aliasing could corrupt the static planes; 63: the benchmark's."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

N_ROWS = 30_000
ENV_STREAMS = "MMLSPARK_AMD_GROWER_STREAMS"
ENV_DIST = "MMLSPARK_AMD_FORCE_DIST_GROWER"
ENV_ROOT_STATIC = "MMLSPARK_AMD_GROWER_ROOT_STATIC"
ENV_ONE_WAIT = "MMLSPARK_AMD_GROWER_ROOT_ONE_WAIT"
ENV_APPLY = "MMLSPARK_AMD_GROWER_APPLY"
SWITCHES = (ENV_ROOT_STATIC, ENV_ONE_WAIT, ENV_APPLY)


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


def _clean_env(mp):
    for name in SWITCHES + (ENV_STREAMS, ENV_DIST,
                            "MMLSPARK_AMD_NO_NATIVE_GROWER"):
        mp.delenv(name, raising=False)


def _new_session(nf, n_cat, num_leaves=63, **cfg_kw):
    from mmlspark_amd.models.gbdt.objectives import make_objective
    from mmlspark_amd.models.gbdt.trainer import TrainConfig, TrainingSession
    from mmlspark_amd.parallel.comm import Comm
    X, y = _dataset(nf, seed=70 + nf + n_cat, n_cat=n_cat)
    cfg = TrainConfig(num_iterations=3, num_leaves=num_leaves,
                      min_data_in_leaf=1,
                      categorical_features=list(range(n_cat)) or None,
                      **cfg_kw)
    return TrainingSession(torch.from_numpy(X).cuda(),
                           torch.from_numpy(y).cuda(), cfg,
                           make_objective("binary"), Comm())


@functools.lru_cache(maxsize=None)
def _grow_inputs(nf, n_cat):
    """One session per data shape, with its first tree's gradients; shared by
    every direct call and never changed."""
    ses = _new_session(nf, n_cat)
    g, h = ses.objective.grad_hess(ses.preds, ses.y, None)
    g, h = g[:, 0].contiguous(), h[:, 0].contiguous()
    ses.grower.set_scales(g, h)
    return ses, g, h


def _grow(nf, n_cat, num_leaves, rows_identity=False, dist=False, **kw):
    """One direct grow_tree_native call, set up as TreeGrower._grow_native
    does; returns {key: numpy array}."""
    from mmlspark_amd.ops import _hip_grower
    ses, g, h = _grow_inputs(nf, n_cat)
    gr, cfg = ses.grower, ses.cfg
    num_mask = cats_t = None
    if n_cat:
        num_mask = torch.ones(gr.nf_pad, dtype=torch.bool, device="cuda")
        num_mask[:n_cat] = False
        cats_t = torch.arange(n_cat, dtype=torch.int64)
    d = _hip_grower.grow_tree_native(
        gr.binned, gr.binned_pair, ses.all_rows, g, h, cfg.max_bin, gr.nf,
        gr.scale_g, gr.scale_h, 0.0, 0.0, 1.0, cfg.min_sum_hessian_in_leaf,
        0.0, 0.0, num_leaves, -1, num_mask, cats_t, gr.cat_smooth, None, dist,
        rows_identity=rows_identity, **kw)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in d.items()}


def _assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for key in want:
        assert got[key].dtype == want[key].dtype, (what, key)
        assert np.array_equal(got[key], want[key]), (what, key)


@requires_gpu
@pytest.mark.parametrize("n_cat", [0, 4])
@pytest.mark.parametrize("num_leaves", [2, 3, 63])
@pytest.mark.parametrize("nf", [5, 9, 100])
def test_rows_identity_same_result_static_planes_untouched(
        nf, num_leaves, n_cat, monkeypatch):
    _clean_env(monkeypatch)
    ses, _, _ = _grow_inputs(nf, n_cat)
    pair0 = ses.grower.binned_pair.clone()
    binned0 = ses.grower.binned.clone()
    for streams in ("1", "3"):
        for dist in (False, True):
            monkeypatch.setenv(ENV_STREAMS, streams)
            what = (streams, dist)
            off = _grow(nf, n_cat, num_leaves, rows_identity=False, dist=dist)
            on = _grow(nf, n_cat, num_leaves, rows_identity=True, dist=dist)
            _assert_same(on, off, what)
            assert 3 <= len(on["feature"]) <= 2 * num_leaves - 1, what
            if num_leaves <= 3:  # this data always has two splits to offer
                assert len(on["feature"]) == 2 * num_leaves - 1, what
            assert int(on["leaf_offsets"][-1]) == N_ROWS, what
            assert np.array_equal(np.sort(on["leaf_rows"]),
                                  np.arange(N_ROWS)), what
            assert torch.equal(ses.grower.binned_pair, pair0), what
            assert torch.equal(ses.grower.binned, binned0), what
    if n_cat and num_leaves == 63:
        assert (on["cat_offset"] >= 0).any(), "no categorical split was taken"


@requires_gpu
def test_rows_identity_needs_every_row(monkeypatch):
    from mmlspark_amd.ops import _hip_grower
    _clean_env(monkeypatch)
    ses, g, h = _grow_inputs(5, 0)
    gr, cfg = ses.grower, ses.cfg
    with pytest.raises(RuntimeError, match="rows_identity"):
        _hip_grower.grow_tree_native(
            gr.binned, gr.binned_pair, ses.all_rows[:1000].contiguous(), g, h,
            cfg.max_bin, gr.nf, gr.scale_g, gr.scale_h, 0.0, 0.0, 1.0, 1e-3,
            0.0, 0.0, 3, -1, None, None, 10.0, None, False,
            rows_identity=True)


@requires_gpu
@pytest.mark.parametrize("nf", [5, 100])
def test_root_one_wait_same_result(nf, monkeypatch):
    _clean_env(monkeypatch)
    for n_cat in (0, 4):
        monkeypatch.setenv(ENV_ONE_WAIT, "0")
        off = _grow(nf, n_cat, 63, rows_identity=True)
        monkeypatch.setenv(ENV_ONE_WAIT, "1")
        on = _grow(nf, n_cat, 63, rows_identity=True)
        _assert_same(on, off, n_cat)


@requires_gpu
def test_grower_applies_update_once_with_python_rounding(monkeypatch):
    """preds_col[row] += (float)((double)value * shrinkage), exactly once,
    into a strided column; switched off, the column is left alone."""
    _clean_env(monkeypatch)
    shrink = 0.1
    for env, applied in ((None, 1), ("0", 0)):
        if env is not None:
            monkeypatch.setenv(ENV_APPLY, env)
        preds = torch.zeros(N_ROWS, 2, device="cuda")
        d = _grow(9, 0, 63, rows_identity=True, preds_col=preds[:, 1],
                  shrinkage=shrink)
        assert d["preds_applied"].tolist() == [applied]
        want = np.zeros(N_ROWS, dtype=np.float32)
        if applied:
            offs = d["leaf_offsets"]
            for i, nid in enumerate(d["leaf_nodes"]):
                want[d["leaf_rows"][offs[i]:offs[i + 1]]] = np.float32(
                    float(d["value"][nid]) * shrink)
            assert np.count_nonzero(want) > N_ROWS // 2
        got = preds.cpu().numpy()
        assert np.array_equal(got[:, 1], want)
        assert not got[:, 0].any()
    no_col = _grow(9, 0, 63, rows_identity=True)
    assert no_col["preds_applied"].tolist() == [0]


def _steps(nf, env, monkeypatch, n_steps=3, **cfg_kw):
    with monkeypatch.context() as mp:
        _clean_env(mp)
        for name, value in env.items():
            mp.setenv(name, value)
        ses = _new_session(nf, 0, **cfg_kw)
        for _ in range(n_steps):
            ses.step()
        torch.cuda.synchronize()
    assert len(ses.trees) == n_steps
    return ses.preds.clone(), ses.booster().save_to_string()


@requires_gpu
@pytest.mark.parametrize("nf", [5, 100])
def test_session_scores_and_trees_independent_of_switches(nf, monkeypatch):
    preds, model = _steps(nf, {}, monkeypatch)
    for name in SWITCHES:
        p, m = _steps(nf, {name: "0"}, monkeypatch)
        assert m == model, name
        assert torch.equal(p, preds), name


def _fit(X, y, monkeypatch, python_grower=False, env=None, **kw):
    """Fit once; returns (model string, rows_identity of every native call,
    preds_applied of every native call)."""
    import pandas as pd
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    from mmlspark_amd.ops import _hip_grower
    df = pd.DataFrame({"features": list(X), "label": y})
    flags, applied = [], []
    real = _hip_grower.grow_tree_native

    def recording(*a, **k):
        flags.append(k.get("rows_identity", a[22] if len(a) > 22 else False))
        d = real(*a, **k)
        applied.append(int(d["preds_applied"][0]))
        return d

    with monkeypatch.context() as mp:
        _clean_env(mp)
        mp.setattr(_hip_grower, "grow_tree_native", recording)
        for name, value in (env or {}).items():
            mp.setenv(name, value)
        if python_grower:
            mp.setenv("MMLSPARK_AMD_NO_NATIVE_GROWER", "1")
        model = LightGBMClassifier(numIterations=3, minDataInLeaf=1,
                                   device="cuda", **kw).fit(df)
    return model.booster.save_to_string(), flags, applied


@requires_gpu
@pytest.mark.parametrize("nf,num_leaves",
                         [(5, 63), (9, 2), (9, 3), (100, 63)])
def test_fit_equals_python_grower_and_passes_identity(nf, num_leaves,
                                                      monkeypatch):
    X, y = _dataset(nf, seed=80 + nf)
    want, none, _ = _fit(X, y, monkeypatch, python_grower=True,
                         numLeaves=num_leaves)
    assert not none, "the Python grower must not call the native one"
    got, flags, applied = _fit(X, y, monkeypatch, numLeaves=num_leaves)
    assert got == want
    assert flags == [True] * 3 and applied == [1] * 3
    # bagging: a row subset, so today's gather
    bag = dict(numLeaves=num_leaves, baggingFraction=0.5, baggingFreq=1)
    want, _, _ = _fit(X, y, monkeypatch, python_grower=True, **bag)
    got, flags, applied = _fit(X, y, monkeypatch, **bag)
    assert got == want
    assert flags == [False] * 3 and applied == [1] * 3


@requires_gpu
@pytest.mark.parametrize("boosting", ["dart", "rf"])
def test_dart_and_rf_unchanged(boosting, monkeypatch):
    """dart hands the update to the grower only in iterations that dropped no
    tree; rf never updates the scores."""
    X, y = _dataset(9, seed=90)
    kw = dict(numLeaves=15, boostingType=boosting)
    if boosting == "dart":
        kw.update(dropRate=0.5, skipDrop=0.0)
    else:
        kw.update(baggingFraction=0.6, baggingFreq=1)
    want, _, _ = _fit(X, y, monkeypatch, python_grower=True, **kw)
    got, flags, applied = _fit(X, y, monkeypatch, **kw)
    assert got == want
    if boosting == "rf":
        assert flags == [False] * 3 and applied == [0] * 3
    else:
        assert flags == [True] * 3 and applied[0] == 1


@requires_gpu
@pytest.mark.parametrize("boosting", ["dart", "rf"])
def test_dart_and_rf_scores_not_updated_twice(boosting, monkeypatch):
    """Scores after 3 steps against the Python grower's.  A second
    application would move a row by a whole shrunken leaf value (1e-2 and
    up here); the two growers' float32 updates differ by rounding at most."""
    kw = dict(boosting=boosting)
    if boosting == "dart":
        kw.update(drop_rate=0.5, skip_drop=0.0)
    else:
        kw.update(bagging_fraction=0.6, bagging_freq=1)
    want, m_want = _steps(9, {"MMLSPARK_AMD_NO_NATIVE_GROWER": "1"},
                          monkeypatch, **kw)
    got, m_got = _steps(9, {}, monkeypatch, **kw)
    assert m_got == m_want
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(),
                               rtol=0, atol=1e-5)


@requires_gpu
@pytest.mark.parametrize("name", SWITCHES)
def test_switches_are_validated(name, monkeypatch):
    _clean_env(monkeypatch)
    for bad in ("2", "on", "-1"):
        monkeypatch.setenv(name, bad)
        with pytest.raises(RuntimeError, match=name):
            _grow(5, 0, 3)
