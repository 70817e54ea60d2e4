"""CSR forest scoring without densifying: the torch reference ops, Booster
and transform() on sparse input — all exact against the dense path."""
import numpy as np
import pandas as pd
import pytest
import torch

from mmlspark_amd.models.gbdt.booster import Booster
from mmlspark_amd.models.gbdt.sparse import CsrMatrix
from mmlspark_amd.ops import backend, cpu_ref

from . import csr_predict_cases as cases

FOREST_NAMES = ["t1", "t3", "t4", "t5", "t9", "stump", "multi3", "cat",
                "beyond", "unstored"]


def _matrix_for(name):
    csr = cases.edge_matrix()
    if name == "unstored":  # the rows that never store the split columns
        csr = csr.row_slice(0, cases.UNSTORED_ROWS)
    return csr


def _forest_args(f, value_key):
    return (f["feature"], f["threshold"], f["left"], f["right"], f[value_key],
            f["offsets"])


def test_edge_matrix_has_the_cases_it_claims():
    csr = cases.edge_matrix()
    assert csr.shape == (cases.N_ROWS, cases.N_COLS)
    lens = (csr.indptr[1:] - csr.indptr[:-1])
    assert lens[0] == 0 and lens[-1] == 0 and lens[10] == 0 and lens[11] == 0
    assert lens[1] == 1 and lens[cases.DENSE_ROW] == cases.N_COLS
    assert (csr.col == 0).any() and (csr.col == cases.N_COLS - 1).any()
    assert (csr.val == 0).any() and torch.isnan(csr.val).any()
    assert (csr.val < 0).any() and (csr.val >= 256).any()
    for r in range(cases.N_ROWS):  # strictly increasing columns per row
        c = csr.col[csr.indptr[r]:csr.indptr[r + 1]]
        assert bool((c[1:] > c[:-1]).all())
    head = csr.row_slice(0, cases.UNSTORED_ROWS)
    assert not np.isin(head.col.numpy(), cases.NEVER_STORED).any()
    b = cases.forests()
    assert any(int(t.feature.max()) >= cases.N_COLS for t in b["beyond"].trees)
    assert b["stump"].trees[0].n_nodes == 1
    assert any((t.cat_offset >= 0).any() for t in b["cat"].trees)


@pytest.mark.parametrize("name", FOREST_NAMES)
def test_cpu_ref_forest_csr_equals_dense(name):
    b = cases.forests()[name]
    csr = _matrix_for(name)
    f = cases.flat(b)
    X = cases.densified(csr, b.n_features)
    kw = dict(cat_offset=f["cat_offset"], cat_words=f["cat_words"])
    for start, num in ((0, -1), (1, 1), (0, 2), (2, -1), (1, 0)):
        ref = cpu_ref.predict_forest(*_forest_args(f, "value"), X,
                                     b.n_outputs, f["weights"], start, num,
                                     **kw)
        got = cpu_ref.predict_forest_csr(
            *_forest_args(f, "value"), csr.indptr, csr.col, csr.val,
            csr.shape[1], b.n_outputs, f["weights"], start, num, **kw)
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert torch.equal(got, ref), (name, start, num)
    # the dispatching op takes CPU tensors to the same reference
    got = backend.predict_forest_csr(
        *_forest_args(f, "value"), csr.indptr, csr.col, csr.val,
        csr.shape[1], b.n_outputs, f["weights"], **kw)
    assert torch.equal(got, cpu_ref.predict_forest(
        *_forest_args(f, "value"), X, b.n_outputs, f["weights"], **kw))


@pytest.mark.parametrize("name", FOREST_NAMES)
def test_cpu_ref_leaf_csr_equals_dense(name):
    b = cases.forests()[name]
    csr = _matrix_for(name)
    f = cases.flat(b)
    X = cases.densified(csr, b.n_features)
    kw = dict(cat_offset=f["cat_offset"], cat_words=f["cat_words"])
    ref = cpu_ref.predict_leaf(*_forest_args(f, "leaf_index"), X, **kw)
    got = cpu_ref.predict_leaf_csr(*_forest_args(f, "leaf_index"),
                                   csr.indptr, csr.col, csr.val,
                                   csr.shape[1], **kw)
    assert got.dtype == torch.int32 and torch.equal(got, ref)
    assert torch.equal(backend.predict_leaf_csr(
        *_forest_args(f, "leaf_index"), csr.indptr, csr.col, csr.val,
        csr.shape[1], **kw), ref)


def test_lookup_does_not_alias_the_next_row():
    """A split column beyond the width must not read the next row's entry
    whose global key (row * n_cols + col) it would share."""
    from mmlspark_amd.models.gbdt.tree import Tree
    nf = 4
    # row 0 empty; row 1 stores column 1 -> key 1*4+1 == 0*4+5
    csr = CsrMatrix(torch.tensor([0, 0, 1]), torch.tensor([1], dtype=torch.int32),
                    torch.tensor([9.0]), (2, nf))
    t = Tree([5, -1, -1], [1.0, 0, 0], [0, 0, 0], [1, -1, -1], [2, -1, -1],
             [0.0, 10.0, 20.0], [2, 1, 1], [1, 0, 0], [-1, 0, 1])
    b = Booster([t], "regression", 1, np.zeros(1, dtype=np.float32), 6)
    assert b.predict_raw(csr).view(-1).tolist() == [10.0, 10.0]
    assert b.predict_leaf(csr).view(-1).tolist() == [0, 0]


@pytest.mark.parametrize("name", FOREST_NAMES)
def test_booster_csr_equals_dense(name):
    b = cases.forests()[name]
    csr = _matrix_for(name)
    X = cases.densified(csr, b.n_features)
    for start, num in ((0, -1), (1, -1), (0, 1), (1, 1)):
        assert torch.equal(b.predict_raw(csr, start, num),
                           b.predict_raw(X, start, num)), (name, start, num)
    assert torch.equal(b.predict_leaf(csr), b.predict_leaf(X))


def test_booster_csr_honours_best_iteration():
    src = cases.forests()["t9"]
    b = Booster(src.trees, src.objective, 1, src.base_score, src.n_features,
                tree_weights=src.tree_weights)
    csr = cases.edge_matrix()
    X = csr.densify()
    full = b.predict_raw(csr)
    b.best_iteration = 3
    stopped = b.predict_raw(csr)
    assert torch.equal(stopped, b.predict_raw(X))
    assert torch.equal(stopped, b.predict_raw(csr, 0, 4))
    assert not torch.equal(stopped, full)
    # an explicit num_iteration overrides best_iteration
    assert torch.equal(b.predict_raw(csr, 0, 9), full)
    assert torch.equal(b.predict_raw(csr, 2, 5), b.predict_raw(X, 2, 5))


def test_zero_rows_and_empty_forest_shapes():
    b3 = cases.forests()["multi3"]
    f = cases.flat(b3)
    empty = CsrMatrix(torch.zeros(1, dtype=torch.int64),
                      torch.zeros(0, dtype=torch.int32),
                      torch.zeros(0), (0, cases.N_COLS))
    got = cpu_ref.predict_forest_csr(
        *_forest_args(f, "value"), empty.indptr, empty.col, empty.val,
        cases.N_COLS, 3, f["weights"])
    assert got.shape == (0, 3) and got.dtype == torch.float32
    got = cpu_ref.predict_leaf_csr(
        *_forest_args(f, "leaf_index"), empty.indptr, empty.col, empty.val,
        cases.N_COLS)
    assert got.shape == (0, 6) and got.dtype == torch.int32
    out = b3.predict_raw(empty)
    assert out.shape == (0, 3) and out.dtype == torch.float32
    assert b3.predict_leaf(empty).shape == (0, 6)

    csr = cases.edge_matrix()
    base = np.array([0.5, -1.0, 2.0], dtype=np.float32)
    none = Booster([], "multiclass", 3, base, cases.N_COLS)
    out = none.predict_raw(csr)
    assert out.shape == (cases.N_ROWS, 3)
    assert torch.equal(out, none.predict_raw(csr.densify()))
    assert torch.equal(out[0], torch.from_numpy(base))
    assert none.predict_raw(empty).shape == (0, 3)
    fe = cases.flat(none)
    assert cpu_ref.predict_forest_csr(
        *_forest_args(fe, "value"), csr.indptr, csr.col, csr.val,
        cases.N_COLS, 3).shape == (cases.N_ROWS, 3)
    assert cpu_ref.predict_leaf_csr(
        *_forest_args(fe, "leaf_index"), csr.indptr, csr.col, csr.val,
        cases.N_COLS).shape == (cases.N_ROWS, 0)
    # an all-empty matrix (no stored entry at all) scores as all zeros
    blank = CsrMatrix(torch.zeros(8, dtype=torch.int64),
                      torch.zeros(0, dtype=torch.int32), torch.zeros(0),
                      (7, cases.N_COLS))
    b = cases.forests()["t5"]
    assert torch.equal(b.predict_raw(blank),
                       b.predict_raw(torch.zeros(7, cases.N_COLS)))


def test_booster_scoring_never_densifies(monkeypatch):
    def boom(self, rows=None):
        raise AssertionError("CSR scoring must not densify")
    monkeypatch.setattr(CsrMatrix, "densify", boom)
    csr = cases.edge_matrix()
    for name in ("t9", "multi3", "cat"):
        b = cases.forests()[name]
        assert b.predict_raw(csr).shape == (cases.N_ROWS, b.n_outputs)
        assert b.predict_prob(csr).shape[0] == cases.N_ROWS
        assert b.predict_leaf(csr).shape == (cases.N_ROWS, b.num_trees)


@pytest.mark.parametrize("name", ["t5", "multi3"])
def test_predict_contrib_csr_equals_dense(name):
    b = cases.forests()[name]
    csr = cases.edge_matrix()
    # SHAP over stored NaNs follows the dense path's own rule either way
    dense = b.predict_contrib(csr.densify())
    got = b.predict_contrib(csr)
    assert got.shape == (cases.N_ROWS, b.n_outputs * (cases.N_COLS + 1))
    assert got.dtype == dense.dtype
    np.testing.assert_array_equal(got, dense)
    # more than one densified tile
    tiles = [c for _, c in csr.densify_chunks(chunk=256)]
    assert len(tiles) == 2
    empty = csr.row_slice(0, 0)
    assert b.predict_contrib(empty).shape == (0, got.shape[1])


def test_transform_with_shap_col_on_sparse_column():
    from mmlspark_amd.core.schema import SparseVector
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    rng = np.random.default_rng(3)
    n, nf = 400, 12
    rows, y = [], np.zeros(n, dtype=np.float32)
    w = rng.normal(size=nf)
    for i in range(n):
        idx = np.sort(rng.choice(nf, size=4, replace=False)).astype(np.int32)
        val = rng.normal(size=4).astype(np.float32)
        y[i] = 1.0 if (w[idx] * val).sum() > 0 else 0.0
        rows.append(SparseVector(nf, idx, val))
    df = pd.DataFrame({"features": rows, "label": y})
    model = LightGBMClassifier(numIterations=5, numLeaves=7, device="cpu",
                               featuresShapCol="shap",
                               leafPredictionCol="leaves").fit(df)
    out = model.transform(df)
    shap = np.stack([np.asarray(v) for v in out["shap"]])
    assert shap.shape == (n, nf + 1)
    X = np.zeros((n, nf), dtype=np.float32)
    for i, v in enumerate(rows):
        X[i, v.indices] = v.values
    Xt = torch.from_numpy(X)
    np.testing.assert_array_equal(
        shap.astype(np.float32), model.booster.predict_contrib(Xt))
    # contributions + expected value add up to the raw margin
    raw = model.booster.predict_raw(Xt).view(-1).numpy()
    np.testing.assert_allclose(shap.sum(axis=1), raw, rtol=1e-4, atol=1e-4)
    leaves = np.stack([np.asarray(v) for v in out["leaves"]])
    np.testing.assert_array_equal(
        leaves, model.booster.predict_leaf(Xt).numpy().astype(np.float64))
