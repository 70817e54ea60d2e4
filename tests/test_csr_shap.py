"""TreeSHAP over CSR rows with compact per-row contributions, on the CPU:
the float64 oracle against the independent per-row recursion, additivity,
compactness on a 100,000-column matrix, the dense contract built from the
compact result, and the estimator's sparse SHAP column."""
import numpy as np
import pandas as pd
import pytest
import torch

from . import csr_predict_cases as cases
from . import csr_shap_cases as shap


@pytest.mark.parametrize("name", shap.FOREST_NAMES)
def test_oracle_matches_independent_recursion(name):
    """cpu_ref.tree_shap_csr vs Tree.shap_values on the densified edge
    matrix.  The two differ only in the f32 folding of shrinkage, weight and
    cover ratio in the flat arrays: per cell within 2^-21 * S."""
    b = cases.forests()[name]
    phi, N, S = shap.edge_oracle(name)
    feats = b.used_features()
    U, K = feats.size, b.n_outputs
    assert phi.shape == (cases.N_ROWS, K, U + 1)
    assert not phi[..., U].any()  # the expected-value cell is the caller's
    X = cases.densified(cases.edge_matrix(), b.n_features).numpy()
    ref = np.zeros((cases.N_ROWS, K, b.n_features + 1))
    for ti, (t, w) in enumerate(zip(b.trees, b.tree_weights)):
        ref[:, ti % K] += t.shap_values(X, scale=float(w))
    rows = np.ones(cases.N_ROWS, dtype=bool)
    if name == "cat":
        rows[shap.CAT_FRACTIONAL_ROW] = False
    unused = np.setdiff1d(np.arange(b.n_features), feats)
    assert not ref[:, :, unused].any()
    err = np.abs(phi[..., :U] - ref[:, :, feats])[rows]
    bound = (2.0 ** -21 * S[..., :U])[rows]
    if err.size:
        print(f"{name}: max |err| {err.max():.3e}, worst err/bound "
              f"{(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert bool((err <= bound).all())
    if U:
        assert S[..., :U].max() > 0 and N[..., :U].max() >= 1


@pytest.mark.parametrize("name", shap.FOREST_NAMES)
def test_compact_values_add_up_to_the_margin(name):
    b = cases.forests()[name]
    csr = cases.edge_matrix()
    feats, values = shap.edge_cpu_compact(name)
    phi, N, S = shap.edge_oracle(name)
    assert isinstance(values, torch.Tensor) and values.dtype == torch.float32
    assert values.shape == phi.shape
    assert feats.dtype == np.int64 and np.array_equal(feats, np.unique(feats))
    # Booster's CPU path is the per-row recursion (bit-equal to the dense CPU
    # path), which truncates the fractional category the scorer rounds
    rows = np.ones(cases.N_ROWS, dtype=bool)
    if name == "cat":
        rows[shap.CAT_FRACTIONAL_ROW] = False
    shap.check_cells(values.numpy()[rows], phi[rows], N[rows], S[rows],
                     b._tree_depth(), name)
    expected = b.expected_value()
    np.testing.assert_array_equal(
        values[:, :, -1].numpy(),
        np.broadcast_to(expected.astype(np.float32), values.shape[:2]))
    raw = b.predict_raw(csr).numpy().astype(np.float64)
    total = values.numpy().astype(np.float64).sum(-1)
    tol = shap.additivity_bound(b, N, S, expected)
    assert bool((np.abs(total - raw) <= tol)[rows].all()), \
        float((np.abs(total - raw) / tol)[rows].max())
    # the op's own CPU implementation is the oracle, cast to float32
    got = shap.run_op(b, csr, "cpu")
    assert got.dtype == torch.float32
    np.testing.assert_array_equal(got.numpy(), phi.astype(np.float32))


def test_wide_matrix_result_is_compact():
    """The CPU path is a per-row recursion, so it explains the first 200
    rows (still 100,000 columns wide); the GPU test runs all 5000."""
    csr, b = cases.wide_case()
    assert csr.shape == (cases.WIDE_ROWS, cases.WIDE_COLS)
    feats, values = b.predict_contrib_sparse(csr.row_slice(0, 200))
    U = feats.size
    assert 0 < U <= 48 and int(feats.min()) >= 90_000
    assert values.shape == (200, 1, U + 1)
    phi, N, S = shap.oracle_on(b, csr.row_slice(0, 200))
    shap.check_cells(values.numpy(), phi, N, S, b._tree_depth(), "wide")


@pytest.mark.parametrize("name", ["t5", "multi3", "beyond"])
def test_dense_contract_is_the_compact_result_scattered(name):
    b = cases.forests()[name]
    csr = cases.edge_matrix()
    feats, values = shap.edge_cpu_compact(name)
    dense = b.predict_contrib(csr)
    K, nf, U = b.n_outputs, b.n_features, feats.size
    assert dense.dtype == np.float32
    assert dense.shape == (cases.N_ROWS, K * (nf + 1))
    want = np.zeros((cases.N_ROWS, K, nf + 1), dtype=np.float32)
    v = values.numpy()
    for j, f in enumerate(feats):
        want[:, :, f] = v[:, :, j]
    want[:, :, nf] = v[:, :, U]
    np.testing.assert_array_equal(dense.reshape(-1, K, nf + 1), want)
    unused = np.setdiff1d(np.arange(nf), feats)
    assert unused.size and not dense.reshape(-1, K, nf + 1)[:, :, unused].any()


def test_row_window_and_degenerate_inputs():
    from mmlspark_amd.models.gbdt.booster import Booster
    from mmlspark_amd.models.gbdt.sparse import CsrMatrix
    b = cases.forests()["multi3"]
    phi, _, _ = shap.edge_oracle("multi3")
    got = shap.run_op(b, cases.edge_matrix(), "cpu", row_begin=37,
                      row_end=263)
    assert got.dtype == torch.float32
    np.testing.assert_array_equal(got.numpy(),
                                  phi[37:263].astype(np.float32))
    U = b.used_features().size
    empty = CsrMatrix(torch.zeros(1, dtype=torch.int64),
                      torch.zeros(0, dtype=torch.int32), torch.zeros(0),
                      (0, cases.N_COLS))
    feats, values = b.predict_contrib_sparse(empty)
    assert values.shape == (0, 3, U + 1)
    assert b.predict_contrib(empty).shape == (0, 3 * (cases.N_COLS + 1))
    blank = CsrMatrix(torch.zeros(8, dtype=torch.int64),
                      torch.zeros(0, dtype=torch.int32), torch.zeros(0),
                      (7, cases.N_COLS))
    _, values = b.predict_contrib_sparse(blank)
    assert values.shape == (7, 3, U + 1)
    shap.check_cells(values.numpy(), *shap.oracle_on(b, blank),
                     b._tree_depth(), "all-empty rows")
    assert bool((values == values[0]).all()) and bool(values[..., :U].any())
    none = Booster([], "multiclass", 3, np.array([0.5, -1.0, 2.0],
                                                 dtype=np.float32),
                   cases.N_COLS)
    feats, values = none.predict_contrib_sparse(cases.edge_matrix())
    assert feats.size == 0 and values.shape == (cases.N_ROWS, 3, 1)
    assert torch.equal(values[:, :, 0], none.predict_raw(cases.edge_matrix()))


def test_estimator_sparse_shap_column():
    from mmlspark_amd.core.schema import SparseVector
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    rng = np.random.default_rng(11)
    n, nf = 600, 40
    rows, y = [], np.zeros(n, dtype=np.float32)
    w = rng.normal(size=nf)
    for i in range(n):
        idx = np.sort(rng.choice(nf, size=6, replace=False)).astype(np.int32)
        val = rng.normal(size=6).astype(np.float32)
        y[i] = 1.0 if (w[idx] * val).sum() > 0 else 0.0
        rows.append(SparseVector(nf, idx, val))
    df = pd.DataFrame({"features": rows, "label": y})
    est = LightGBMClassifier(numIterations=4, numLeaves=7, device="cpu",
                             featuresShapCol="shap", featuresShapSparse=True)
    model = est.fit(df)
    assert model.get("featuresShapSparse") is True
    col = model.transform(df)["shap"]
    used = model.booster.used_features()
    assert 0 < used.size < nf
    want_idx = np.concatenate([used, [nf]])
    for v in col:
        assert isinstance(v, SparseVector) and v.size == nf + 1
        assert np.array_equal(v.indices, want_idx)
    model.set("featuresShapSparse", False)
    dense = np.stack([np.asarray(v) for v in model.transform(df)["shap"]])
    assert dense.shape == (n, nf + 1)
    np.testing.assert_array_equal(
        np.stack([v.to_dense() for v in col]), dense.astype(np.float32))
    # dense features: the flag changes nothing
    X = np.stack([v.to_dense() for v in rows])
    ddf = pd.DataFrame({"features": list(X), "label": y})
    model.set("featuresShapSparse", True)
    out = model.transform(ddf)["shap"]
    assert not isinstance(out.iloc[0], SparseVector)
    assert np.asarray(out.iloc[0]).shape == (nf + 1,)
