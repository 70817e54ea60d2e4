"""tree_shap_csr_k on MI355X against the float64 oracle, per cell within
(N + D + 5) * 2^-23 * S (csr_shap_cases.cell_bound has the derivation)."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from . import csr_predict_cases as cases
from . import csr_shap_cases as shap

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")


@functools.lru_cache(maxsize=None)
def _edge_on_device():
    return cases.edge_matrix().to("cuda")


def _check_edge(name, lo=0, hi=cases.N_ROWS, **kw):
    b = cases.forests()[name]
    phi, N, S = shap.edge_oracle(name)
    got = shap.run_op(b, _edge_on_device(), "cuda", row_begin=lo, row_end=hi,
                      **kw)
    assert got.is_cuda and got.dtype == torch.float32
    assert got.shape == (hi - lo,) + phi.shape[1:]
    assert not bool(got[..., -1].any())  # expected value is the caller's
    shap.check_cells(got.cpu().numpy(), phi[lo:hi], N[lo:hi], S[lo:hi],
                     b._tree_depth(), f"{name}[{lo}:{hi}] {kw}")
    return got


@requires_gpu
@pytest.mark.parametrize("name", shap.FOREST_NAMES)
def test_every_forest_on_the_edge_matrix(name):
    _check_edge(name)


@requires_gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_launch_shapes_tiled_rows(n):
    """tiled_matrix(n) row i is edge row (i + 5) % 300: the oracle is the
    edge oracle, indexed."""
    b = cases.forests()["t9"]
    phi, N, S = shap.edge_oracle("t9")
    idx = (np.arange(n) + 5) % cases.N_ROWS
    got = shap.run_op(b, cases.tiled_matrix(n), "cuda")
    assert got.shape == (n,) + phi.shape[1:]
    shap.check_cells(got.cpu().numpy(), phi[idx], N[idx], S[idx],
                     b._tree_depth(), f"t9 tiled {n}")


@requires_gpu
@pytest.mark.parametrize("max_blocks", [1, 2])
def test_grid_stride_passes(max_blocks):
    """300 rows x 9 trees = 2700 pairs on 256 or 512 threads: 11 or 6
    grid-stride passes, the last one ragged."""
    _check_edge("t9", max_blocks=max_blocks)


@requires_gpu
def test_row_window_mid_matrix():
    _check_edge("t9", 37, 263)
    _check_edge("multi3", 37, 263, max_blocks=1)


@requires_gpu
def test_multiclass_trees_land_in_their_class_plane():
    """multi3 has 6 trees; dropping all trees but those of class k must
    reproduce plane k and leave the other planes zero."""
    from mmlspark_amd.models.gbdt.booster import Booster
    from mmlspark_amd.models.gbdt.tree import Tree
    b = cases.forests()["multi3"]
    _check_edge("multi3")
    zero = Tree([-1], [0.0], [0], [-1], [-1], [0.0], [1.0], [0.0], [0])
    for k in range(3):
        # class-k trees at their positions t % 3 == k, 0-valued stumps else
        trees = [t if i % 3 == k else zero for i, t in enumerate(b.trees)]
        only = Booster(trees, "multiclass", 3, b.base_score, b.n_features,
                       tree_weights=b.tree_weights)
        got = shap.run_op(only, _edge_on_device(), "cuda").cpu()
        assert bool(got[:, k].any())
        for other in range(3):
            if other != k:
                assert not bool(got[:, other].any())
        phi, N, S = shap.oracle_on(only, cases.edge_matrix())
        shap.check_cells(got.numpy(), phi, N, S, only._tree_depth(),
                         f"multi3 class {k}")


@requires_gpu
@pytest.mark.parametrize("name", ["beyond", "unstored"])
def test_features_no_row_stores_are_credited(name):
    """`beyond` splits on columns at or past the matrix width, `unstored` on
    columns rows [0, 200) never store: those rows read 0.0 there and the
    contributions are the oracle's — present, not dropped."""
    b = cases.forests()[name]
    hi = cases.UNSTORED_ROWS if name == "unstored" else cases.N_ROWS
    got = _check_edge(name, 0, hi).cpu().numpy()
    feats = b.used_features()
    absent = (feats >= cases.N_COLS) if name == "beyond" \
        else np.isin(feats, cases.NEVER_STORED)
    assert absent.any()
    phi, _, _ = shap.edge_oracle(name)
    assert np.abs(phi[:hi][:, :, :-1][:, :, absent]).max() > 1e-3
    assert np.abs(got[:, :, :-1][:, :, absent]).max() > 1e-3


@requires_gpu
def test_wide_matrix_stays_compact_on_the_device():
    csr, b = cases.wide_case()
    dev = csr.to("cuda")
    b._flat(dev.device), b._shap_flat(dev.device)  # cached model arrays
    raw = b.predict_raw(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    feats, values = b.predict_contrib_sparse(dev)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"wide: peak memory rise {rise / 2**20:.2f} MiB")
    assert rise < 64 * 2**20  # a dense tile of these rows would be 2 GB
    U = feats.size
    assert values.is_cuda and values.shape == (cases.WIDE_ROWS, 1, U + 1)
    assert U <= 48
    phi, N, S = shap.wide_oracle()
    v = values.cpu().numpy()
    shap.check_cells(v[:200], phi[:200], N[:200], S[:200], b._tree_depth(),
                     "wide, first 200 rows")
    expected = b.expected_value()
    total = v.astype(np.float64).sum(-1)
    tol = shap.additivity_bound(b, N, S, expected)
    err = np.abs(total - raw.cpu().numpy().astype(np.float64))
    print(f"wide additivity: worst err/bound {(err / tol).max():.3f}")
    assert bool((err <= tol).all())


@requires_gpu
def test_zero_rows_empty_rows_and_empty_forest():
    from mmlspark_amd.models.gbdt.booster import Booster
    from mmlspark_amd.models.gbdt.sparse import CsrMatrix
    b = cases.forests()["multi3"]
    U = b.used_features().size
    empty = CsrMatrix(torch.zeros(1, dtype=torch.int64),
                      torch.zeros(0, dtype=torch.int32), torch.zeros(0),
                      (0, cases.N_COLS)).to("cuda")
    out = shap.run_op(b, empty, "cuda")
    assert out.is_cuda and out.shape == (0, 3, U + 1)
    feats, values = b.predict_contrib_sparse(empty)
    assert values.is_cuda and values.shape == (0, 3, U + 1)
    assert b.predict_contrib(empty).shape == (0, 3 * (cases.N_COLS + 1))
    # an empty window of a non-empty matrix
    out = shap.run_op(b, _edge_on_device(), "cuda", row_begin=40, row_end=40)
    assert out.shape == (0, 3, U + 1)
    blank = CsrMatrix(torch.zeros(8, dtype=torch.int64),
                      torch.zeros(0, dtype=torch.int32), torch.zeros(0),
                      (7, cases.N_COLS))
    got = shap.run_op(b, blank, "cuda")
    assert got.shape == (7, 3, U + 1)
    shap.check_cells(got.cpu().numpy(), *shap.oracle_on(b, blank),
                     b._tree_depth(), "all-empty rows")
    none = Booster([], "multiclass", 3,
                   np.array([0.5, -1.0, 2.0], dtype=np.float32), cases.N_COLS)
    feats, values = none.predict_contrib_sparse(_edge_on_device())
    assert feats.size == 0 and values.is_cuda
    assert values.shape == (cases.N_ROWS, 3, 1)
    assert torch.equal(values[:, :, 0], none.predict_raw(_edge_on_device()))
    torch.cuda.synchronize()


@requires_gpu
@pytest.mark.parametrize("name", ["t9", "multi3", "cat"])
def test_dense_contract_equals_the_dense_kernel(name):
    """predict_contrib(csr.cuda()) vs predict_contrib(densified.cuda()): both
    kernels add the same addends in their own atomic order, so each is
    within the cell bound of the oracle and they are within twice it of each
    other; cells of unused features are exactly 0 in both."""
    b = cases.forests()[name]
    dev = _edge_on_device()
    K, nf = b.n_outputs, b.n_features
    sparse = b.predict_contrib(dev).reshape(-1, K, nf + 1)
    dense = b.predict_contrib(
        cases.densified(dev, nf)).reshape(-1, K, nf + 1)
    feats = b.used_features()
    _, N, S = shap.edge_oracle(name)
    tol = 2 * shap.cell_bound(N, S, b._tree_depth())[..., :-1]
    diff = np.abs(sparse[:, :, feats].astype(np.float64) - dense[:, :, feats])
    print(f"{name}: max |csr - dense| {diff.max():.3e}, worst diff/bound "
          f"{(diff / np.maximum(tol, 1e-300)).max():.3f}")
    assert bool((diff <= tol).all())
    unused = np.setdiff1d(np.arange(nf), feats)
    assert not sparse[:, :, unused].any() and not dense[:, :, unused].any()
    np.testing.assert_array_equal(sparse[:, :, nf], dense[:, :, nf])


@requires_gpu
def test_estimator_sparse_shap_column_on_the_device():
    from mmlspark_amd.core.schema import SparseVector
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    rng = np.random.default_rng(4)
    n, nf = 2000, 60
    rows, y = [], np.zeros(n, dtype=np.float32)
    w = rng.normal(size=nf)
    for i in range(n):
        idx = np.sort(rng.choice(nf, size=10, replace=False)).astype(np.int32)
        val = rng.normal(size=10).astype(np.float32)
        y[i] = 1.0 if (w[idx] * val).sum() > 0 else 0.0
        rows.append(SparseVector(nf, idx, val))
    df = pd.DataFrame({"features": rows, "label": y})
    model = LightGBMClassifier(numIterations=10, numLeaves=15, device="cuda",
                               featuresShapCol="shap",
                               featuresShapSparse=True).fit(df)
    out = model.transform(df)
    b = model.booster
    used = b.used_features()
    col = out["shap"]
    assert all(isinstance(v, SparseVector) and v.size == nf + 1
               and np.array_equal(v.indices, np.concatenate([used, [nf]]))
               for v in col)
    compact = np.stack([v.to_dense() for v in col]).astype(np.float64)
    model.set("featuresShapSparse", False)
    flag_off = np.stack([np.asarray(v) for v in
                         model.transform(df)["shap"]]).astype(np.float64)
    csr = model._X(df, torch.device("cpu"))
    _, N, S = shap.oracle_on(b, csr)
    cell = shap.cell_bound(N, S, b._tree_depth())[:, 0, :-1]
    diff = np.abs(compact[:, used] - flag_off[:, used])
    print(f"estimator: worst diff/bound "
          f"{(diff / np.maximum(2 * cell, 1e-300)).max():.3f}")
    assert bool((diff <= 2 * cell).all())  # two runs of the float atomics
    unused = np.setdiff1d(np.arange(nf), used)
    assert not compact[:, unused].any() and not flag_off[:, unused].any()
    np.testing.assert_array_equal(compact[:, nf], flag_off[:, nf])
    margin = np.stack([np.asarray(v) for v in out["rawPrediction"]])[:, -1]
    tol = shap.additivity_bound(b, N, S, b.expected_value())[:, 0]
    assert bool((np.abs(compact.sum(axis=1) - margin) <= tol).all())
