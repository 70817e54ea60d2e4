"""CSR forest scoring kernels on MI355X: bit-equal to the dense kernels on
the densified matrix, and to the CPU CSR reference's leaf assignment."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from . import csr_predict_cases as cases

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

FOREST_NAMES = ["t1", "t3", "t4", "t5", "t9", "stump", "multi3", "cat",
                "beyond", "unstored"]
# one row, a ragged single block, one row into a second block, the edge
# matrix itself (0 = as built, 300 rows), and many blocks with a ragged last
# one
ROW_COUNTS = [1, 255, 257, 0, 70_001]


@functools.lru_cache(maxsize=None)
def _matrix(n_rows):
    """(csr on cpu, csr on device) — built once per row count, read-only."""
    csr = cases.edge_matrix() if n_rows == 0 else cases.tiled_matrix(n_rows)
    return csr, csr.to("cuda")


def _inputs(name, n_rows):
    b = cases.forests()[name]
    cpu, dev = _matrix(n_rows)
    if name == "unstored":  # rows that never store the split columns
        assert n_rows == 0
        cpu = cpu.row_slice(0, cases.UNSTORED_ROWS)
        dev = dev.row_slice(0, cases.UNSTORED_ROWS)
    return b, cpu, dev


def _args(f, value_key):
    return (f["feature"], f["threshold"], f["left"], f["right"], f[value_key],
            f["offsets"])


def _check(b, cpu, dev):
    from mmlspark_amd.ops import backend, cpu_ref
    f = cases.flat(b, "cuda")
    fc = cases.flat(b, "cpu")
    kw = dict(cat_offset=f["cat_offset"], cat_words=f["cat_words"])
    X = cases.densified(dev, b.n_features)
    n = cpu.shape[0]
    for start, num in ((0, -1), (1, 1)):
        got = backend.predict_forest_csr(
            *_args(f, "value"), dev.indptr, dev.col, dev.val, dev.shape[1],
            b.n_outputs, f["weights"], start, num, **kw)
        ref = backend.predict_forest(*_args(f, "value"), X, b.n_outputs,
                                     f["weights"], start, num, **kw)
        assert got.is_cuda and got.shape == (n, b.n_outputs)
        assert torch.equal(got, ref), (start, num)
    leaf = backend.predict_leaf_csr(*_args(f, "leaf_index"), dev.indptr,
                                    dev.col, dev.val, dev.shape[1], **kw)
    assert leaf.dtype == torch.int32
    assert torch.equal(leaf, backend.predict_leaf(*_args(f, "leaf_index"), X,
                                                  **kw))
    # independent of the dense kernels and of densify(): the CPU CSR lookup
    ref_leaf = cpu_ref.predict_leaf_csr(
        *_args(fc, "leaf_index"), cpu.indptr, cpu.col, cpu.val, cpu.shape[1],
        cat_offset=fc["cat_offset"], cat_words=fc["cat_words"])
    assert torch.equal(leaf.cpu(), ref_leaf)
    # the scores are the leaves the CPU reference reaches, in tree order
    if b.n_outputs == 1:
        node = _leaf_nodes(fc, ref_leaf)
        vals = (fc["value"][node] * fc["weights"].unsqueeze(0))
        got = backend.predict_forest_csr(
            *_args(f, "value"), dev.indptr, dev.col, dev.val, dev.shape[1],
            1, f["weights"], **kw).cpu().view(-1)
        # float sums in another order: a few ulps of the largest partial sum
        tol = 4 * len(b.trees) * torch.finfo(torch.float32).eps \
            * vals.abs().sum(dim=1).clamp(min=1.0)
        assert bool(((got - vals.sum(dim=1)).abs() <= tol).all())


def _leaf_nodes(fc, leaf_ordinals):
    """Flat node id of leaf ordinal k in tree t."""
    off = fc["offsets"]
    out = torch.empty_like(leaf_ordinals, dtype=torch.int64)
    for t in range(off.numel() - 1):
        li = fc["leaf_index"][off[t]:off[t + 1]]
        pos = torch.full((int(li.max()) + 1,), -1, dtype=torch.int64)
        nodes = torch.nonzero(li >= 0).view(-1)
        pos[li[nodes].long()] = nodes + off[t]
        out[:, t] = pos[leaf_ordinals[:, t].long()]
    return out


@requires_gpu
@pytest.mark.parametrize("name,n_rows", [
    (name, n) for name in FOREST_NAMES for n in ROW_COUNTS
    # "unstored" is defined on the edge matrix's first rows only
    if name != "unstored" or n == 0])
def test_csr_kernels_equal_dense_kernels(name, n_rows):
    _check(*_inputs(name, n_rows))


@requires_gpu
def test_csr_kernels_wide_matrix_high_columns():
    csr, b = cases.wide_case()
    assert csr.shape == (5000, 100_000)
    assert int((csr.indptr[1:] - csr.indptr[:-1]).max()) <= 40
    assert min(int(t.feature[t.feature >= 0].min()) for t in b.trees) >= 90_000
    _check(b, csr, csr.to("cuda"))


@requires_gpu
def test_csr_ops_zero_rows_and_empty_window():
    from mmlspark_amd.models.gbdt.sparse import CsrMatrix
    from mmlspark_amd.ops import backend
    b = cases.forests()["multi3"]
    f = cases.flat(b, "cuda")
    empty = CsrMatrix(torch.zeros(1, dtype=torch.int64),
                      torch.zeros(0, dtype=torch.int32), torch.zeros(0),
                      (0, cases.N_COLS)).to("cuda")
    out = backend.predict_forest_csr(
        *_args(f, "value"), empty.indptr, empty.col, empty.val, cases.N_COLS,
        3, f["weights"])
    assert out.shape == (0, 3) and out.is_cuda
    assert backend.predict_leaf_csr(
        *_args(f, "leaf_index"), empty.indptr, empty.col, empty.val,
        cases.N_COLS).shape == (0, 6)
    _, dev = _matrix(0)
    out = backend.predict_forest_csr(
        *_args(f, "value"), dev.indptr, dev.col, dev.val, cases.N_COLS, 3,
        f["weights"], start_tree=3, num_iteration=0)
    assert out.shape == (cases.N_ROWS, 3) and not bool(out.any())
    assert b.predict_raw(empty).shape == (0, 3)
    blank = CsrMatrix(torch.zeros(8, dtype=torch.int64),
                      torch.zeros(0, dtype=torch.int32), torch.zeros(0),
                      (7, cases.N_COLS)).to("cuda")
    assert torch.equal(b.predict_raw(blank), b.predict_raw(
        torch.zeros(7, cases.N_COLS, device="cuda")))


@requires_gpu
def test_sparse_fit_transform_equals_densified_scoring():
    """A model fit on sparse rows on the GPU scores its sparse column through
    the CSR kernels; the outputs equal scoring the densified rows with the
    same booster through the dense kernels."""
    from mmlspark_amd.core.schema import SparseVector
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    rng = np.random.default_rng(4)
    n, nf = 6000, 60
    rows, y = [], np.zeros(n, dtype=np.float32)
    w = rng.normal(size=nf)
    for i in range(n):
        idx = np.sort(rng.choice(nf, size=10, replace=False)).astype(np.int32)
        val = rng.normal(size=10).astype(np.float32)
        y[i] = 1.0 if (w[idx] * val).sum() > 0 else 0.0
        rows.append(SparseVector(nf, idx, val))
    df = pd.DataFrame({"features": rows, "label": y})
    model = LightGBMClassifier(numIterations=10, numLeaves=15, device="cuda",
                               leafPredictionCol="leaves",
                               featuresShapCol="shap").fit(df)
    out = model.transform(df)
    X = np.zeros((n, nf), dtype=np.float32)
    for i, v in enumerate(rows):
        X[i, v.indices] = v.values
    Xd = torch.from_numpy(X).cuda()
    booster = model.booster
    raw = np.stack([np.asarray(v) for v in out["rawPrediction"]])
    prob = np.stack([np.asarray(v) for v in out["probability"]])
    dense_raw = booster.predict_raw(Xd, 0, 10)
    dense_prob = booster.predict_prob(Xd).cpu().numpy().astype(np.float64)
    margin = dense_raw.cpu().numpy().astype(np.float64)[:, 0]
    np.testing.assert_array_equal(raw[:, -1], margin)
    np.testing.assert_array_equal(prob, dense_prob)
    leaves = np.stack([np.asarray(v) for v in out["leaves"]])
    np.testing.assert_array_equal(
        leaves, booster.predict_leaf(Xd).cpu().numpy().astype(np.float64))
    # SHAP: tree_shap_k adds per-tree terms with float atomics, so two runs
    # of it differ in summation order — not a bit-equality case.  Ten trees
    # of |leaf| < 1 terms: reordering moves a sum by ~10 * 2^-23 * sum|term|,
    # well inside 1e-5.
    shap = np.stack([np.asarray(v) for v in out["shap"]])
    assert shap.shape == (n, nf + 1)
    np.testing.assert_allclose(shap, booster.predict_contrib(Xd),
                               rtol=0, atol=1e-5)
    np.testing.assert_allclose(shap.sum(axis=1), margin, rtol=0, atol=1e-4)
