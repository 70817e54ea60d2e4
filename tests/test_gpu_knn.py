"""knn_partial_topk_k + knn_merge_k on MI355X: bit-for-bit against the
float64 oracle on the exact (integer) cases of knn_cases, ties, splits,
labels and repeatability included; the float cases within the bound derived
in knn_cases; KNN / ConditionalKNN through the fused path against the
torch path they replace."""
import numpy as np
import pandas as pd
import pytest
import torch

from mmlspark_amd.models.knn import KNN, ConditionalKNN
from mmlspark_amd.ops import backend

from . import knn_cases as kc

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")


@requires_gpu
@pytest.mark.parametrize("name", kc.EXACT_NAMES)
def test_exact_cases_bit_for_bit_and_repeatable(name):
    d2, idx = kc.run(name, "cuda")
    assert d2.is_cuda and idx.is_cuda
    kc.check_exact(d2, idx, name)
    again_d, again_i = kc.run(name, "cuda")
    assert torch.equal(d2, again_d) and torch.equal(idx, again_i)


@requires_gpu
def test_identical_points_come_back_in_index_order():
    _, idx = kc.run("identical-300", "cuda")
    want = torch.arange(64, dtype=torch.int32).expand(3, 64)
    assert torch.equal(idx.cpu(), want)


@requires_gpu
@pytest.mark.parametrize("name", kc.SPLIT_NAMES)
def test_every_split_count_gives_identical_tensors(name):
    base_d, base_i = kc.run(name, "cuda", splits=1)
    kc.check_exact(base_d, base_i, name)
    for splits in (2, 7):
        d2, idx = kc.run(name, "cuda", splits=splits)
        assert torch.equal(d2, base_d) and torch.equal(idx, base_i)


@requires_gpu
@pytest.mark.parametrize("name", ("float-33", "float-33-labels"))
def test_float_results_do_not_depend_on_splits(name):
    base_d, base_i = kc.run(name, "cuda", splits=1)
    for splits in (0, 2, 7):
        d2, idx = kc.run(name, "cuda", splits=splits)
        assert torch.equal(d2, base_d) and torch.equal(idx, base_i)


@requires_gpu
@pytest.mark.parametrize("name", kc.LABEL_NAMES)
def test_label_edge_queries(name):
    c = kc.case(name)
    d2, idx = kc.run(name, "cuda")
    d2, idx = d2.cpu(), idx.cpu()
    assert (idx[0] == -1).all() and torch.isinf(d2[0]).all()
    if c["allowed"][1].sum() < c["k"]:
        m = int(c["allowed"][1].sum())
        assert (idx[1, :m] >= 0).all() and (idx[1, m:] == -1).all()
        assert torch.isinf(d2[1, m:]).all()
    free_d, free_i = kc.run(name, "cuda", labels=False)
    assert torch.equal(idx[2], free_i[2].cpu())
    assert torch.equal(d2[2], free_d[2].cpu())


@requires_gpu
@pytest.mark.parametrize("name", kc.FLOAT_NAMES)
def test_float_cases_within_bound(name):
    d2, idx = kc.run(name, "cuda")
    worst = kc.check_float(d2, idx, name)
    print(f"{name}: worst share of the bound on gfx950 {worst:.3f}")
    again_d, again_i = kc.run(name, "cuda")
    assert torch.equal(d2, again_d) and torch.equal(idx, again_i)


# ------------------------------------------------------------------ models
def _int_frames(n_labels=None, n=600, n_q=70, d=4, seed=30):
    """Integer features in [-1000, 1000]: every squared norm, product sum
    and squared distance stays below 4 * 2000^2 < 2^24, so float32 is exact
    and both paths must agree to the bit; the seed is one without ties
    among any query's 600 distances (asserted)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-1000, 1001, size=(n, d)).astype(np.float32)
    Q = rng.integers(-1000, 1001, size=(n_q, d)).astype(np.float32)
    D = ((Q[:, None, :].astype(np.int64) - X[None, :, :].astype(np.int64))
         ** 2).sum(axis=2)
    assert all(len(np.unique(row)) == n for row in D)
    index = pd.DataFrame({"features": list(X), "values": list(range(n))})
    query = pd.DataFrame({"features": list(Q)})
    labels = None
    if n_labels:
        labels = rng.integers(0, n_labels, size=n)
        index["labels"] = labels
        query["conditioner"] = [
            rng.choice(n_labels, size=rng.integers(1, 4),
                       replace=False).tolist() for _ in range(n_q)]
    return index, query, D, labels


def _both_paths(model, query, monkeypatch):
    monkeypatch.setenv("MMLSPARK_AMD_KNN_FUSED", "0")
    old = model.transform(query)["output"].tolist()
    monkeypatch.setenv("MMLSPARK_AMD_KNN_FUSED", "1")
    new = model.transform(query)["output"].tolist()
    return old, new


@requires_gpu
def test_knn_model_fused_equals_torch_path(monkeypatch):
    index, query, D, _ = _int_frames()
    model = KNN(k=5).fit(index)
    old, new = _both_paths(model, query, monkeypatch)
    assert new == old   # values and distances, exactly
    want = np.argsort(D, axis=1, kind="stable")[:, :5]
    assert [[m["value"] for m in row] for row in new] == want.tolist()


@requires_gpu
def test_conditional_knn_16_labels_fused_equals_torch_path(monkeypatch):
    index, query, _, _ = _int_frames(n_labels=16)
    model = ConditionalKNN(k=5).fit(index)
    old, new = _both_paths(model, query, monkeypatch)
    assert new == old


@requires_gpu
def test_conditional_knn_100_labels_against_brute_force(monkeypatch):
    index, query, D, labels = _int_frames(n_labels=100)
    model = ConditionalKNN(k=5).fit(index)
    widths = []
    real = backend.knn_topk

    def spy(Q, X, xsq, k, label_ids=None, allow_bits=None, splits=0):
        widths.append(None if allow_bits is None else allow_bits.shape[1])
        return real(Q, X, xsq, k, label_ids, allow_bits, splits)

    monkeypatch.setattr(backend, "knn_topk", spy)
    out = model.transform(query)["output"].tolist()
    assert widths == [4]
    for i, row in enumerate(out):
        ok = np.isin(labels, query["conditioner"][i])
        cand = np.flatnonzero(ok)
        order = cand[np.argsort(D[i, cand], kind="stable")][:5]
        assert [m["value"] for m in row] == order.tolist()
        assert [m["label"] for m in row] == labels[order].tolist()
        # d2 is exact; the float32 square root may differ by an ulp
        np.testing.assert_allclose([m["distance"] for m in row],
                                   np.sqrt(D[i, order].astype(np.float64)),
                                   rtol=2.0 ** -22, atol=0)


@requires_gpu
def test_k_above_the_kernel_limit_takes_the_torch_path(monkeypatch):
    index, query, D, _ = _int_frames()
    k = backend.KNN_MAX_K + 1
    model = KNN(k=k).fit(index)
    calls = []
    real = backend.knn_topk
    monkeypatch.setattr(backend, "knn_topk",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    out = model.transform(query)["output"].tolist()
    assert not calls
    want = np.sort(np.sqrt(D.astype(np.float64)), axis=1)[:, :k]
    got = np.array([[m["distance"] for m in row] for row in out])
    assert got.shape == (len(query), k)
    np.testing.assert_allclose(np.sort(got, axis=1), want, rtol=2.0 ** -22,
                               atol=0)


@requires_gpu
def test_index_is_uploaded_once_per_model():
    index, query, _, _ = _int_frames()
    model = KNN(k=5).fit(index)
    model.transform(query)
    X, xsq = model._index_on(torch.device("cuda"))
    model.transform(query)
    again_X, again_xsq = model._index_on(torch.device("cuda"))
    assert again_X is X and again_xsq is xsq
    assert X.is_cuda and X.shape == (600, 4)
