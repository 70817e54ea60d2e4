"""backend.knn_topk on CPU tensors (cpu_ref.knn_topk), its float64 oracle,
the host-side validation and the label-bitset helper of models/knn.py.  The
cases and checks are those the GPU kernels face in test_gpu_knn.py."""
import numpy as np
import pytest
import torch

from mmlspark_amd.models.knn import label_bitsets
from mmlspark_amd.ops import backend

from . import knn_cases as kc


@pytest.mark.parametrize("name", ("q129-n129-d33-k64", "triples",
                                  "labels-33"))
def test_f64_oracle_is_the_int64_brute_force(name):
    c = kc.case(name)
    Q = c["Q"].numpy().astype(np.int64)
    X = c["X"].numpy().astype(np.int64)
    k = c["k"]
    D = ((Q[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    big = np.iinfo(np.int64).max
    if c["allowed"] is not None:
        D = np.where(c["allowed"], D, big)
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(D, order, axis=1)
    want_i = np.where(dist == big, -1, order)
    want_d = np.where(dist == big, np.inf, dist.astype(np.float64))
    got_d, got_i = kc.oracle(name)
    assert np.array_equal(got_i.numpy(), want_i)
    assert np.array_equal(got_d.numpy(), want_d)


@pytest.mark.parametrize("name", kc.EXACT_NAMES)
def test_exact_cases(name):
    d2, idx = kc.run(name, "cpu")
    kc.check_exact(d2, idx, name)


def test_identical_points_come_back_in_index_order():
    _, idx = kc.run("identical-300", "cpu")
    assert torch.equal(idx, torch.arange(64, dtype=torch.int32).expand(3, 64))


@pytest.mark.parametrize("name", kc.LABEL_NAMES)
def test_label_edge_queries(name):
    c = kc.case(name)
    d2, idx = kc.run(name, "cpu")
    assert (idx[0] == -1).all() and torch.isinf(d2[0]).all()
    if c["allowed"][1].sum() < c["k"]:
        m = int(c["allowed"][1].sum())
        assert (idx[1, :m] >= 0).all() and (idx[1, m:] == -1).all()
        assert torch.isinf(d2[1, m:]).all()
    free_d, free_i = kc.run(name, "cpu", labels=False)
    assert torch.equal(idx[2], free_i[2]) and torch.equal(d2[2], free_d[2])


@pytest.mark.parametrize("name", kc.FLOAT_NAMES)
def test_float_cases_within_bound(name):
    d2, idx = kc.run(name, "cpu")
    worst = kc.check_float(d2, idx, name)
    print(f"{name}: worst share of the bound {worst:.3f}")


@pytest.mark.parametrize("L", (1, 32, 33, 64, 65, 200))
def test_label_bitsets_against_isin(L):
    rng = np.random.default_rng(L)
    uniq = np.unique(rng.choice(10 * L + 5, size=L, replace=False))
    unknown = int(uniq.max()) + 7
    conds = [int(uniq[0]), int(uniq[-1]), [], [unknown],
             [int(uniq[-1]), unknown], list(uniq), tuple(uniq[::2]),
             set(uniq[::3].tolist()), uniq[: max(1, L // 2)], unknown]
    conds += [rng.choice(uniq, size=rng.integers(1, L + 1),
                         replace=False).tolist() for _ in range(8)]
    conds_arr = np.empty(len(conds), dtype=object)
    conds_arr[:] = conds
    bits = label_bitsets(uniq, conds_arr)
    W = max(1, (L + 31) // 32)
    assert bits.dtype == np.int32 and bits.shape == (len(conds), W)
    words = bits.view(np.uint32)
    j = np.arange(32 * W)
    got = ((words[:, j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(bool)
    for i, c in enumerate(conds):
        allowed = list(c) if isinstance(c, (list, tuple, set, np.ndarray)) \
            else [c]
        assert np.array_equal(got[i, :L], np.isin(uniq, allowed))
        assert not got[i, L:].any()


def test_label_bitsets_with_string_labels():
    uniq = np.unique(np.array(["b", "a", "c"]))
    conds = np.empty(3, dtype=object)
    conds[:] = ["a", ["c", "zz"], ["a", "b", "c"]]
    assert label_bitsets(uniq, conds).tolist() == [[1], [4], [7]]


def _valid():
    Q = torch.zeros(4, 3)
    X = torch.zeros(10, 3)
    return dict(Q=Q, X=X, xsq=torch.zeros(10), k=2,
                label_ids=torch.zeros(10, dtype=torch.int32),
                allow_bits=torch.ones(4, 1, dtype=torch.int32), splits=0)


class _Huge:
    """Stands in for a 2^31-row index: only what the validation reads."""
    dtype = torch.float32
    device = torch.device("cpu")
    shape = (1 << 31, 3)

    def is_contiguous(self):
        return True

    def dim(self):
        return 2


@pytest.mark.parametrize("change", [
    dict(Q=torch.zeros(4, 3, dtype=torch.float64)),
    dict(X=torch.zeros(10, 3, dtype=torch.float16)),
    dict(xsq=torch.zeros(10, dtype=torch.float64)),
    dict(Q=torch.zeros(3, 4).t()),
    dict(X=torch.zeros(10, 6)[:, ::2]),
    dict(Q=torch.zeros(4, 5)),
    dict(Q=torch.zeros(12)),
    dict(xsq=torch.zeros(9)),
    dict(k=0),
    dict(k=backend.KNN_MAX_K + 1),
    dict(splits=-1),
    dict(splits=backend.KNN_MAX_SPLITS + 1),
    dict(label_ids=None),
    dict(allow_bits=None),
    dict(label_ids=torch.zeros(10, dtype=torch.int64)),
    dict(allow_bits=torch.ones(4, 1, dtype=torch.int64)),
    dict(label_ids=torch.zeros(9, dtype=torch.int32)),
    dict(allow_bits=torch.ones(3, 1, dtype=torch.int32)),
    dict(allow_bits=torch.ones(4, 0, dtype=torch.int32)),
    dict(label_ids=torch.full((10,), 32, dtype=torch.int32)),
    dict(label_ids=torch.full((10,), -1, dtype=torch.int32)),
    dict(X=_Huge(), xsq=torch.zeros(1), label_ids=None, allow_bits=None),
], ids=lambda c: "-".join(c))
def test_validation_raises_value_error(change):
    args = dict(_valid(), **change)
    with pytest.raises(ValueError, match="knn_topk"):
        backend.knn_topk(**args)


def test_valid_inputs_pass_and_label_32w_minus_1_is_accepted():
    args = _valid()
    args["label_ids"] = torch.full((10,), 31, dtype=torch.int32)
    args["allow_bits"] = torch.full((4, 1), -(1 << 31), dtype=torch.int32)
    d2, idx = backend.knn_topk(**args)
    assert idx.tolist() == [[0, 1]] * 4 and (d2 == 0).all()
