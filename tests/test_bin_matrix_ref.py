"""cpu_ref.bin_matrix against the per-element oracle of bin_matrix_cases,
and the agreement of the binning rule with the scorer's routing, on the CPU
reference.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from mmlspark_amd.ops import cpu_ref

from . import bin_matrix_cases as bc
from .csr_predict_cases import flat


@pytest.mark.parametrize("c", bc.CASES, ids=bc.case_id)
def test_cpu_ref_bins_equal_the_oracle(c):
    X, ub, want = bc.case(c)
    Xt, ubt = bc.to_torch(X, ub)
    out = cpu_ref.bin_matrix(Xt, ubt, c[1])
    assert out.dtype == torch.uint8 and tuple(out.shape) == want.shape
    assert np.array_equal(out.numpy(), want)


def test_cases_hold_the_edges():
    """Bounds themselves, both neighbours, signed zeros, infinities, NaN,
    subnormals and +-FLT_MAX are in the data; duplicate, all-inf, inf-padded
    and -inf-first bound rows are among the bounds."""
    ub = bc.bounds(5, 255)
    X = bc.all_values_data(ub)
    for f in range(5):
        col = X[:, f]
        finite = np.unique(ub[f][np.isfinite(ub[f])])
        assert np.isin(finite, col).all()
        with np.errstate(over="ignore"):
            assert np.isin(np.nextafter(finite, bc.INF), col).all()
            assert np.isin(np.nextafter(finite, -bc.INF), col).all()
        assert np.isnan(col).any() and np.isposinf(col).any()
        assert np.isneginf(col).any()
        assert (col == bc.FLT_MAX).any() and (col == -bc.FLT_MAX).any()
        assert ((col != 0) & (np.abs(col) < bc.TINY)).any()     # subnormal
        zeros = col[col == 0]
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
    assert (ub[0] == 0.0).any()
    assert (ub[1][1:] == ub[1][:-1]).any()                         # duplicates
    assert np.isposinf(ub[2][127:]).all() and np.isfinite(ub[2][0])
    assert np.isposinf(ub[3]).all()
    assert np.isneginf(ub[4][0])


def test_x_equal_to_a_bound_stays_in_the_bounds_bin():
    ub = np.array([[-1.0, 0.0, 2.0]], dtype=np.float32)
    X = np.array([[-1.0], [0.0], [-0.0], [2.0], [2.5], [np.nan]],
                 dtype=np.float32)
    assert bc.oracle_bins(X, ub, 4)[:, 0].tolist() == [0, 1, 1, 2, 3, 0]


@pytest.mark.parametrize("n_bins", [2, 16, 255, 256])
def test_binning_agrees_with_routing_on_the_cpu_reference(n_bins):
    X, ub, booster, where = bc.routing_case(n_bins)
    Xt, ubt = bc.to_torch(X, ub)
    out = cpu_ref.bin_matrix(Xt, ubt, n_bins).numpy()
    assert np.array_equal(out, bc.oracle(X, ub, n_bins))
    f = flat(booster)
    leaf = cpu_ref.predict_leaf(f["feature"], f["threshold"], f["left"],
                                f["right"], f["leaf_index"], f["offsets"], Xt)
    bc.check_routing(leaf.numpy(), bc.oracle_bins(X, ub, n_bins), where)
