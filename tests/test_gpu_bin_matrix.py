"""bin_matrix_k on MI355X against the per-element oracle of
bin_matrix_cases: the whole (ngroups, n, 4) tensor, pad lanes included, on
every case; a run long enough for the grid-stride loop's second pass; the
agreement of the binning rule with the device scorer's routing; and the
binding's argument checks."""
import numpy as np
import pytest
import torch

from mmlspark_amd.ops import backend

from . import bin_matrix_cases as bc
from .csr_predict_cases import flat

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")


@requires_gpu
@pytest.mark.parametrize("c", bc.CASES, ids=bc.case_id)
def test_bins_equal_the_oracle(c):
    X, ub, want = bc.case(c)
    Xd, ubd = bc.to_torch(X, ub, "cuda")
    out = backend.bin_matrix(Xd, ubd, c[1])
    assert out.is_cuda and out.dtype == torch.uint8
    assert tuple(out.shape) == want.shape
    assert np.array_equal(out.cpu().numpy(), want)


@requires_gpu
def test_grid_stride_second_pass():
    nf, nb, n = bc.STRIDE_CASE
    ub = bc.bounds(nf, nb)
    X = bc.data(ub, n)
    Xd, ubd = bc.to_torch(X, ub, "cuda")
    out = backend.bin_matrix(Xd, ubd, nb).cpu().numpy()
    want = bc.oracle(X, ub, nb)
    assert out.shape == want.shape == (1, n, 4)
    assert np.array_equal(out[:, -3:], want[:, -3:])      # the second pass
    assert np.array_equal(out, want)


@requires_gpu
@pytest.mark.parametrize("n_bins", [2, 16, 255, 256])
def test_binning_agrees_with_device_routing(n_bins):
    """Training routes a row by `bin <= b`, scoring by `x <= ub[f][b] ||
    isnan(x)`: the two agree for every bound index and every edge value."""
    X, ub, booster, where = bc.routing_case(n_bins)
    Xd, ubd = bc.to_torch(X, ub, "cuda")
    out = backend.bin_matrix(Xd, ubd, n_bins).cpu().numpy()
    assert np.array_equal(out, bc.oracle(X, ub, n_bins))
    nf = X.shape[1]
    bins = np.stack([out[f // 4, :, f % 4] for f in range(nf)], axis=1)
    f = flat(booster, "cuda")
    leaf = backend.predict_leaf(f["feature"], f["threshold"], f["left"],
                                f["right"], f["leaf_index"], f["offsets"], Xd)
    bc.check_routing(leaf.cpu().numpy(), bins.astype(np.int64), where)


# Every call below stops at an argument check of the binding: none reaches a
# kernel launch.
@requires_gpu
def test_bin_matrix_rejects_bad_arguments():
    X = torch.zeros(10, 3, device="cuda")

    def ub(nf=3, nb=15, dtype=torch.float32, device="cuda"):
        return torch.zeros(nf, nb, dtype=dtype, device=device)

    assert backend.bin_matrix(X, ub(), 16).shape == (1, 10, 4)
    ext = backend._require_ext()
    for args in ((X, ub(), 15), (X, ub(), 17),            # (nf, n_bins - 1)
                 (X, ub(2), 16), (X, ub(4), 16),
                 (X, ub(3, 256), 257),                    # bins are uint8
                 (X, ub(3, 0), 1),
                 (X, ub(dtype=torch.float64), 16),
                 (X, ub().reshape(-1), 16),
                 (X.double(), ub(), 16),
                 (X[0], ub(), 16),
                 (X, ub(3, 30)[:, ::2], 16)):
        with pytest.raises(RuntimeError):
            backend.bin_matrix(*args)
    for args in ((X, ub(device="cpu"), 16), (X.cpu(), ub(), 16)):
        with pytest.raises(RuntimeError):
            ext.bin_matrix(*args)
