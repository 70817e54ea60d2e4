"""vw_sgd_interact_k / vw_predict_interact_k on MI355X against the float64
oracle over the numpy expansion of vw_interact_cases, in-row collisions, the
empty batch and fusedInteractions end to end."""
import numpy as np
import pytest
import torch

from . import vw_interact_cases as ic
from . import vw_kernel_cases as cases
from .test_vw_interact_ref import _backend, check, check_public_interface

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU")]


@pytest.mark.parametrize("config", ic.CONFIGS, ids=cases.grid_id)
@pytest.mark.parametrize("shape", ic.ALL_SHAPES)
def test_kernel_matches_oracle(shape, config):
    from mmlspark_amd.ops import backend
    check(shape, config, cases.GPU_MARGIN[cases.family(config[0], config[2])],
          "cuda", window=backend.vw_interact_window())


def test_predict_with_in_row_collisions():
    """bits = 6: the generated features of an example share slots and stay
    separate terms.  A lane adds lane_terms products (one accumulator over
    the columns and pairs), then 6 tree levels: the error is within
    (lane_terms + 6 + 1) eps/2 of sum|w x|."""
    _, sizes, pairs, kw = ic.SHAPES["grid"]
    c = ic.build(7, sizes, pairs, bits=6, **kw)
    slot, x, off = ic.expand_arrays(c)
    assert len(np.unique(slot)) < len(slot)
    w = cases.warm_tables(8, 64)[0]
    t = w[slot].astype(np.float64) * x.astype(np.float64)
    got = _backend()[1](*c.tensors("cuda"), torch.from_numpy(w).cuda())
    assert got.shape == (len(sizes),) and got.dtype == torch.float32
    for ex, (a, b) in enumerate(zip(off[:-1], off[1:])):
        tol = (ic.lane_terms(c)[ex] + 7) * 0.5 * cases.F32_EPS * np.abs(
            t[a:b]).sum()
        assert abs(float(got[ex]) - t[a:b].sum()) <= tol, (ex, tol)


@pytest.mark.parametrize("invariant", [False, True])
def test_no_examples(invariant):
    sgd, predict = _backend()
    c = ic.build(1, np.zeros((0, 2), dtype=np.int64), [(0, 1)])
    w0, g0 = cases.warm_tables(42, 1 << c.bits)
    w, g = torch.from_numpy(w0).cuda(), torch.from_numpy(g0).cuda()
    s = torch.full_like(w, 0.5)
    y = torch.zeros(0, device="cuda")
    out = sgd(*c.tensors("cuda"), y, w, g, cases.LR, cases.L2, 0.5,
              "logistic", y, s, invariant)
    assert out.shape == (0,) and out.is_cuda
    assert predict(*c.tensors("cuda"), w).shape == (0,)
    assert np.array_equal(w.cpu().numpy().view(np.int32), w0.view(np.int32))
    assert np.array_equal(g.cpu().numpy().view(np.int32), g0.view(np.int32))
    assert bool((s == 0.5).all())


def test_public_interface_gpu():
    check_public_interface("cuda", cases.GPU_MARGIN["exact"])
