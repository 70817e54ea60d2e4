"""coalition_values_k + coalition_merge_k on MI355X against explain_cases: exact
cases bit for bit per tile size, float cases within bound, the explainers."""
import numpy as np
import pytest
import torch

from mmlspark_amd.ops import backend

from . import explain_cases as ec
from .test_explain_ref import transforms_of

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")


@requires_gpu
@pytest.mark.parametrize("name", ec.CASES)
def test_exact_cases_bit_for_bit_for_every_tile_and_repeatable(name):
    want = ec.reference(name, True)[0]
    for tile in ec.TILES:
        out = ec.run(name, "cuda", True, tile_nodes=tile)
        assert out.is_cuda and out.dtype == torch.float64
        assert np.array_equal(out.cpu().numpy(), want), tile
    assert torch.equal(out, ec.run(name, "cuda", True, tile_nodes=ec.TILES[-1]))


@requires_gpu
@pytest.mark.parametrize("name", ec.CASES)
def test_float_cases_within_bound_and_repeatable(name):
    for transform in transforms_of(name):
        for tile in ec.TILES[:2]:
            out = ec.run(name, "cuda", False, transform, tile_nodes=tile)
            worst = ec.worst_share(out, name, transform)
            print(f"{name} {transform} tile {tile}: worst share of the bound "
                  f"on gfx950 {worst:.3f}")
        again = ec.run(name, "cuda", False, transform, tile_nodes=tile)
        assert torch.equal(out, again)


@requires_gpu
def test_draws_split_over_segments_and_merged_in_order():
    """3 x 257 coalitions x 400 cycled draws: 134 segments of 3 draws (the
    last holds 1) per coalition; exact leaves, so it equals the CPU path."""
    c = ec.case("nf32-z257-r3-cycle5-t5-leaf-first", True)
    bg = torch.randn(400, 32, generator=torch.Generator().manual_seed(11))
    args = lambda dev: ([a.to(dev) for a in c["forest"]]
                        + [c["X"].to(dev), bg.to(dev), c["masks"].to(dev),
                           None, 400, c["base"].to(dev), 1])
    want = backend.coalition_values(*args("cpu"))
    out = backend.coalition_values(*args("cuda"))
    assert torch.equal(out.cpu(), want)
    assert torch.equal(out, backend.coalition_values(*args("cuda"), tile_nodes=4))


@requires_gpu
@pytest.mark.parametrize("check", ec.CHECKS)
def test_fused_sampling_on_the_gpu(check, monkeypatch):
    check("cuda", monkeypatch)
