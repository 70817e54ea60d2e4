"""backend.coalition_values on the CPU against the float64 reference of
explain_cases, its argument checks, and explain_cases' checks of the
explainers' fusedSampling path against the sample path it replaces."""
import numpy as np
import pytest
import torch

from mmlspark_amd.ops import backend

from . import explain_cases as ec


def transforms_of(name):
    return ("identity", "sigmoid" if ec.CASES[name][9] == 1 else "softmax")


@pytest.mark.parametrize("name", ec.CASES)
def test_cpu_path_equals_reference_exactly_or_within_bound(name):
    out = ec.run(name, "cpu", True)
    assert np.array_equal(out.numpy(), ec.reference(name, True)[0])
    for transform in transforms_of(name):
        ec.worst_share(ec.run(name, "cpu", False, transform), name, transform)


def _call(**change):
    c = ec.case("nf33-z1-r3-b3-t9-range", True)
    kw = dict(X=c["X"], bg=c["bg"], masks=c["masks"], bidx=c["bidx"], B=c["B"],
              classes=(0,))
    kw.update(change)
    return backend.coalition_values(
        *c["forest"], kw["X"], kw["bg"], kw["masks"], kw["bidx"], kw["B"],
        c["base"], 1, "identity", 1.0, kw["classes"])


@pytest.mark.parametrize("change", [
    dict(X=torch.zeros(3, 33, dtype=torch.float64)),            # dtype
    dict(X=torch.zeros(3, 66)[:, ::2]),                         # contiguity
    dict(X=torch.zeros(3, 33, device="meta")),                  # device
    dict(bg=torch.zeros(6, 32)),                                # shape
    dict(masks=torch.zeros(1, 1, 1, dtype=torch.int32)),        # W vs nf
    dict(masks=torch.zeros(2, 1, 2, dtype=torch.int32)),        # Rm not 1 or R
    dict(bidx=torch.full((3, 1, 3), 6, dtype=torch.int32)),     # bidx == nb
    dict(B=0, bidx=torch.zeros(3, 1, 0, dtype=torch.int32)),    # B < 1
    dict(classes=(1,)),                                         # class >= K
], ids=lambda c: "-".join(c))
def test_malformed_arguments_raise(change):
    _call()
    with pytest.raises(ValueError, match="coalition_values"):
        _call(**change)


@pytest.mark.parametrize("check", ec.CHECKS)
def test_fused_sampling_on_the_cpu(check, monkeypatch):
    check("cpu", monkeypatch)
