"""The torch CPU reference of the vw_*_interact kernels against the float64
oracle over the numpy expansion of vw_interact_cases, and fusedInteractions
on the CPU.  Runs without a GPU."""
import numpy as np
import pytest

from . import vw_interact_cases as ic
from . import vw_kernel_cases as cases
from .test_vw_oracle import check_case


def _backend():
    from mmlspark_amd.ops import backend
    return backend.vw_sgd_minibatch_interact, backend.vw_predict_interact


def check(shape, config, margin, device="cpu", **kw):
    spec, n_steps = ic.spec_for(shape, **kw)
    c, case = ic.make_case(shape, spec, config, n_steps)
    check_case(case, *ic.adaptors(c, *_backend(), device), margin, device)


@pytest.mark.parametrize("config", ic.CONFIGS, ids=cases.grid_id)
@pytest.mark.parametrize("shape", ic.ALL_SHAPES)
def test_reference_matches_oracle(shape, config):
    check(shape, config, cases.CPU_MARGIN)


def check_public_interface(device, margin):
    """fit == one oracle step over the expansion, transform == the oracle's
    scores, both within the kernels' floors; the materialised path scores
    the same table within the float32 summation bound of the two orders,
    (depth_fused + depth_flat) eps/2 sum|w x|, where a depth is the longest
    chain of additions plus one for the product: n for the CPU reference's
    sequential index_add, per-lane terms + 6 tree levels on the GPU."""
    from mmlspark_amd.models.vw.estimators import VowpalWabbitRegressor
    df, c = ic.frame()
    flat = ic.expand(c)
    kw = dict(numBits=c.bits, numPasses=1, batchSize=64, device=device)
    est = VowpalWabbitRegressor(args="-q ::", additionalFeatures=["b"],
                                fusedInteractions=True, **kw)
    model = est.fit(df)
    w, g = np.zeros(1 << c.bits), np.zeros(1 << c.bits)
    cases.oracle_step(flat, w, g, None, cases.f32(est.get("learningRate")),
                      0.0, 0.5, "squared", False)
    touched = flat.touched()
    assert np.count_nonzero(model.weights) == len(touched)
    floor = cases.FLOOR["exact"]
    assert cases.rel_err(model.weights[touched], w[touched]) \
        <= margin * floor["w"]
    got = model.transform(df)["prediction"].to_numpy()
    p, p_abs = cases.predict_oracle(flat, model.weights)
    assert cases.rel_err(got, p) <= margin * floor["preds"]
    model.set("fusedInteractions", False)
    n = np.diff(flat.off)
    depth = 2 * n if device == "cpu" else (
        ic.lane_terms(c) + 7 + -(-n // 64) + 7)
    err = np.abs(model.transform(df)["prediction"].to_numpy() - got)
    assert bool((err <= depth * 0.5 * cases.F32_EPS * p_abs).all())
    # a three-column spec takes the materialised path, parameter on or off
    three = [VowpalWabbitRegressor(
        interactions=[["features", "b", "c"]], additionalFeatures=["b", "c"],
        fusedInteractions=on, **kw).fit(df) for on in (True, False)]
    assert np.array_equal(three[0].weights, three[1].weights)
    assert np.array_equal(three[0].transform(df)["prediction"].to_numpy(),
                          three[1].transform(df)["prediction"].to_numpy())


def test_public_interface_cpu():
    check_public_interface("cpu", cases.CPU_MARGIN)
