"""cpu_ref.split_scan against the float64 oracle of split_scan_cases, on
every case of both families, with the case builders' margin assertions and
the measurement behind the Family B tolerance.  Runs without a GPU."""
import numpy as np
import pytest

from mmlspark_amd.ops import cpu_ref

from . import split_scan_cases as sc


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_case_margins_hold(name):
    sc.check_margins(name)


@pytest.mark.parametrize("name", sc.A_NAMES)
def test_cpu_ref_is_exact_on_family_a(name):
    out = sc.run(cpu_ref.split_scan, name)
    sc.check_result(out, name, *sc.tolerances(name))


def test_family_b_tolerance_is_the_measured_one():
    """The recorded constants are what cpu_ref shows on these cases: not
    exceeded, and not padded beyond a factor of two."""
    worst_g = worst_p = 0.0
    for name in sc.B_NAMES:
        out = sc.run(cpu_ref.split_scan, name)
        g, p = sc.check_result(out, name, sc.B_GAIN_MEASURED,
                               sc.B_PREFIX_MEASURED)
        worst_g, worst_p = max(worst_g, g), max(worst_p, p)
    print("measured gain %.4g prefix %.4g" % (worst_g, worst_p))
    assert 0.5 * sc.B_GAIN_MEASURED <= worst_g <= sc.B_GAIN_MEASURED
    assert 0.5 * sc.B_PREFIX_MEASURED <= worst_p <= sc.B_PREFIX_MEASURED
    assert sc.B_GAIN_BOUND == 4 * sc.B_GAIN_MEASURED
    assert sc.B_PREFIX_BOUND == 4 * sc.B_PREFIX_MEASURED


def test_family_b_is_mostly_empty_bins():
    for name in sc.B_NAMES:
        empty = (sc.cases()[name]["hists"][..., 2] == 0).mean()
        assert 0.6 < empty < 0.8, (name, empty)


def test_designed_properties_of_the_cases():
    """What each trap is meant to be, checked on the oracle's tables."""
    o = sc.expected("last_bin")
    assert o["best"][0][0] < 0            # "everything left" would give 0
    o = sc.expected("one_bin_min_data_0")
    assert o["best"][0][0] < 0            # a degenerate feature's 0 would win
    assert np.all(o["gain"][0, [0, 1, 3]] == sc.NEG_INF)
    o = sc.expected("l1_everywhere")
    assert o["best"][0][0] == 0.0 and np.all(o["scale"] == 0.0)
    o = sc.expected("l1_one_side")
    _, f, b = o["best"][0]
    assert abs(o["prefix"][0, f, b, 0]) < sc.cases()["l1_one_side"]["l1"]
    # pad and masked features hold the histograms that would win by far
    for name in ("mask_f0", "nf_real_1", "nf_real_pad_minus_3"):
        c = sc.cases()[name]
        free = sc.oracle(c["hists"], c["l1"], c["l2"], c["min_data"],
                         c["min_hess"], c["hists"].shape[1], None)
        assert free["best"][0][0] >= 4 * sc.expected(name)["best"][0][0]
    # the tied runs straddle the halving boundaries of the block arg-max
    g = sc.expected("runs_mid")["gain"]
    for hi, f, lo, hi_bin in ((0, 1, 127, 128), (1, 2, 63, 64),
                              (2, 3, 31, 32)):
        assert g[hi, f, lo] == g[hi, f, hi_bin] == g[hi].max()


def test_one_occupied_bin_never_splits_in_cpu_ref():
    """The reference used to answer gain 0 at bin 0 for a feature with one
    occupied bin when min_data <= 0; the kernel answers -inf."""
    import torch
    h = torch.zeros(1, 2, 8, 3)
    h[0, 0, 3] = torch.tensor([5.0, 2.0, 7.0])
    h[0, 1, 0] = torch.tensor([-5.0, 2.0, 7.0])
    out = cpu_ref.split_scan(h, 8, 0.0, 0.0, 0.0, 0.0, 0.0, 2)
    assert out[0, 0] == sc.NEG_INF
