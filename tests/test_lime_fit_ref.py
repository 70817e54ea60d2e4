"""cpu_ref.lime_fit, what CPU tensors get from backend.lime_fit, against the
float64 reference of lime_fit_cases on two small cases: equal sweep counts,
everything else inside the yardstick."""
import pytest

from . import lime_fit_cases as lc


@pytest.mark.parametrize("idx", [1, 4], ids=lambda i: str(lc.CASES[i][:4]))
def test_cpu_lime_fit(idx):
    lc.check(idx, "cpu")
