"""lime_fit_k on MI355X against lime_fit_cases: the sweep counts of the
float64 reference, coefficients, intercepts and r2 inside the yardstick (how
far the host's lasso_regression is from that reference), constant columns
exactly 0; and the LIME stages with fusedFit on the GPU against the CPU
definition."""
import numpy as np
import pytest

from mmlspark_amd.explainers.lime import TabularLIME, VectorLIME

from . import lime_fit_cases as lc
from .explain_cases import trained

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("idx", range(len(lc.CASES)),
                         ids=lambda i: str(lc.CASES[i][:4]))
def test_lime_fit_kernel(idx):
    lc.check(idx, "cuda")


@pytest.mark.parametrize("cls", [TabularLIME, VectorLIME])
def test_fused_fit_stage(cls, monkeypatch):
    model, df, cols = trained("cuda", True)
    kw = dict(model=model, targetCol="probability", targetClasses=[0, 1],
              numSamples=200, seed=3, backgroundData=df.head(40), rowBatch=3,
              **(dict(inputCols=cols) if cls is TabularLIME else {}))
    rows = df.iloc[40:48]

    def run(fused):
        out = cls(fusedFit=fused, **kw).transform(rows)
        return (np.stack(out["explanation"].to_numpy()),
                np.stack(out["r2"].to_numpy()))

    gpu = run(True)
    monkeypatch.setenv("MMLSPARK_AMD_LIME_FUSED", "0")
    ref = run(True)
    off = run(False)
    bound = lc.max_yardstick()
    for g, r, o in zip(gpu, ref, off):
        assert g.shape == r.shape == o.shape
        assert np.abs(g - r).max() <= bound
    assert gpu[0].shape == (8, 2, 6)
