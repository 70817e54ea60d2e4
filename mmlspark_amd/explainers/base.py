"""LocalExplainer scaffold (core/.../explainers/LocalExplainer.scala:16).

The perturbation fan-out batches ALL samples for a chunk of rows into one
DataFrame and scores it with a single model.transform — on GPU this drives
the batched HIP scoring kernels (the reference instead exploded rows into
Spark and scored per-row UDFs).

With fusedSampling=True the vector and tabular explainers skip the fan-out
for models that offer score_coalitions (the GBDT family): the coalition
masks, the background table and the drawn background row indices go to the
device and one kernel selects each feature value while it walks the forest,
averaging over the background draws as it goes.  The random draws are the
same, in the same order, as with the parameter off."""
from __future__ import annotations


import numpy as np
import pandas as pd

from ..core.param import Param, toBool, toInt, toList
from ..core.pipeline import Transformer


class LocalExplainer(Transformer):
    model = Param("model", "the model Transformer to explain", None,
                  is_complex=True)
    targetCol = Param("targetCol", "model output column to explain",
                      "probability")
    targetClasses = Param("targetClasses", "class indices to explain", [1],
                          toList)
    outputCol = Param("outputCol", "explanation output column", "explanation")
    numSamples = Param("numSamples", "perturbations per row (default: "
                       "modality-specific)", None)
    metricsCol = Param("metricsCol", "fit-metric output column (r2)", "r2")
    seed = Param("seed", "sampling seed", 0, toInt)
    rowBatch = Param("rowBatch", "rows explained per scoring fan-out", 16, toInt)
    fusedSampling = Param("fusedSampling", "vector/tabular explainers: score "
                          "coalitions inside the model's forest kernel "
                          "instead of building the perturbed samples (models "
                          "without score_coalitions, and targets it cannot "
                          "serve, take the sample path)", False, toBool)

    def _score_samples(self, samples_df: pd.DataFrame) -> np.ndarray:
        """Run the inner model; return (n, n_target_classes) target values."""
        model = self.get("model")
        out = model.transform(samples_df)
        col = out[self.get("targetCol")].to_numpy()
        classes = self.get("targetClasses")
        if len(col) and isinstance(col[0], (np.ndarray, list)):
            mat = np.stack([np.asarray(v) for v in col])
            return mat[:, classes]
        return np.asarray(col, dtype=np.float64)[:, None]

    def _fused_model(self, bg):
        """(model, its device copy of the background bg) if fusedSampling is
        on and the model can score coalitions, else (None, None).  Called
        once per transform, so the background is uploaded once."""
        model = self.get("model")
        if self.get("fusedSampling") and hasattr(model, "score_coalitions"):
            return model, model.coalition_background(bg)
        return None, None

    def _draw_background(self, rng, nb, n, B):
        """VectorSampler.apply's background choice for n = nZ * B samples,
        consuming rng exactly as it does: None (cycle every background row
        once per coalition, nothing drawn) or n drawn row indices."""
        if B > 1 and B == nb and n % B == 0:
            return None
        return rng.integers(0, nb, size=n)

    def _score_matrix(self, X: np.ndarray, cols=None) -> np.ndarray:
        """Score a raw feature MATRIX.  Models exposing score_matrix (the
        GBDT models) skip the whole DataFrame round trip — the fan-out
        builds millions of object cells otherwise; generic transformers
        fall back to _score_samples."""
        model = self.get("model")
        if hasattr(model, "score_matrix"):
            v = model.score_matrix(X, self.get("targetCol"),
                                   self.get("targetClasses"))
            if v is not None:
                return v
        if cols is not None:
            return self._score_samples(pd.DataFrame(X, columns=list(cols)))
        from ..core.schema import matrix_to_vector_column
        fcol = model.get("featuresCol") if "featuresCol" in model.params() \
            else "features"
        return self._score_samples(pd.DataFrame({
            fcol: matrix_to_vector_column(X.astype(np.float32))}))
