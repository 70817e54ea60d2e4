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
same, in the same order, as with the parameter off.

The image explainers honour it for models that offer score_image_batch
(TorchModel, ImageFeaturizer) on a GPU: a uint8 image is segmented by the SLIC
kernels, the drawn states are bit-packed, and one kernel writes every masked
sample into the model's float32 NCHW input batch (ops/backend.py::
slic_segment, ::masked_image_batch).  The draws are again the same."""
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
                          "serve, take the sample path); image explainers: "
                          "segment uint8 images and write the masked samples "
                          "into the model's input batch on the GPU (models "
                          "without score_image_batch, models on the CPU, "
                          "other targets and other images take the sample "
                          "path)", False, toBool)

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

    def _fused_image_model(self, img: np.ndarray):
        """The model, if fusedSampling is on and the image explainers' device
        path can serve this image: the model scores ready batches
        (score_image_batch), targetCol is its output column, it runs on a GPU,
        the image is uint8 with 1 or 3 channels and its centre count and
        sides are within the kernels' limits.  Else None."""
        model = self.get("model")
        if not (self.get("fusedSampling")
                and hasattr(model, "score_image_batch")
                and "outputCol" in model.params()
                and self.get("targetCol") == model.get("outputCol")):
            return None
        from ..ops import backend
        from ..utils.devices import default_device
        if default_device(model.get("device")).type != "cuda" \
                or img.dtype != np.uint8 \
                or not (img.ndim == 2 or (img.ndim == 3
                                          and img.shape[2] in (1, 3))) \
                or max(img.shape[:2]) > backend.SLIC_MAX_DIM \
                or not 1 <= backend.slic_num_centers(
                    img.shape[0], img.shape[1],
                    self.get("cellSize")) <= backend.SLIC_MAX_K:
            return None
        return model

    def _device_segments(self, model, img: np.ndarray):
        """The image on the model's device and its superpixel map segmented
        there, (H, W) int32."""
        import torch
        from ..ops import backend
        from ..utils.devices import default_device
        dev_img = torch.from_numpy(np.ascontiguousarray(img)).to(
            default_device(model.get("device")))
        labels, _ = backend.slic_segment([dev_img], self.get("cellSize"),
                                         float(self.get("modifier")))
        return dev_img, labels[0]

    def _masked_image_scores(self, model, dev_img, seg, m, states):
        """_score_samples of ImageSampler(img, segments).apply(states): one
        kernel writes the samples into the model's input batch on the
        device, the model scores that batch."""
        from ..models.image_featurizer import _unit_lut
        from ..ops import backend
        batch = backend.masked_image_batch(
            dev_img, seg, backend.pack_states(states).to(dev_img.device), 0,
            model.image_input_size(dev_img.shape), _unit_lut(dev_img.device),
            m=m)
        return model.score_image_batch(batch)[:, self.get("targetClasses")]

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
