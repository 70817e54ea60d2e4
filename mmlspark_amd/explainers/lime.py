"""LIME explainers (LIMEBase.scala:49; TabularLIME:17, VectorLIME, ImageLIME,
TextLIME + the legacy Superpixel transformer of core/.../lime/).

Per row: Bernoulli on/off states → perturbed samples → batched scoring →
kernel-weighted lasso per target class (kernel weight
sqrt(exp(-(d/width)^2)), LIMEBase.scala:55-65; per-row lasso :96-113).
Output per row: (n_classes, m) coefficient matrix.
With fusedSampling=True, TabularLIME and VectorLIME send each chunk's states
and drawn background rows to the model's score_coalitions (GBDT models: one
fused forest kernel, no perturbed samples) and fit the lasso on its output;
ImageLIME segments uint8 images and builds the masked model input on the GPU
(explainers/base.py), and SuperpixelTransformer(device="cuda") segments a
whole column in batched launches.
With fusedFit=True the four LIME stages pack a chunk's states, send them with
the scores to the model's device and fit every row's and class's surrogate in
one float64 kernel launch (ops/backend.py::lime_fit) instead of one host
lasso each; the random draws and everything before the fit are unchanged."""
from __future__ import annotations

import numpy as np
import pandas as pd
import torch

from ..core.param import (Param, toBool, toFloat, toInt, toList,
                          toString)
from ..core.registry import register
from ..core.schema import matrix_to_vector_column, vector_column_to_matrix
from .base import LocalExplainer
from .regression import lasso_regression
from .sampler import (ImageSampler, TextSampler, VectorSampler,
                      lime_sample_states, slic_superpixels)


class LIMEBase(LocalExplainer):
    kernelWidth = Param("kernelWidth", "RBF kernel width on state distance",
                        0.75, toFloat)
    regularization = Param("regularization", "lasso alpha", 0.0, toFloat)
    fusedFit = Param("fusedFit", "fit every surrogate of a chunk (rowBatch "
                     "rows, or one image or text) in one float64 kernel "
                     "launch on the model's GPU instead of one host lasso "
                     "per row and class (more than 512 features or 8 target "
                     "classes take the host fit; without a GPU the same "
                     "float64 fit runs on the CPU)", False, toBool)

    def _default_samples(self, m):
        return 1000

    def _weights(self, states: np.ndarray) -> np.ndarray:
        d = np.sqrt(((1.0 - states) ** 2).sum(axis=1)) / max(states.shape[1], 1) ** 0.5
        w = np.exp(-(d / self.get("kernelWidth")) ** 2)
        return np.sqrt(w)

    def _fit_states(self, states, scores, r2_out=None):
        """Weighted lasso per class; optionally records the weighted R² of
        the local surrogate (the reference's metricsCol output,
        LIMEBase.scala r2 column)."""
        w = self._weights(states)
        coefs = []
        r2s = []
        Xs = torch.from_numpy(states.astype(np.float64))
        wt = torch.from_numpy(w)
        for k in range(scores.shape[1]):
            yv = torch.from_numpy(scores[:, k].astype(np.float64))
            res = lasso_regression(Xs, yv, alpha=self.get("regularization"),
                                   sample_weight=wt)
            coefs.append(res.coefficients.numpy())
            if r2_out is not None:
                r2s.append(float(res.r_squared))
        if r2_out is not None:
            r2_out.append(np.asarray(r2s))
        return np.stack(coefs)  # (n_classes, m)

    def _fit_chunk(self, states_l, scores, r2_out):
        """_fit_states of every row of a chunk: states_l holds one (n, m)
        state matrix per row, scores their scores back to back.  With
        fusedFit the chunk is one backend.lime_fit call on the model's
        device."""
        from ..ops import backend
        from ..utils.devices import default_device
        R = len(states_l)
        n, m = states_l[0].shape if R else (0, 0)
        if not (self.get("fusedFit") and n >= 1
                and 1 <= m <= backend.LIME_FIT_MAX_FEATURES
                and 1 <= scores.shape[1] <= backend.LIME_FIT_MAX_OUTPUTS):
            return [self._fit_states(st, scores[i * n:(i + 1) * n],
                                     r2_out=r2_out)
                    for i, st in enumerate(states_l)]
        model = self.get("model")
        dev = default_device(model.get("device")
                             if "device" in model.params() else "auto")
        if dev.type == "cuda" and not torch.cuda.is_available():
            dev = torch.device("cpu")
        bits = torch.stack([backend.pack_states(st) for st in states_l])
        y = torch.from_numpy(np.ascontiguousarray(
            scores, dtype=np.float64).reshape(R, n, -1))
        coef, _, r2, _ = backend.lime_fit(
            bits.to(dev), m, y.to(dev), self.get("kernelWidth"),
            self.get("regularization"))
        r2_out.extend(r2.cpu().numpy())
        return list(coef.cpu().numpy())

    def _fused_chunk_scores(self, model, bg_dev, chunk, bg, states_l, rng,
                            score_samples):
        """Scores of the chunk's samples, (len(chunk) * n_samp, C), from the
        model's fused coalition kernel.  rng is consumed as the sample path
        does: the states are drawn already, now one draw of background rows
        per explained row.  bg_dev is the model's device copy of bg, made
        once per transform.  If the model declines, the same draws feed
        score_samples."""
        n = states_l[0].shape[0]
        draws = [self._draw_background(rng, len(bg), n, 1) for _ in chunk]
        v = model.score_coalitions(
            chunk, bg_dev, np.stack(states_l), np.stack(draws), 1,
            self.get("targetCol"), self.get("targetClasses"))
        if v is not None:
            return v
        return score_samples(np.concatenate(
            [st * x[None, :] + (1 - st) * bg[d]
             for x, st, d in zip(chunk, states_l, draws)]))


@register
class TabularLIME(LIMEBase):
    inputCols = Param("inputCols", "feature columns", None, toList)
    backgroundData = Param("backgroundData", "background DataFrame", None,
                           is_complex=True)

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        cols = self.get("inputCols")
        m = len(cols)
        bg = self.get("backgroundData")[cols].to_numpy(dtype=np.float64)
        rng = np.random.default_rng(self.get("seed"))
        n_samp = self.get("numSamples") or self._default_samples(m)
        explanations = []
        r2s = []
        rows = df[cols].to_numpy(dtype=np.float64)
        batch = self.get("rowBatch")
        fused, bg_dev = self._fused_model(bg)
        for s0 in range(0, len(rows), batch):
            chunk = rows[s0:s0 + batch]
            states_l = [lime_sample_states(m, n_samp, rng) for _ in chunk]
            if fused is not None:
                scores = self._fused_chunk_scores(
                    fused, bg_dev, chunk, bg, states_l, rng,
                    lambda p: self._score_matrix(p, cols))
                perts = states_l   # one score per state, as one per sample
            else:
                perts = [VectorSampler(bg, rng).apply(x, st)
                         for x, st in zip(chunk, states_l)]
                # one scoring fan-out for the whole chunk
                scores = self._score_matrix(np.concatenate(perts), cols)                 if perts else np.zeros((0, 1))
            explanations.extend(self._fit_chunk(states_l, scores, r2s))
        out = df.copy()
        out[self.get("outputCol")] = explanations
        if self.get("metricsCol"):
            out[self.get("metricsCol")] = r2s
        return out


@register
class VectorLIME(LIMEBase):
    featuresCol = Param("featuresCol", "dense vector column", "features")
    backgroundData = Param("backgroundData", "background DataFrame", None,
                           is_complex=True)

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        fcol = self.get("featuresCol")
        bg = vector_column_to_matrix(self.get("backgroundData"), fcol)
        bg = bg.astype(np.float64)
        m = bg.shape[1]
        rng = np.random.default_rng(self.get("seed"))
        n_samp = self.get("numSamples") or self._default_samples(m)
        rows = vector_column_to_matrix(df, fcol).astype(np.float64)
        explanations = []
        r2s = []
        batch = self.get("rowBatch")
        fused, bg_dev = self._fused_model(bg)
        for s0 in range(0, len(rows), batch):
            chunk = rows[s0:s0 + batch]
            states_l = [lime_sample_states(m, n_samp, rng) for _ in chunk]
            if fused is not None:
                scores = self._fused_chunk_scores(
                    fused, bg_dev, chunk, bg, states_l, rng,
                    lambda p: self._score_matrix(p.astype(np.float32)))
                perts = states_l   # one score per state, as one per sample
            else:
                perts = [VectorSampler(bg, rng).apply(x, st).astype(np.float32)
                         for x, st in zip(chunk, states_l)]
                scores = self._score_matrix(np.concatenate(perts))                 if perts else np.zeros((0, 1))
            explanations.extend(self._fit_chunk(states_l, scores, r2s))
        out = df.copy()
        out[self.get("outputCol")] = explanations
        if self.get("metricsCol"):
            out[self.get("metricsCol")] = r2s
        return out


@register
class TextLIME(LIMEBase):
    inputCol = Param("inputCol", "text column", "text")
    tokensCol = Param("tokensCol", "output tokens column", "tokens")

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        rng = np.random.default_rng(self.get("seed"))
        explanations, tokens_col, r2s = [], [], []
        for _, row in df.iterrows():
            tokens = str(row[self.get("inputCol")]).split()
            tokens_col.append(tokens)
            m = max(len(tokens), 1)
            n_samp = self.get("numSamples") or self._default_samples(m)
            states = lime_sample_states(m, n_samp, rng)
            texts = TextSampler(tokens).apply(states)
            scores = self._score_samples(
                pd.DataFrame({self.get("inputCol"): texts}))
            explanations.extend(self._fit_chunk([states], scores, r2s))
        out = df.copy()
        out[self.get("outputCol")] = explanations
        if self.get("metricsCol"):
            out[self.get("metricsCol")] = r2s
        out[self.get("tokensCol")] = tokens_col
        return out


@register
class ImageLIME(LIMEBase):
    inputCol = Param("inputCol", "image column", "image")
    cellSize = Param("cellSize", "superpixel cell size", 16, toInt)
    modifier = Param("modifier", "superpixel color weight", 10.0, toFloat)
    superpixelCol = Param("superpixelCol", "segment map column", "superpixels")

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        rng = np.random.default_rng(self.get("seed"))
        explanations, segs_col, r2s = [], [], []
        for _, row in df.iterrows():
            img = np.asarray(row[self.get("inputCol")])
            fused = self._fused_image_model(img)
            if fused is not None:
                dev_img, seg = self._device_segments(fused, img)
                segments = seg.cpu().numpy().astype(np.int64)
            else:
                segments = slic_superpixels(img, self.get("cellSize"),
                                            self.get("modifier"))
            segs_col.append(segments)
            m = int(segments.max()) + 1
            n_samp = self.get("numSamples") or min(self._default_samples(m), 512)
            states = lime_sample_states(m, n_samp, rng)
            if fused is not None:
                scores = self._masked_image_scores(fused, dev_img, seg, m,
                                                   states)
            else:
                imgs = ImageSampler(img, segments).apply(states)
                scores = self._score_samples(
                    pd.DataFrame({self.get("inputCol"): imgs}))
            explanations.extend(self._fit_chunk([states], scores, r2s))
        out = df.copy()
        out[self.get("outputCol")] = explanations
        if self.get("metricsCol"):
            out[self.get("metricsCol")] = r2s
        out[self.get("superpixelCol")] = segs_col
        return out


@register
class SuperpixelTransformer(LIMEBase):
    """Standalone superpixel segmentation (lime/SuperpixelTransformer.scala)."""
    inputCol = Param("inputCol", "image column", "image")
    outputCol = Param("outputCol", "segment map column", "superpixels")
    cellSize = Param("cellSize", "superpixel cell size", 16, toInt)
    modifier = Param("modifier", "superpixel color weight", 10.0, toFloat)
    nIter = Param("nIter", "k-means iterations", 5, toInt)
    device = Param("device", "cpu|cuda|auto: on a GPU the uint8 images of "
                   "the column are segmented together in batched kernel "
                   "launches", "cpu", toString)

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        from ..ops import backend
        from ..utils.devices import default_device
        cell, mod, n_iter = (self.get("cellSize"), self.get("modifier"),
                             self.get("nIter"))
        imgs = [np.asarray(v) for v in df[self.get("inputCol")].to_numpy()]
        segs = [None] * len(imgs)
        device = default_device(self.get("device"))
        if device.type == "cuda":
            # one upload and one set of launches for every image the kernels
            # take; the rest keep the numpy function
            on = [i for i, a in enumerate(imgs)
                  if a.dtype == np.uint8
                  and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] in (1, 3)))
                  and max(a.shape[:2]) <= backend.SLIC_MAX_DIM
                  and 1 <= backend.slic_num_centers(
                      a.shape[0], a.shape[1], cell) <= backend.SLIC_MAX_K]
            if on:
                flat = torch.from_numpy(np.concatenate(
                    [imgs[i].reshape(-1) for i in on])).to(device)
                views = [v.view(imgs[i].shape) for v, i in zip(
                    flat.split([imgs[i].size for i in on]), on)]
                labels, _ = backend.slic_segment(views, cell, mod, n_iter)
                sizes = [v.numel() for v in labels]
                host = torch.cat([v.reshape(-1) for v in labels]).cpu() \
                    .numpy().astype(np.int64)
                for i, v in zip(on, np.split(host, np.cumsum(sizes)[:-1])):
                    segs[i] = v.reshape(imgs[i].shape[:2])
        out = df.copy()
        out[self.get("outputCol")] = [
            slic_superpixels(a, cell, mod, n_iter) if s is None else s
            for a, s in zip(imgs, segs)]
        return out
