"""KNN / ConditionalKNN — exact nearest-neighbor search, MI355X-first.

The reference broadcasts a ball tree and runs a bound-pruned DFS per row UDF
(core/.../nn/BallTree.scala:109, ConditionalKNN.scala:32-100).  On MI355X the
idiomatic design is brute-force tiled distance computation on the matrix
cores (torch matmul → rocBLAS MFMA GEMM: ||q-x||² = ||q||² - 2q·x + ||x||²)
+ device top-k, batched over queries — exact, and faster than tree traversal
on 8 TB/s HBM for the data sizes the reference targets.  ConditionalKNN
masks disallowed labels before the top-k (label-filtered search parity).

On a GPU with the HIP extension the search is two fused kernels
(ops/hip/knn_kernels.hip through backend.knn_topk): f32 MFMA distances with
the top-k kept in LDS, so no (queries, index) tile is ever written, ties
ordered by index, and per-query label bitsets of any width.  k above
backend.KNN_MAX_K, CPU and MMLSPARK_AMD_KNN_FUSED=0 keep the torch path."""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np
import pandas as pd
import torch

from ..core.param import Param, toInt
from ..core.pipeline import Estimator, Model
from ..core.registry import register
from ..core.schema import features_matrix
from ..utils.devices import default_device


class _KNNParamsMixin:
    featuresCol = Param("featuresCol", "query features column", "features")
    valuesCol = Param("valuesCol", "payload column carried to matches", "values")
    outputCol = Param("outputCol", "matches output column", "output")
    k = Param("k", "number of neighbors", 5, toInt)
    batchSize = Param("batchSize", "query rows per device batch", 4096, toInt)
    leafSize = Param("leafSize", "ball-tree leaf size (used only by the CPU "
                     "BallTree view, getBallTree(); the GPU path is exact "
                     "brute-force — KNN.scala leafSize)", 50, toInt)


@register
class KNN(_KNNParamsMixin, Estimator):
    """Fit = index the reference DataFrame (KNN.scala:48)."""

    def _fit(self, df: pd.DataFrame):
        X = features_matrix(df, self.get("featuresCol"), None)
        values = df[self.get("valuesCol")].tolist() \
            if self.get("valuesCol") in df.columns else list(range(len(df)))
        model = KNNModel(index=X, values=values)
        for p in ("featuresCol", "outputCol", "k", "batchSize", "leafSize"):
            model.set(p, self.get(p))
        return model


@register
class KNNModel(_KNNParamsMixin, Model):
    indexData = Param("indexData", "indexed matrix + payload", None,
                      is_complex=True)

    def getBallTree(self):
        """The reference's broadcast ball tree (BallTree.scala:109) over the
        same index; built lazily on the CPU.  Scoring here uses the exact
        brute-force MFMA path, so this exists for API/introspection parity
        and CPU-side traversal."""
        from .balltree import BallTree
        if getattr(self, "_ball_tree", None) is None:
            d = self.get("indexData")
            self._ball_tree = BallTree(d["index"], list(d["values"]),
                                       leaf_size=self.get("leafSize"))
        return self._ball_tree

    def __init__(self, index: Optional[np.ndarray] = None,
                 values: Optional[List] = None, labels=None, **kwargs):
        super().__init__(**kwargs)
        if index is not None:
            payload = {"index": np.ascontiguousarray(index, dtype=np.float32)}
            payload["values"] = np.asarray(values, dtype=object).astype(str) \
                if values is not None and not np.issubdtype(
                    np.asarray(values).dtype, np.number) \
                else np.asarray(values if values is not None else [])
            if labels is not None:
                payload["labels"] = np.asarray(labels)
            self.set("indexData", {k: v for k, v in payload.items()})

    def _index_on(self, device):
        """Device copy of the index and its squared row norms, uploaded once
        per (device, indexData array) and kept on the model like _ball_tree:
        not a Param, not serialised."""
        index = self.get("indexData")["index"]
        key = (str(device), id(index))
        cache = getattr(self, "_index_cache", None)
        if cache is None or cache[0] != key:
            X = torch.from_numpy(index).to(device)
            # holding `index` keeps its id from being reused while cached
            cache = (key, X, (X * X).sum(dim=1), {}, index)
            self._index_cache = cache
        return cache[1], cache[2]

    def _label_ids_on(self, device, label_ids: np.ndarray):
        """int32 device copy of the index's label ids, cached beside the
        index (the ids are a function of indexData['labels'])."""
        self._index_on(device)
        extra = self._index_cache[3]
        if "label_ids" not in extra:
            extra["label_ids"] = torch.from_numpy(
                np.ascontiguousarray(label_ids, dtype=np.int32)).to(device)
        return extra["label_ids"]

    def _use_fused(self, device=None) -> bool:
        """The fused HIP search serves GPU devices when the extension is
        loaded, k fits the kernel and MMLSPARK_AMD_KNN_FUSED is not 0."""
        from ..ops import backend
        device = default_device("auto") if device is None else device
        n = self.get("indexData")["index"].shape[0]
        return (device.type == "cuda" and backend.hip_available()
                and 1 <= min(self.get("k"), n) <= backend.KNN_MAX_K
                and os.environ.get("MMLSPARK_AMD_KNN_FUSED", "1") != "0")

    def _search_fused(self, Q: np.ndarray, device, label_ids, label_bits):
        """All queries through backend.knn_topk, a launch per 2^20 queries;
        no (n_q, n_index) tile and no batch clamp.  Returns what _search
        returns; a slot without a match has index -1 and distance inf."""
        from ..ops import backend
        X, xsq = self._index_on(device)
        k = min(self.get("k"), X.shape[0])
        lid = (self._label_ids_on(device, label_ids)
               if label_bits is not None else None)
        all_idx, all_dist = [], []
        step = 1 << 20
        for s in range(0, len(Q), step):
            q = torch.from_numpy(np.ascontiguousarray(
                Q[s:s + step], dtype=np.float32)).to(device)
            bits = (torch.from_numpy(np.ascontiguousarray(
                label_bits[s:s + step])).to(device)
                    if label_bits is not None else None)
            d2, idx = backend.knn_topk(q, X, xsq, k, lid, bits)
            all_idx.append(idx.cpu().numpy().astype(np.int64))
            all_dist.append(d2.clamp_min(0).sqrt().cpu().numpy())
        return np.concatenate(all_idx), np.concatenate(all_dist)

    def _search(self, Q: np.ndarray, cond_masks=None, cond_bits=None,
                label_ids=None, label_bits=None):
        """Nearest neighbours of every query: (idx (n_q, k), dist (n_q, k)).

        On a GPU with the HIP extension the fused kernels run (see
        _use_fused); conditioning is then `label_bits`, (n_q, W) int32
        bitsets over `label_ids`, for any number of labels.

        Otherwise: tiled MFMA-GEMM distances + device top-k.
        Conditioning: either host bool masks (small corpora), or — the
        large-corpus path — per-query uint64 label bitmasks tested on
        device against the index's label-id vector, so no (n_q, n_index)
        host matrix ever exists."""
        device = default_device("auto")
        if cond_masks is None and cond_bits is None \
                and self._use_fused(device):
            return self._search_fused(Q, device, label_ids, label_bits)
        X, xsq = self._index_on(device)
        k = min(self.get("k"), X.shape[0])
        # memory-aware batch clamp: the (bs, n) distance tile (plus the
        # transient mask tile) must stay bounded as the corpus grows
        bs = min(self.get("batchSize"),
                 max(128, int((1 << 31) / max(1, X.shape[0]))))
        lid = (torch.from_numpy(label_ids).to(device)
               if label_ids is not None else None)
        all_idx, all_dist = [], []
        for s in range(0, len(Q), bs):
            q = torch.from_numpy(Q[s:s + bs]).to(device)
            d2 = (q * q).sum(1, keepdim=True) - 2.0 * (q @ X.t()) + xsq
            if cond_bits is not None:
                bits = torch.from_numpy(cond_bits[s:s + bs]).to(device)
                allowed = ((bits.unsqueeze(1) >> lid.unsqueeze(0)) & 1).bool()
                d2 = torch.where(allowed, d2,
                                 torch.full_like(d2, float("inf")))
            elif cond_masks is not None:
                m = torch.from_numpy(cond_masks[s:s + bs]).to(device)
                d2 = torch.where(m, d2, torch.full_like(d2, float("inf")))
            dist, idx = torch.topk(d2, k, dim=1, largest=False)
            all_idx.append(idx.cpu().numpy())
            all_dist.append(dist.clamp_min(0).sqrt().cpu().numpy())
        return np.concatenate(all_idx), np.concatenate(all_dist)

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        Q = features_matrix(df, self.get("featuresCol"), None)
        data = self.get("indexData")
        vals = data.get("values")
        idx, dist = self._search(Q) if len(df) else (np.zeros((0, 0), int),
                                                     np.zeros((0, 0)))
        has_vals = len(vals) > 0
        matches = [
            [{"value": (vals[j].item() if hasattr(vals[j], "item")
                        else vals[j]) if has_vals else j,
              "distance": d}
             for j, d in zip(ir, dr)]
            for ir, dr in zip(idx.tolist(), dist.tolist())]
        out = df.copy()
        out[self.get("outputCol")] = matches
        return out


def label_bitsets(uniq, conds) -> np.ndarray:
    """Allowed-label bitsets for the fused search: (len(conds), W) int32 with
    W = max(1, ceil(len(uniq) / 32)).  Bit (j & 31) of word (j >> 5) of row i
    is set when conditioner i allows uniq[j]; a conditioner is one value or
    a list/tuple/set/array of them, and values not in `uniq` are ignored.
    The words are unsigned bit patterns stored as int32 (bit 31 is a label
    like any other)."""
    uniq = np.asarray(uniq)
    W = max(1, (len(uniq) + 31) // 32)
    pos = {v: i for i, v in enumerate(uniq.tolist())}
    bits = np.zeros((len(conds), W), dtype=np.uint32)
    for i, c in enumerate(conds):
        allowed = (c if isinstance(c, (list, tuple, set, np.ndarray))
                   else [c])
        for v in allowed:
            j = pos.get(v.item() if isinstance(v, np.generic) else v)
            if j is not None:
                bits[i, j >> 5] |= np.uint32(1 << (j & 31))
    return bits.view(np.int32)


@register
class ConditionalKNN(_KNNParamsMixin, Estimator):
    """Label-conditioned KNN (ConditionalKNN.scala:32): each query carries a
    set of allowed labels; only index points with those labels match."""
    labelCol = Param("labelCol", "index label column", "labels")
    conditionerCol = Param("conditionerCol", "query allowed-label-set column",
                           "conditioner")

    def _fit(self, df: pd.DataFrame):
        X = features_matrix(df, self.get("featuresCol"), None)
        values = df[self.get("valuesCol")].tolist() \
            if self.get("valuesCol") in df.columns else list(range(len(df)))
        labels = df[self.get("labelCol")].to_numpy()
        model = ConditionalKNNModel(index=X, values=values, labels=labels)
        for p in ("featuresCol", "outputCol", "k", "batchSize",
                  "conditionerCol"):
            model.set(p, self.get(p))
        return model


@register
class ConditionalKNNModel(KNNModel):
    conditionerCol = Param("conditionerCol", "query allowed-label-set column",
                           "conditioner")

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        Q = features_matrix(df, self.get("featuresCol"), None)
        data = self.get("indexData")
        labels = data["labels"]
        vals = data.get("values")
        conds = df[self.get("conditionerCol")].to_numpy()
        uniq, label_ids = np.unique(labels, return_inverse=True)
        if len(df) == 0:
            idx, dist = np.zeros((0, 0), int), np.zeros((0, 0))
        elif self._use_fused():
            # any number of labels: (n_q, W) bitsets tested in the kernel
            idx, dist = self._search(Q, label_ids=label_ids,
                                     label_bits=label_bitsets(uniq, conds))
        elif len(uniq) <= 64:
            # large-corpus path: per-query uint64 allowed-label bitmask,
            # tested on device — no (n_q, n_index) host matrix
            pos = {v: i for i, v in enumerate(uniq)}
            bits = np.zeros(len(df), dtype=np.int64)
            for i, c in enumerate(conds):
                allowed = (c if isinstance(c, (list, tuple, set, np.ndarray))
                           else [c])
                b = 0
                for v in allowed:
                    j = pos.get(v)
                    if j is not None:
                        b |= (1 << j)
                bits[i] = b
            idx, dist = self._search(Q, cond_bits=bits,
                                     label_ids=label_ids.astype(np.int64))
        else:
            masks = np.zeros((len(df), len(labels)), dtype=bool)
            for i, c in enumerate(conds):
                allowed = set(c) if isinstance(
                    c, (list, tuple, set, np.ndarray)) else {c}
                masks[i] = np.isin(labels, list(allowed))
            idx, dist = self._search(Q, masks)
        matches = []
        for i in range(len(df)):
            row = []
            for c, j in enumerate(idx[i]):
                if np.isfinite(dist[i, c]):
                    row.append({
                        "value": (vals[j].item() if hasattr(vals[j], "item")
                                  else vals[j]) if len(vals) else int(j),
                        "distance": float(dist[i, c]),
                        "label": labels[j].item() if hasattr(labels[j], "item")
                                 else labels[j]})
            matches.append(row)
        out = df.copy()
        out[self.get("outputCol")] = matches
        return out
