"""Query-group plumbing of the ranker: the per-fit inputs of the rank kernels
(ops/hip/rank_kernels.hip), their host-side validation, and NDCG@k computed
from in-group ranks without a loop over groups.

Everything a kernel indexes with is built and checked here, once, on the
host: group offsets (start at 0, non-decreasing, end at n), the group id of
each document, and - when a labelGain table is given - that every label is
an integer inside the table.  A violation raises ValueError before anything
is launched.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from ...ops import backend


def kernel_path_enabled() -> bool:
    """MMLSPARK_AMD_LAMBDARANK=0 keeps device tensors on the per-group loops
    (gradients and NDCG); default 1.  Read before any launch."""
    return os.environ.get("MMLSPARK_AMD_LAMBDARANK", "1") != "0"


def check_offsets(offsets: np.ndarray, n: int) -> np.ndarray:
    """Group boundaries as a validated (G+1) int64 array."""
    offsets = np.asarray(offsets)
    if offsets.ndim != 1 or offsets.size < 1:
        raise ValueError("group offsets must be a (G+1) vector")
    offsets = offsets.astype(np.int64)
    if offsets[0] != 0:
        raise ValueError("group offsets must start at 0")
    if (np.diff(offsets) < 0).any():
        raise ValueError("group offsets must be non-decreasing "
                         "(negative group size)")
    if offsets[-1] != n:
        raise ValueError(
            f"group offsets must end at the number of documents "
            f"({int(offsets[-1])} != {n})")
    return offsets


def offsets_from_sizes(group_sizes, n: int) -> np.ndarray:
    sizes = (group_sizes.detach().cpu().numpy()
             if isinstance(group_sizes, torch.Tensor)
             else np.asarray(group_sizes))
    sizes = sizes.astype(np.int64).reshape(-1)
    return check_offsets(np.concatenate([[0], np.cumsum(sizes)]), n)


def check_labels(label: np.ndarray, label_gain) -> None:
    """With a labelGain table every label must index it."""
    if label_gain is None or label.size == 0:
        return
    ok = np.isfinite(label) & (label == np.floor(label)) \
        & (label >= 0) & (label < len(label_gain))
    if not ok.all():
        bad = label[~ok][0]
        raise ValueError(
            f"label {bad!r} is not an integer in [0, {len(label_gain)}): "
            "outside the labelGain table")


def _group_ids(offsets: np.ndarray) -> np.ndarray:
    sizes = np.diff(offsets)
    return np.repeat(np.arange(sizes.size, dtype=np.int32), sizes)


def discount_table(m: int) -> np.ndarray:
    """1 / log2(r + 2) for r in [0, m), float64."""
    return 1.0 / np.log2(np.arange(m, dtype=np.float64) + 2.0)


def ideal_dcg(gain: np.ndarray, offsets: np.ndarray, gid: np.ndarray,
              disc: np.ndarray, k: Optional[int] = None) -> np.ndarray:
    """Per-group DCG of the gains sorted descending (float64), over the first
    min(k, m) positions when k is given."""
    n_groups = offsets.size - 1
    if gain.size == 0:
        return np.zeros(n_groups, dtype=np.float64)
    order = np.lexsort((-gain, gid))  # by group, gains descending inside
    pos = np.arange(gain.size) - offsets[gid]
    terms = gain[order].astype(np.float64) * disc[pos]
    if k is not None:
        terms = np.where(pos < k, terms, 0.0)
    return np.bincount(gid, weights=terms, minlength=n_groups)


@dataclass
class RankInputs:
    """What the rank kernels read besides the scores, on one device."""
    n: int
    n_groups: int
    offsets: torch.Tensor   # (G+1) int64
    gid: torch.Tensor       # (n) int32
    label: torch.Tensor     # (n) f32
    gain: torch.Tensor      # (n) f32
    inv_idcg: torch.Tensor  # (G) f32
    disc_tbl: torch.Tensor  # (max group size, at least 1) f32


def build_rank_inputs(group_sizes, label: torch.Tensor,
                      gains_fn: Callable[[torch.Tensor], torch.Tensor],
                      label_gain, device) -> RankInputs:
    """Validate and build the per-fit kernel inputs.  gains_fn maps a CPU
    label tensor to float32 gains (LambdarankObjective._gains); it runs only
    after the labels have been checked against the table."""
    label_cpu = label.detach().to("cpu", torch.float32).reshape(-1)
    n = label_cpu.numel()
    offsets = offsets_from_sizes(group_sizes, n)
    label_np = label_cpu.numpy()
    check_labels(label_np, label_gain)
    gain_cpu = gains_fn(label_cpu).to(torch.float32)
    gid = _group_ids(offsets)
    max_m = int(np.diff(offsets).max()) if offsets.size > 1 else 0
    disc = discount_table(max(max_m, 1))
    idcg = ideal_dcg(gain_cpu.numpy(), offsets, gid, disc)
    inv_idcg = (1.0 / np.maximum(idcg, 1e-12)).astype(np.float32)
    return RankInputs(
        n=n, n_groups=offsets.size - 1,
        offsets=torch.from_numpy(offsets).to(device),
        gid=torch.from_numpy(gid).to(device),
        label=label_cpu.to(device),
        gain=gain_cpu.to(device),
        inv_idcg=torch.from_numpy(inv_idcg).to(device),
        disc_tbl=torch.from_numpy(disc.astype(np.float32)).to(device))


class NdcgEvaluator:
    """NDCG@k of one labelled, grouped set for any number of score vectors.

    Built once per validation set: the group table, the float64 gains and
    the ideal DCG per (group, k) stay on the labels' device.  A call ranks
    the scores with `backend.group_rank` (stable descending, ties by index:
    np.argsort(-s, kind="stable")), forms where(rank < k, gain * disc[rank],
    0) in float64 and segment-sums it by group.  Semantics of the host loop
    it replaces: empty groups are skipped, a group's value is dcg / idcg or 0
    when idcg == 0, the result is the mean over non-empty groups, 0 when
    there are none."""

    def __init__(self, labels: torch.Tensor, offsets,
                 eval_at: Sequence[int], label_gain=None):
        device = labels.device
        label_cpu = labels.detach().to("cpu", torch.float32).reshape(-1)
        label_np = label_cpu.numpy()
        n = label_np.size
        if isinstance(offsets, torch.Tensor):
            offsets = offsets.detach().cpu().numpy()
        offsets = check_offsets(offsets, n)
        check_labels(label_np, label_gain)
        if label_gain is not None:
            gain = np.asarray(label_gain, dtype=np.float64)[
                label_np.astype(np.int64)]
        else:
            gain = (np.float32(2.0) ** label_np
                    - np.float32(1.0)).astype(np.float64)
        gid = _group_ids(offsets)
        sizes = np.diff(offsets)
        disc = discount_table(max(int(sizes.max()) if sizes.size else 0, 1))
        self.eval_at = [int(k) for k in eval_at]
        idcg = np.stack([ideal_dcg(gain, offsets, gid, disc, k)
                         for k in self.eval_at]) if self.eval_at else \
            np.zeros((0, sizes.size))
        self.n = n
        self.n_groups = int(sizes.size)
        self.n_nonempty = int((sizes > 0).sum())
        self.offsets = torch.from_numpy(offsets).to(device)
        self.gid = torch.from_numpy(gid).to(device)
        self.gid_long = self.gid.long()
        self.label = label_cpu.to(device)
        self.gain32 = torch.from_numpy(gain.astype(np.float32)).to(device)
        self.disc32 = torch.from_numpy(disc.astype(np.float32)).to(device)
        self.gain = torch.from_numpy(gain).to(device)
        self.disc = torch.from_numpy(disc).to(device)
        self.idcg = torch.from_numpy(idcg).to(device)

    def __call__(self, scores: torch.Tensor) -> List[float]:
        if not self.eval_at:
            return []
        if self.n_nonempty == 0:
            return [0.0] * len(self.eval_at)
        s = scores.reshape(-1).to(torch.float32).contiguous()
        if s.numel() != self.n:
            raise ValueError("scores must have one entry per document")
        rank, _ = backend.group_rank(s, self.offsets, self.gid, self.label,
                                     self.gain32, self.disc32)
        rank = rank.long()
        contrib = self.gain * self.disc[rank]
        zero = torch.zeros_like(contrib)
        means = []
        for ki, k in enumerate(self.eval_at):
            dcg = torch.zeros(self.n_groups, dtype=torch.float64,
                              device=s.device)
            dcg.index_add_(0, self.gid_long,
                           torch.where(rank < k, contrib, zero))
            idcg = self.idcg[ki]
            val = torch.where(idcg > 0, dcg / idcg, torch.zeros_like(dcg))
            means.append(val.sum() / self.n_nonempty)
        return torch.stack(means).tolist()  # one readback for every k


def ndcg_at(scores: torch.Tensor, labels: torch.Tensor, offsets,
            eval_at: Sequence[int], label_gain=None) -> List[float]:
    """Mean NDCG@k over the non-empty query groups, one value per k of
    eval_at, on the device of `scores` and `labels` (HIP kernel for device
    tensors, torch reference on the CPU)."""
    return NdcgEvaluator(labels, offsets, eval_at, label_gain)(scores)
