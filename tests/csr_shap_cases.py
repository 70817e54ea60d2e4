"""Shared helpers for the CSR TreeSHAP tests (CPU and GPU files): the flat
arrays the op takes, the float64 oracle computed once per case, and the
derived per-cell error bound."""
import functools

import numpy as np
import torch

from . import csr_predict_cases as cases

FOREST_NAMES = ["t1", "t3", "t4", "t5", "t9", "stump", "multi3", "cat",
                "beyond", "unstored"]
CAT_FRACTIONAL_ROW = 8   # category 31.5: Tree.cat_goes_left truncates


def op_args(booster, device="cpu"):
    """(positional node arrays, n_slots, keyword cat arrays, depth) for
    backend.tree_shap_csr / cpu_ref.tree_shap_csr."""
    dev = torch.device(device)
    f = booster._flat(dev)
    sf = booster._shap_flat(dev)
    nodes = (f["feature"], f["threshold"], f["left"], f["right"],
             sf["value"], sf["count"], f["offsets"], sf["slot"])
    kw = dict(cat_offset=f.get("cat_offset"), cat_words=f.get("cat_words"))
    return nodes, int(booster.used_features().size), kw, booster._tree_depth()


def oracle_on(booster, csr):
    """(phi, N, S) float64 / int64 / float64 numpy, (n, K, U + 1)."""
    from mmlspark_amd.ops import cpu_ref
    nodes, U, kw, _ = op_args(booster, "cpu")
    phi, N, S = cpu_ref.tree_shap_csr(
        *nodes, U, csr.indptr, csr.col, csr.val, csr.shape[1],
        booster.n_outputs, return_bound=True, **kw)
    return phi.numpy(), N.numpy(), S.numpy()


@functools.lru_cache(maxsize=None)
def edge_oracle(name):
    """Oracle of forest `name` on the 300-row edge matrix; read-only."""
    return oracle_on(cases.forests()[name], cases.edge_matrix())


@functools.lru_cache(maxsize=None)
def edge_cpu_compact(name):
    """Booster.predict_contrib_sparse of forest `name` on the edge matrix on
    the CPU (a per-row recursion: computed once); read-only."""
    return cases.forests()[name].predict_contrib_sparse(cases.edge_matrix())


@functools.lru_cache(maxsize=None)
def wide_oracle():
    """Oracle on all 5000 rows of the wide case; read-only."""
    csr, booster = cases.wide_case()
    return oracle_on(booster, csr)


def cell_bound(N, S, depth):
    """|kernel - oracle| allowed per cell: (N + D + 5) * 2^-23 * S.

    An addend's magnitude carries <= D + 3 relative roundings of 2^-24 (the
    f32 cover ratios if the device division is not correctly rounded, plus
    the cast to f32) and an absolute 2^-24 * S share from (o - z); the f32
    accumulation of N addends adds N * 2^-24 * S.  The bound is twice the
    sum of these."""
    return (N + depth + 5) * 2.0 ** -23 * S


def additivity_bound(booster, N, S, expected):
    """Allowed |sum of a row's cells - predict_raw| per (row, class): the
    cell bounds added up, the f32 cast of the expected value, and
    predict_raw's own f32 sum of T leaf values and the base score (T + 2
    roundings of at most 2^-24 relative to the sum of the largest |leaf
    value| of each tree and |base|, doubled like the cell bound)."""
    K = booster.n_outputs
    f = booster._shap_flat(torch.device("cpu"))
    off = booster._flat(torch.device("cpu"))["offsets"].numpy()
    mag = np.abs(np.resize(booster.base_score.astype(np.float64), K)) \
        if booster.base_score.size else np.zeros(K)
    mag = mag.copy()
    val = f["value"].numpy().astype(np.float64)
    for t in range(len(booster.trees)):
        mag[t % K] += np.abs(val[off[t]:off[t + 1]]).max()
    T = len(booster.trees)
    cells = cell_bound(N, S, booster._tree_depth()).sum(-1)
    return cells + 2.0 ** -23 * np.abs(expected)[None, :] \
        + (T + 2) * 2.0 ** -23 * mag[None, :]


def check_cells(got, phi, N, S, depth, what=""):
    """got (n, K, U + 1) vs the oracle on the contribution cells; prints the
    worst ratio before asserting."""
    got = np.asarray(got, dtype=np.float64)
    U = phi.shape[-1] - 1
    err = np.abs(got[..., :U] - phi[..., :U])
    bound = cell_bound(N, S, depth)[..., :U]
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max |err| {err.max() if err.size else 0.0:.3e}, "
          f"worst err/bound {ratio:.3f}")
    assert bool((err <= bound).all()), (what, ratio)


def run_op(booster, csr, device, **kw):
    """backend.tree_shap_csr on `csr` moved to `device`; (rows, K, U + 1)."""
    from mmlspark_amd.ops import backend
    nodes, U, cat, depth = op_args(booster, device)
    dev = csr.to(device)
    return backend.tree_shap_csr(
        *nodes, U, dev.indptr, dev.col, dev.val, dev.shape[1],
        booster.n_outputs, depth, **kw, **cat)
