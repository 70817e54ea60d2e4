"""Chosen (not found) cases for CSR forest scoring, shared by the CPU and GPU
test files: hand-built forests from a seeded generator and a 300x50 CSR
matrix that contains every row/entry shape the lookup can get wrong."""
import functools

import numpy as np
import torch

from mmlspark_amd.models.gbdt.booster import Booster
from mmlspark_amd.models.gbdt.sparse import CsrMatrix
from mmlspark_amd.models.gbdt.tree import Tree

N_ROWS, N_COLS = 300, 50
CAT_COLS = (3, 41)          # hold integer category codes
NEVER_STORED = (7, 23)      # no row before DENSE_ROW stores these columns
DENSE_ROW = 200             # the one fully dense row
UNSTORED_ROWS = DENSE_ROW   # rows [0, UNSTORED_ROWS) never store NEVER_STORED


def random_tree(rng, features, max_depth, cat_features=(), p_leaf=0.15):
    """Random binary tree, parents before children.  `features` is the pool
    of numeric split columns, `cat_features` the pool of categorical ones."""
    feat, thr, left, right, value, count = [], [], [], [], [], []
    leaf_index, cat_offset, cat_words = [], [], []

    def new_node():
        for a in (feat, thr, left, right, value, count, leaf_index,
                  cat_offset):
            a.append(0)
        return len(feat) - 1

    def grow(i, depth):
        if depth >= max_depth or (depth > 0 and rng.random() < p_leaf):
            feat[i], left[i], right[i] = -1, -1, -1
            thr[i] = 0.0
            value[i] = float(rng.normal())
            count[i] = float(rng.integers(1, 50))
            leaf_index[i] = sum(1 for f in feat[:i] if f == -1)
            cat_offset[i] = -1
            return
        if len(cat_features) and rng.random() < 0.4:
            feat[i] = int(rng.choice(cat_features))
            cat_offset[i] = len(cat_words) // 8
            cat_words.extend(int(w) for w in
                             rng.integers(0, 2**32, size=8, dtype=np.uint64))
            thr[i] = 0.0
        else:
            feat[i] = int(rng.choice(features))
            cat_offset[i] = -1
            # exact 0.0 thresholds put absent / stored-0.0 on the boundary
            thr[i] = 0.0 if rng.random() < 0.2 else float(rng.normal())
        leaf_index[i] = -1
        li, ri = new_node(), new_node()
        left[i], right[i] = li, ri
        grow(li, depth + 1)
        grow(ri, depth + 1)
        count[i] = count[li] + count[ri]
        value[i] = (value[li] * count[li] + value[ri] * count[ri]) / count[i]

    grow(new_node(), 0)
    # leaf ordinals in node order
    k = 0
    for i, f in enumerate(feat):
        if f == -1:
            leaf_index[i] = k
            k += 1
    n = len(feat)
    return Tree(feat, thr, np.zeros(n, dtype=np.int32), left, right, value,
                count, np.ones(n, dtype=np.float32), leaf_index,
                shrinkage=float(rng.uniform(0.05, 0.5)),
                cat_offset=cat_offset,
                cat_words=np.array(cat_words, dtype=np.uint32)
                if cat_words else None)


def stump(rng):
    return random_tree(rng, [0], max_depth=0)


@functools.lru_cache(maxsize=None)
def forests():
    """name -> Booster.  Single-output tree counts 1, 3, 4, 5, 9 cover the
    4-tree interleave body and its tail; non-unit tree weights throughout."""
    rng = np.random.default_rng(20240611)
    numeric = [c for c in range(N_COLS) if c not in CAT_COLS]
    out = {}

    def booster(trees, n_outputs=1, n_features=N_COLS):
        w = rng.uniform(0.25, 1.75, size=len(trees)).astype(np.float32)
        return Booster(trees, "regression" if n_outputs == 1 else "multiclass",
                       n_outputs,
                       rng.normal(size=n_outputs).astype(np.float32),
                       n_features, tree_weights=w)

    for nt in (1, 3, 4, 5, 9):
        trees = [random_tree(rng, numeric, max_depth=int(rng.integers(2, 9)))
                 for _ in range(nt)]
        if nt == 5:
            trees[2] = stump(rng)  # a finished chain inside the interleave
        if nt == 9:
            trees[0] = random_tree(rng, [0, N_COLS - 1], max_depth=8,
                                   p_leaf=0.0)  # full depth-8 tree
        out[f"t{nt}"] = booster(trees)
    out["stump"] = booster([stump(rng)])
    out["multi3"] = booster(
        [random_tree(rng, numeric, max_depth=5) for _ in range(6)],
        n_outputs=3)
    out["cat"] = booster(
        [random_tree(rng, numeric, max_depth=6, cat_features=CAT_COLS)
         for _ in range(5)])
    # splits on columns at/after the matrix width, mixed with real columns
    out["beyond"] = booster(
        [random_tree(rng, [0, 5, N_COLS - 1, N_COLS, N_COLS + 3,
                           N_COLS + 17], max_depth=5) for _ in range(5)],
        n_features=N_COLS + 18)
    # splits only on columns that rows [0, UNSTORED_ROWS) never store
    out["unstored"] = booster(
        [random_tree(rng, list(NEVER_STORED), max_depth=4)
         for _ in range(4)])
    return out


def _csr_from_rows(rows, n_cols):
    """rows: list of (cols ndarray int, vals ndarray f32), cols increasing."""
    lens = np.array([len(c) for c, _ in rows], dtype=np.int64)
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    col = (np.concatenate([c for c, _ in rows]).astype(np.int32)
           if lens.sum() else np.zeros(0, dtype=np.int32))
    val = (np.concatenate([v for _, v in rows]).astype(np.float32)
           if lens.sum() else np.zeros(0, dtype=np.float32))
    return CsrMatrix(torch.from_numpy(indptr), torch.from_numpy(col),
                     torch.from_numpy(val), (len(rows), n_cols))


def _values_for(rng, cols):
    v = rng.normal(size=len(cols)).astype(np.float32)
    for j, c in enumerate(cols):
        if c in CAT_COLS:
            v[j] = float(rng.integers(0, 40))
    r = rng.random(len(cols))
    v[r < 0.04] = 0.0          # stored zeros
    v[r > 0.96] = np.nan       # stored NaNs
    return v


@functools.lru_cache(maxsize=None)
def _edge_rows():
    rng = np.random.default_rng(77)
    f32 = np.float32
    rows = []
    for i in range(N_ROWS):
        allowed = np.array([c for c in range(N_COLS)
                            if i > DENSE_ROW or c not in NEVER_STORED])
        k = int(rng.integers(0, 13))
        cols = np.sort(rng.choice(allowed, size=k, replace=False))
        rows.append((cols, _values_for(rng, cols)))
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=f32))
    for i in (0, 10, 11, N_ROWS - 1):   # first, two adjacent, last
        rows[i] = empty
    rows[1] = (np.array([0]), np.array([-1.5], dtype=f32))         # 1 entry
    rows[2] = (np.array([N_COLS - 1]), np.array([0.25], dtype=f32))
    # stored 0.0 / NaN / negative, column 0 and nf-1, category >= 256
    rows[5] = (np.array([0, 3, 4, 9, 12, N_COLS - 1]),
               np.array([0.7, 300.0, 0.0, np.nan, -2.5, -0.1], dtype=f32))
    # negative and NaN categories, fractional category
    rows[6] = (np.array([3, 41]), np.array([-2.0, np.nan], dtype=f32))
    rows[8] = (np.array([3, 41]), np.array([255.0, 31.5], dtype=f32))
    rows[9] = (np.array([3, 41]), np.array([256.0, 0.0], dtype=f32))
    allc = np.arange(N_COLS)
    rows[DENSE_ROW] = (allc, _values_for(rng, allc))               # dense
    return rows


@functools.lru_cache(maxsize=None)
def edge_matrix():
    """The 300x50 matrix.  Treat as read-only (shared between tests)."""
    return _csr_from_rows(_edge_rows(), N_COLS)


def tiled_matrix(n, shift=5):
    """n rows cycling through the edge matrix, starting at row `shift`
    (so n == 1 is the stored 0.0 / NaN / negative / category-300 row)."""
    base = _edge_rows()
    return _csr_from_rows([base[(i + shift) % N_ROWS] for i in range(n)],
                          N_COLS)


def densified(csr, n_cols=None):
    """Dense copy, zero-padded to n_cols (for forests that split on columns
    at or beyond the matrix width)."""
    X = csr.densify()
    if n_cols is not None and n_cols > X.shape[1]:
        X = torch.cat([X, torch.zeros(X.shape[0], n_cols - X.shape[1],
                                      dtype=X.dtype, device=X.device)], dim=1)
    return X


def flat(booster, device="cpu"):
    return booster._flat(torch.device(device))


WIDE_ROWS, WIDE_COLS = 5000, 100_000


@functools.lru_cache(maxsize=None)
def wide_case():
    """5000 x 100000 matrix with <= 40 entries per row and a forest that
    splits on high column indices the rows do store."""
    rng = np.random.default_rng(5)
    hot = np.sort(rng.choice(np.arange(90_000, WIDE_COLS), size=48,
                             replace=False))
    hot[-1] = WIDE_COLS - 1
    rows = []
    for i in range(WIDE_ROWS):
        k_hot = int(rng.integers(0, 17))
        k_any = int(rng.integers(0, 25))
        cols = np.unique(np.concatenate([
            rng.choice(hot, size=k_hot, replace=False),
            rng.integers(0, WIDE_COLS, size=k_any)]))
        rows.append((cols, rng.normal(size=len(cols)).astype(np.float32)))
    csr = _csr_from_rows(rows, WIDE_COLS)
    trees = [random_tree(rng, list(hot), max_depth=7) for _ in range(9)]
    w = rng.uniform(0.25, 1.75, size=len(trees)).astype(np.float32)
    booster = Booster(trees, "regression", 1, np.zeros(1, dtype=np.float32),
                      WIDE_COLS, tree_weights=w)
    return csr, booster
