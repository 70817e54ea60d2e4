"""Shared cases and oracle of the binning tests (CPU and GPU files).

The oracle is a per-element numpy searchsorted(side="left") over the
feature's bounds, clamped to n_bins - 1, NaN -> bin 0: bin = the number of
bounds strictly below x, so x == bound stays in the bound's own bin (the rule
that agrees with the scorer's `x <= threshold || isnan(x)`).  It is exact;
the tests compare the whole (ngroups, n, 4) tensor, pad lanes included."""
import functools

import numpy as np
import torch

from mmlspark_amd.models.gbdt.booster import Booster
from mmlspark_amd.models.gbdt.tree import Tree

f32 = np.float32
INF = f32(np.inf)
FLT_MAX = np.finfo(f32).max
TINY = np.finfo(f32).tiny            # smallest normal
SUB = f32(1e-45)                     # smallest subnormal

NFS = (1, 3, 4, 5, 9)
NBINS = (2, 3, 16, 255, 256)
NS = (0, 1, 255, 257)
# more rows than one launch's 8192 blocks x 256 threads: the grid-stride loop
# of bin_matrix_k runs a second pass for the last 3 rows
STRIDE_CASE = (1, 255, 8192 * 256 + 3)

CASES = tuple((nf, nb, n) for nf in NFS for nb in NBINS for n in NS)


def case_id(c):
    return "nf%d-bins%d-n%d" % c


def bounds(nf, n_bins):
    """(nf, n_bins - 1) float32, each row ascending.  Row kinds by feature
    index mod 5: distinct values around 0 with subnormals; every value twice;
    +inf from the middle to the end; all +inf; -inf first."""
    nb = n_bins - 1
    rng = np.random.default_rng(1000 * nf + n_bins)
    rows = []
    for f in range(nf):
        kind = f % 5
        v = np.sort(rng.normal(size=nb).astype(f32) * f32(3))
        fixed = np.array([0.0, -SUB, SUB, TINY, -1.0, 1.0, -FLT_MAX],
                         dtype=f32)[:max(nb - 1, 1)]
        v[:len(fixed)] = fixed
        v = np.sort(v)
        if kind == 1:
            v = np.sort(np.repeat(v[::2], 2)[:nb] if nb > 1 else v)
        elif kind == 2:
            v[nb // 2:] = INF
        elif kind == 3:
            v[:] = INF
        elif kind == 4:
            v[0] = -INF
        if kind in (0, 1, 4) and nb > 1:
            v[-1] = INF                       # the mapper's own padding
        assert len(v) == nb and np.all(v[1:] >= v[:-1])
        rows.append(v.astype(f32))
    return np.stack(rows)


def values_for(row):
    """Every value a bound row can get wrong: each bound, its neighbours in
    both directions, signed zeros, infinities, NaN, subnormals, +-FLT_MAX."""
    b = np.unique(row)
    with np.errstate(over="ignore", invalid="ignore"):
        near = np.concatenate([b, np.nextafter(b, -INF), np.nextafter(b, INF)])
    extra = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, SUB, -SUB,
                      f32(1e-40), f32(-1e-40), TINY, -TINY, FLT_MAX,
                      -FLT_MAX, 0.5, -0.5], dtype=f32)
    return np.concatenate([near.astype(f32), extra])


def data(ub, n):
    """(n, nf) float32: column f walks through values_for(ub[f]), each
    column from a different start."""
    nf = ub.shape[0]
    X = np.empty((n, nf), dtype=f32)
    for f in range(nf):
        vals = values_for(ub[f])
        X[:, f] = vals[(np.arange(n) + 97 * f) % len(vals)]
    return X


def all_values_data(ub):
    """Rows enough for every column to hold every one of its values."""
    n = max(len(values_for(r)) for r in ub)
    return data(ub, n)


def oracle_bins(X, ub, n_bins):
    """(n, nf) int64 bins, element by element."""
    n, nf = X.shape
    out = np.zeros((n, nf), dtype=np.int64)
    for f in range(nf):
        col = X[:, f]
        nan = np.isnan(col)
        idx = np.searchsorted(ub[f], np.where(nan, f32(0), col), side="left")
        out[:, f] = np.where(nan, 0, np.minimum(idx, n_bins - 1))
    return out


def oracle(X, ub, n_bins):
    """(ngroups, n, 4) uint8, pad lanes of the last group 0."""
    n, nf = X.shape
    ng = (nf + 3) // 4
    out = np.zeros((ng, n, 4), dtype=np.uint8)
    bins = oracle_bins(X, ub, n_bins)
    for f in range(nf):
        out[f // 4, :, f % 4] = bins[:, f]
    return out


@functools.lru_cache(maxsize=None)
def case(c):
    """(X, ub, expected) of a (nf, n_bins, n) case; read-only."""
    nf, nb, n = c
    ub = bounds(nf, nb)
    X = data(ub, n)
    return X, ub, oracle(X, ub, nb)


@functools.lru_cache(maxsize=None)
def routing_case(n_bins):
    """(X, ub, stump booster, (feature, bound index) per stump): one stump
    per feature and bound index b with threshold ub[f][b], over data that
    holds every value of values_for in every column."""
    nf = 5
    ub = bounds(nf, n_bins)
    X = all_values_data(ub)
    trees, where = [], []
    for f in range(nf):
        for b in range(n_bins - 1):
            trees.append(Tree([f, -1, -1], [ub[f, b], 0.0, 0.0],
                              [b, 0, 0], [1, -1, -1], [2, -1, -1],
                              [0.0, -1.0, 1.0], [2.0, 1.0, 1.0],
                              [1.0, 0.0, 0.0], [-1, 0, 1]))
            where.append((f, b))
    booster = Booster(trees, "regression", 1, np.zeros(1, dtype=f32), nf)
    return X, ub, booster, np.array(where)


def check_routing(leaf, bins, where):
    """leaf (n, n_stumps) from predict_leaf, bins (n, nf): a row went left
    (leaf 0) exactly when its bin is <= the stump's bound index."""
    leaf = np.asarray(leaf)
    assert set(np.unique(leaf)) <= {0, 1}
    went_left = leaf == 0
    want = bins[:, where[:, 0]] <= where[None, :, 1]
    bad = np.argwhere(went_left != want)
    assert bad.size == 0, ("row, stump", bad[:5].tolist())


def to_torch(X, ub, device="cpu"):
    return (torch.from_numpy(np.ascontiguousarray(X)).to(device),
            torch.from_numpy(np.ascontiguousarray(ub)).to(device))
