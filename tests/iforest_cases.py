"""Cases and the checker shared by test_iforest_build_ref.py (the numpy
definition) and test_gpu_iforest_build.py (iforest_build_k on MI355X).

The checker is plain numpy in float64 and knows nothing of the random
numbers: it routes each tree's sample down the tree and checks structure."""
import functools
import math

import numpy as np
import torch

from mmlspark_amd.ops import backend

N_TREES = 7
SEED = 11
# name -> (n, nf, maxSamples, maxFeatures, bootstrap, data)
CASES = {
    "default-staged": (300, 3, 256, 1.0, False, "normal"),
    "sub-equals-n-97": (97, 5, 97, 1.0, False, "normal"),
    "two-samples": (64, 4, 2, 1.0, False, "normal"),
    "gather-pool-1024": (5000, 40, 1024, 0.5, False, "normal"),
    "bootstrap-duplicates": (50, 4, 256, 1.0, True, "normal"),
    "ties-three-constant": (400, 4, 256, 1.0, False, "ties"),
    "all-constant": (200, 3, 128, 1.0, False, "constant"),
    "lds-limit-4096": (6000, 2, 4096, 1.0, False, "normal"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(X float32 (n, nf), sub_n, n_feat, bootstrap), sized as _fit does."""
    n, nf, ms, mf, boot, data = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if data == "normal":
        X = rng.normal(size=(n, nf))
    elif data == "ties":
        X = np.ones((n, nf))
        X[:, 2] = rng.integers(0, 3, size=n)
    else:
        X = np.full((n, nf), 2.5)
    return X.astype(np.float32), min(ms, n), max(1, int(mf * nf)), boot


def build(name, device):
    X, sub_n, n_feat, boot = case(name)
    out = backend.iforest_build(torch.from_numpy(X).to(device), N_TREES,
                                sub_n, n_feat, boot, SEED)
    return [t.cpu().numpy() for t in out]


def check_forest(X, sub_n, n_feat, bootstrap, out, n_trees=N_TREES):
    rows, feat, thr, left, right, size, depth, offs = out
    n, nf = X.shape
    height = math.ceil(math.log2(max(sub_n, 2)))
    assert rows.shape == (n_trees, sub_n)
    assert rows.min() >= 0 and rows.max() < n
    if not bootstrap:
        assert all(len(np.unique(r)) == sub_n for r in rows)
    assert offs[0] == 0 and len(offs) == n_trees + 1
    N = int(offs[-1])
    counts = np.diff(offs)
    assert (counts >= 1).all() and (counts <= 2 * sub_n - 1).all()
    assert all(len(a) == N for a in (feat, thr, left, right, size, depth))
    base = np.repeat(offs[:-1], counts)
    local = np.arange(N) - base
    inner = feat >= 0
    roots = offs[:-1]
    assert (depth[roots] == 0).all() and (size[roots] == sub_n).all()
    # level order: children follow parents, left to right, each node once
    assert (left[inner] > local[inner]).all()
    assert (right[inner] == left[inner] + 1).all()
    assert (right[inner] < np.repeat(counts, counts)[inner]).all()
    gl, gr = (base + left)[inner], (base + right)[inner]
    assert (depth[gl] == depth[inner] + 1).all()
    assert (depth[gr] == depth[inner] + 1).all()
    kids = np.sort(np.concatenate([gl, gr]))
    assert np.array_equal(kids, np.setdiff1d(np.arange(N), roots))
    same_tree = np.diff(base[inner]) == 0
    assert (np.diff(left[inner])[same_tree] == 2).all()
    assert (left[~inner] == -1).all() and (right[~inner] == -1).all()
    assert (depth <= height).all() and (depth[inner] < height).all()
    assert ((feat[inner] < nf)).all()
    for t in range(n_trees):
        used = feat[offs[t]:offs[t + 1]]
        assert len(np.unique(used[used >= 0])) <= n_feat
    # route the samples
    x = X.astype(np.float64)[rows.reshape(-1)]
    cur = np.repeat(roots, sub_n)
    reach = np.zeros(N, np.int64)
    mn, mx = np.full((N, nf), np.inf), np.full((N, nf), -np.inf)
    act = np.arange(len(cur))
    while len(act):
        np.add.at(reach, cur[act], 1)
        np.minimum.at(mn, cur[act], x[act])
        np.maximum.at(mx, cur[act], x[act])
        act = act[inner[cur[act]]]
        node = cur[act]
        go_left = x[act, feat[node]] < thr[node]
        cur[act] = base[node] + np.where(go_left, left[node], right[node])
    assert np.array_equal(reach, size)
    lo, hi = mn[inner, feat[inner]], mx[inner, feat[inner]]
    t64 = thr[inner].astype(np.float64)
    assert (lo < t64).all() and (t64 <= hi).all()
    assert (size[gl] >= 1).all() and (size[gr] >= 1).all()
    early = ~inner & (size > 1) & (depth < height)
    assert (mn[early] == mx[early]).any(axis=1).all()
