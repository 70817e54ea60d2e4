"""Inputs, oracles and checks shared by test_knn_fused.py (CPU reference) and
test_gpu_knn.py (knn_partial_topk_k + knn_merge_k on MI355X).

Exact cases: integer features in [-8, 8] stored as float32 with d <= 200, so
every product, partial sum and squared norm is an integer below 2^24 and
float32 arithmetic is exact in any order.  The answer must then equal the
float64 oracle bit for bit, ties (by ascending index) included.

Float cases: standard-normal data against float64 distances D, per pair
within B = (d + 3) * 2^-23 * S, S = ||q||^2 + ||x||^2 + 2 sum|q_i x_i|: each
of the three sums carries at most d roundings of 2^-24 relative to its sum
of magnitudes, combining them adds two more, and B is twice that
first-order worst case."""
import functools

import numpy as np
import torch

from mmlspark_amd.ops import backend, cpu_ref

# name -> (n_q, n, d, k): every n_q in {1, 127, 129}, n in {1, 5, 128, 129,
# 1000}, d in {1, 3, 31, 32, 33, 128, 200} and k in {1, 5, 64} occurs.
SHAPES = {
    "q1-n1-d1-k1": (1, 1, 1, 1),
    "q1-n5-d3-k5": (1, 5, 3, 5),
    "q127-n128-d31-k64": (127, 128, 31, 64),
    "q129-n129-d33-k64": (129, 129, 33, 64),
    "q129-n1000-d200-k64": (129, 1000, 200, 64),
    "q127-n1000-d128-k5": (127, 1000, 128, 5),
    "q1-n1000-d32-k1": (1, 1000, 32, 1),
    "q129-n5-d128-k1": (129, 5, 128, 1),
    "q127-n129-d1-k5": (127, 129, 1, 5),
    "q129-n128-d200-k5": (129, 128, 200, 5),
    "q1-n129-d33-k64": (1, 129, 33, 64),
    "q127-n1000-d3-k64": (127, 1000, 3, 64),
}
TIE_NAMES = ("identical-300", "triples")
LABEL_COUNTS = (1, 32, 33, 65, 200)
SPLIT_NAMES = ("q129-n1000-d200-k64", "q129-n129-d33-k64")
FLOAT_DIMS = (3, 33, 128)


def _ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float32)


def bits_from_sets(sets, n_labels):
    """(len(sets), ceil(L / 32)) int32 bitsets, built without the model's
    helper."""
    W = max(1, (n_labels + 31) // 32)
    bits = np.zeros((len(sets), W), dtype=np.uint32)
    for i, allowed in enumerate(sets):
        for j in allowed:
            bits[i, j >> 5] |= np.uint32(1) << np.uint32(j & 31)
    return bits.view(np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(Q, X, k, label_ids, allow_bits, allowed): CPU tensors, the last
    three None without labels; `allowed` is the (n_q, n) bool truth."""
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name))
    rng = np.random.default_rng(seed)
    lab = bits = allowed = None
    if name in SHAPES:
        n_q, n, d, k = SHAPES[name]
        Q, X = _ints(rng, (n_q, d)), _ints(rng, (n, d))
    elif name == "identical-300":
        k = 64
        Q, X = _ints(rng, (3, 5)), np.tile(_ints(rng, (1, 5)), (300, 1))
    elif name == "triples":
        k = 10
        base = _ints(rng, (100, 4))
        X = np.tile(base, (3, 1))[rng.permutation(300)]
        Q = _ints(rng, (33, 4))
    elif name.startswith("labels-"):
        L, k = int(name.split("-")[1]), 5
        n_q, n = 40, 1000
        Q, X = _ints(rng, (n_q, 8)), _ints(rng, (n, 8))
        lab = rng.integers(0, L, size=n)
        if L > 1:   # the last label covers exactly three points: fewer than k
            lab[lab == L - 1] = 0
            lab[rng.choice(n, size=3, replace=False)] = L - 1
        sets = [set(), {L - 1}, set(range(L))]
        sets += [set(rng.choice(L, size=rng.integers(1, L + 1),
                                replace=False).tolist())
                 for _ in range(n_q - 3)]
        bits = bits_from_sets(sets, L)
        allowed = np.array([[int(l) in s for l in lab] for s in sets])
    elif name.startswith("float-"):
        parts = name.split("-")
        d, k = int(parts[1]), 10
        n_q, n = 129, 1000
        Q = rng.normal(size=(n_q, d)).astype(np.float32)
        X = rng.normal(size=(n, d)).astype(np.float32)
        X[rng.choice(n, size=50, replace=False)] = Q[rng.choice(n_q, size=50)]
        if len(parts) > 2:   # float-33-labels
            L = 33
            lab = rng.integers(0, L, size=n)
            sets = [set(rng.choice(L, size=rng.integers(4, L + 1),
                                   replace=False).tolist())
                    for _ in range(n_q)]
            bits = bits_from_sets(sets, L)
            allowed = np.array([[int(l) in s for l in lab] for s in sets])
    else:
        raise KeyError(name)
    out = {"Q": torch.from_numpy(Q), "X": torch.from_numpy(X), "k": k,
           "label_ids": None, "allow_bits": None, "allowed": allowed}
    if lab is not None:
        out["label_ids"] = torch.from_numpy(lab.astype(np.int32))
        out["allow_bits"] = torch.from_numpy(bits)
    return out


LABEL_NAMES = tuple("labels-%d" % L for L in LABEL_COUNTS)
EXACT_NAMES = tuple(SHAPES) + TIE_NAMES + LABEL_NAMES
FLOAT_NAMES = tuple("float-%d" % d for d in FLOAT_DIMS) + ("float-33-labels",)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(D (n_q, k) float64, idx (n_q, k) int32) of cpu_ref.knn_topk_f64."""
    c = case(name)
    return cpu_ref.knn_topk_f64(c["Q"], c["X"], c["k"], c["label_ids"],
                                c["allow_bits"])


def run(name, device, splits=0, labels=True):
    """backend.knn_topk on the case's tensors moved to `device`."""
    c = case(name)
    Q, X = c["Q"].to(device), c["X"].to(device)
    lab = bits = None
    if labels and c["label_ids"] is not None:
        lab, bits = c["label_ids"].to(device), c["allow_bits"].to(device)
    return backend.knn_topk(Q, X, (X * X).sum(dim=1), c["k"], lab, bits,
                            splits)


def check_exact(d2, idx, name):
    """Bit-for-bit equality with the oracle: no tolerance."""
    want_d, want_i = oracle(name)
    c = case(name)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32
    assert tuple(d2.shape) == tuple(idx.shape) == (c["Q"].shape[0], c["k"])
    assert torch.equal(idx.cpu(), want_i)
    assert torch.equal(d2.cpu(), want_d.to(torch.float32))
    assert torch.equal(want_d.to(torch.float32).double(), want_d)  # exact


def check_float(d2, idx, name):
    """The float checks; returns the worst share of a bound used."""
    c = case(name)
    Q, X, k = c["Q"].double().numpy(), c["X"].double().numpy(), c["k"]
    n_q, d = Q.shape
    n = X.shape[0]
    d2 = d2.cpu().double().numpy()
    idx = idx.cpu().numpy().astype(np.int64)
    allowed = (np.ones((n_q, n), dtype=bool) if c["allowed"] is None
               else c["allowed"])
    D = ((Q[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    S = ((Q * Q).sum(1)[:, None] + (X * X).sum(1)[None, :]
         + 2.0 * np.abs(Q[:, None, :] * X[None, :, :]).sum(axis=2))
    B = (d + 3) * 2.0 ** -23 * S
    worst = 0.0
    for i in range(n_q):
        assert allowed[i].sum() >= k   # the float cases leave no short list
        row = idx[i]
        assert len(set(row.tolist())) == k
        assert ((row >= 0) & (row < n)).all() and allowed[i, row].all()
        assert (np.diff(d2[i]) >= 0).all()
        b_max = B[i, allowed[i]].max()
        d_sorted = np.sort(D[i, allowed[i]])
        own = np.abs(d2[i] - D[i, row])
        assert (own <= B[i, row]).all()
        stat = np.abs(d2[i] - d_sorted[:k])
        assert (stat <= b_max).all()
        assert (D[i, row] <= d_sorted[k - 1] + 2 * b_max).all()
        worst = max(worst, (own / B[i, row]).max(), (stat / b_max).max())
    return worst
