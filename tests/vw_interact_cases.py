"""Compact namespace batches for the vw_*_interact kernels and their numpy
expansion, from the slot rules alone, to the flat batches that the float64
oracle of vw_kernel_cases runs over.  Every seed below is one for which the
expanded slots are distinct (Batch asserts it)."""
import numpy as np

from . import vw_kernel_cases as cases

FNV = 16777619
BITS = 20


class Compact:
    """idx int32 raw, val float32, ns_off int64 (n_ex, n_cols + 1), col_seed
    and pair_seed int32, pairs int32 (n_pairs, 2); labels y, weights h."""

    def __init__(self, idx, val, ns_off, col_seed, pairs, pair_seed, bits,
                 y, h):
        i32 = np.int32
        self.idx, self.val = np.asarray(idx, i32), np.asarray(val, np.float32)
        self.ns_off = np.asarray(ns_off, np.int64)
        self.col_seed = np.asarray(col_seed, i32)
        self.pair_seed = np.asarray(pair_seed, i32)
        self.pairs = np.asarray(pairs, i32).reshape(-1, 2)
        self.bits, self.y, self.h = bits, y, h

    def tensors(self, device):
        import torch
        return [torch.from_numpy(a.copy()).to(device) for a in (
            self.idx, self.val, self.ns_off, self.col_seed, self.pairs,
            self.pair_seed)] + [self.bits]


def expand_arrays(c):
    """(slots, float32 values, offsets) of the flat batch: per example the
    linear entries column by column, then pair after pair, j fastest."""
    m = (1 << c.bits) - 1
    raw = c.idx.astype(np.int64)
    slots, vals, off = [], [], [0]
    for row in c.ns_off:
        n = 0
        for k, seed in enumerate(c.col_seed):
            sl = slice(row[k], row[k + 1])
            slots.append(((raw[sl] + int(seed)) & 0x3FFFFFFF) & m)
            vals.append(c.val[sl])
            n += row[k + 1] - row[k]
        for (a, b), seed in zip(c.pairs, c.pair_seed):
            ri, rj = raw[row[a]:row[a + 1]], raw[row[b]:row[b + 1]]
            hsh = (((ri[:, None] * FNV) & 0xFFFFFFFF) ^ rj[None, :]) & m
            slots.append((((hsh + int(seed)) & 0x3FFFFFFF) & m).reshape(-1))
            vals.append((c.val[row[a]:row[a + 1], None]    # float32 product
                         * c.val[None, row[b]:row[b + 1]]).reshape(-1))
            n += ri.size * rj.size
        off.append(off[-1] + n)
    return np.concatenate(slots), np.concatenate(vals), np.array(off)


expand = lambda c: cases.Batch(*expand_arrays(c), c.y, c.h)  # noqa: E731

def lane_terms(c):
    """Products per lane and example: columns and pairs with |B| < 64 are
    strided (flattened), a pair with |B| >= 64 along j for every i."""
    cnt = np.diff(c.ns_off, axis=1)
    t = (-(-cnt // 64)).sum(axis=1)
    for a, b in c.pairs:
        na, nb = cnt[:, a], cnt[:, b]
        t = t + np.where(nb < 64, -(-(na * nb) // 64), na * -(-nb // 64))
    return t


def build(seed, sizes, pairs, bits=BITS, col_seed=None, pair_seed=None,
          labels="pm1", raw_bits=24):
    """Columns of the given sizes per example, raw indices distinct."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n_ex, n_cols = sizes.shape
    ns_off = np.zeros((n_ex, n_cols + 1), dtype=np.int64)
    ns_off[:, 1:] = np.cumsum(sizes.reshape(-1)).reshape(sizes.shape)
    ns_off[1:, 0] = ns_off[:-1, -1]
    nnz = int(sizes.sum())
    idx = rng.choice(1 << raw_bits, nnz, replace=False)
    val = cases._values(rng, nnz)
    y = rng.choice([-1.0, 1.0], n_ex)
    if labels == "real":
        y = y * rng.uniform(4.0, 8.0, n_ex)
    h = rng.uniform(0.25, 4.0, n_ex)
    if col_seed is None:
        col_seed = np.append(0, rng.integers(1, 1 << 30, n_cols - 1))
    if pair_seed is None:
        pair_seed = rng.integers(1, 1 << 30, len(pairs))
    return Compact(idx, val, ns_off, col_seed, pairs, pair_seed, bits,
                   y.astype(np.float32), h.astype(np.float32))


# seeds that, with the raw indices' top bits, wrap past 0x3FFFFFFF
WRAP = 0x3FFFFF00
# name -> (seed, sizes, pairs, extra build arguments)
SHAPES = {
    # both lane splits and their tails, empty sides, an empty example and a
    # third column that is in no pair; two blocks
    "grid": (2, ((63, 1, 2), (64, 2, 0), (65, 3, 1), (1, 130, 3), (2, 65, 0),
                 (0, 7, 1), (7, 0, 2), (0, 0, 0)), [(0, 1)], {}),
    # a self pair, two pairs sharing a column, a pair and its reverse
    "pairs": (1, [(5, 9, 4), (3, 0, 6), (8, 2, 1), (1, 1, 1), (6, 7, 0)],
              [(0, 0), (0, 1), (1, 0), (1, 2)],
              dict(col_seed=[WRAP + 1, WRAP + 77, WRAP + 150],
                   pair_seed=[WRAP + 5, WRAP + 9, WRAP + 200, WRAP + 250],
                   raw_bits=30)),
}


def window_shape(window):
    """Column 0 fills the window, column 1 is the first overflow entry (both
    in pair (0, 1)), column 2 lies past it: (1, 2) runs along j in global."""
    return (1, [(window, 1, 70), (3, 2, 0)], [(0, 1), (1, 2)], {})


def wrap_shape():
    """One example more than 4096 blocks x 4 waves hold, one linear feature
    each; the first, the wrapped and a middle example also have a pair."""
    sizes = np.zeros((16385, 2), dtype=np.int64)
    sizes[:, 0] = 1
    sizes[[0, 9000, 16384], 1] = 3
    return (1, sizes, [(0, 1)], dict(raw_bits=BITS, col_seed=[0, 12345]))


# the grid's configurations: (loss, invariant, power_t, normalized, l2)
CONFIGS = cases.SHAPE_CONFIGS + (
    ("logistic", True, cases.POWER_TS[2], False, cases.L2),
    ("squared", False, cases.POWER_TS[2], True, 0.0))


def make_case(name, spec, config, n_steps):
    seed, sizes, pairs, kw = spec
    loss, invariant, power_t, normalized, l2 = config
    c = build(seed, sizes, pairs,
              labels="real" if loss == "squared" else "pm1", **kw)
    w0, g0 = cases.warm_tables(seed + 100, 1 << c.bits)
    return c, cases.Case("%s-%s" % (name, cases.grid_id(config)), expand(c),
                         w0, g0, loss, invariant, power_t, normalized, l2,
                         (cases.LR,) * n_steps)


def adaptors(c, sgd, predict, device):
    """sgd/predict as check_case calls the flat kernels, over c instead."""
    t = c.tensors(device)
    return (lambda idx, val, off, *rest: sgd(*t, *rest),
            lambda idx, val, off, w: predict(*t, w))


ALL_SHAPES = list(SHAPES) + ["window", "wrap"]


def spec_for(shape, window=512):
    # (spec, successive calls): three on the grids, one on launch shapes
    if shape in SHAPES:
        return SHAPES[shape], 3
    return (window_shape(window) if shape == "window" else wrap_shape()), 1


def frame(seed=1, n=12):
    """Sparse-vector columns features and b over disjoint raw indices, c for
    the three-column spec; and the compact batch of '-q ::' over the two."""
    import pandas as pd
    from mmlspark_amd.core.schema import SparseVector
    from mmlspark_amd.models.vw.murmur import hash_string
    rng = np.random.default_rng(seed)
    sizes = np.stack([rng.integers(1, 7, n),
                      rng.integers(0, 6, n)], axis=1)
    c = build(seed, sizes, [(0, 0), (0, 1), (1, 1)], labels="real",
              col_seed=[0, hash_string("b") & 0x3FFFFFFF],
              pair_seed=[hash_string("__interact_%d" % k) & 0x3FFFFFFF
                         for k in range(3)])

    def column(k):
        return [SparseVector(1 << 30, c.idx[r[k]:r[k + 1]],
                             c.val[r[k]:r[k + 1]]) for r in c.ns_off]

    third = [SparseVector(1 << 30, np.array([5 + r], np.int32),
                          np.array([1.5], np.float32))
             for r in range(n)]
    df = pd.DataFrame({"features": column(0), "b": column(1), "c": third,
                       "label": c.y.astype(np.float64)})
    c.h = None
    return df, c
