#!/usr/bin/env python3
"""Booster.predict_raw on a CsrMatrix: the CSR traversal kernel against the
densify-then-dense-kernel loop it replaced.

Model: a seeded synthetic forest, 100 trees x 63 leaves, built directly as
Tree objects (leaf-wise random growth, no training).  Inputs: seeded CSR with
exactly 20 stored values per row at 1M x 100 and 1M x 100,000 columns.  Stored
columns and split features are drawn from the same skewed distribution (low
column ids are frequent), so traversals hit stored entries as they do on a
trained sparse model instead of missing everywhere.

Protocol: warm both paths up, then alternate them in this process --rounds
times each; every sample is device events around enough back-to-back calls
to cover --min-ms of work.  Prints per-call median and min-max for both and
the ratio of medians.  Needs a GPU: there is no fallback.

  python tools/csr_predict_bench.py [--rows 1000000] [--rounds 5]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

NNZ = 20
SKEW = 3.0


def skewed_columns(rng, size, nf):
    """Column ids in [0, nf - NNZ], low ids frequent."""
    return np.floor((nf - NNZ + 1) * rng.random(size) ** SKEW).astype(np.int64)


def synthetic_forest(nf, n_trees=100, n_leaves=63, seed=1):
    from mmlspark_amd.models.gbdt.booster import Booster
    from mmlspark_amd.models.gbdt.tree import Tree
    rng = np.random.default_rng(seed)
    trees = []
    for _ in range(n_trees):
        n_nodes = 2 * n_leaves - 1
        feat = np.full(n_nodes, -1, dtype=np.int32)
        thr = np.zeros(n_nodes, dtype=np.float32)
        left = np.full(n_nodes, -1, dtype=np.int32)
        right = np.full(n_nodes, -1, dtype=np.int32)
        leaves, used = [0], 1
        while len(leaves) < n_leaves:  # split a random leaf (leaf-wise)
            i = leaves.pop(int(rng.integers(len(leaves))))
            feat[i] = skewed_columns(rng, 1, nf)[0] + rng.integers(0, NNZ)
            thr[i] = rng.normal(scale=0.5)
            left[i], right[i] = used, used + 1
            leaves += [used, used + 1]
            used += 2
        is_leaf = feat < 0
        leaf_index = np.full(n_nodes, -1, dtype=np.int32)
        leaf_index[is_leaf] = np.arange(n_leaves, dtype=np.int32)
        value = np.where(is_leaf, rng.normal(size=n_nodes), 0.0)
        trees.append(Tree(feat, thr, np.zeros(n_nodes, dtype=np.int32), left,
                          right, value, np.ones(n_nodes), np.zeros(n_nodes),
                          leaf_index, shrinkage=0.1))
    return Booster(trees, "regression", 1, np.zeros(1, dtype=np.float32), nf)


def synthetic_csr(n, nf, seed=2):
    """Exactly NNZ strictly increasing columns per row."""
    from mmlspark_amd.models.gbdt.sparse import CsrMatrix
    rng = np.random.default_rng(seed)
    col = np.sort(skewed_columns(rng, (n, NNZ), nf), axis=1) + np.arange(NNZ)
    val = rng.normal(size=n * NNZ).astype(np.float32)
    indptr = np.arange(0, (n + 1) * NNZ, NNZ, dtype=np.int64)
    return CsrMatrix(torch.from_numpy(indptr),
                     torch.from_numpy(col.reshape(-1).astype(np.int32)),
                     torch.from_numpy(val), (n, nf))


def densify_chunks_baseline(booster, csr):
    """What Booster.predict_raw did with a CsrMatrix before the CSR kernel:
    dense tiles of up to 1 GB (zero-fill + scatter), each through the dense
    forest kernel."""
    outs = [booster.predict_raw(chunk) for _, chunk in csr.densify_chunks()]
    return torch.cat(outs, dim=0)


def timed_ms(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, nargs="+",
                    default=[100, 100_000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-ms", type=float, default=400.0,
                    help="device time each timed sample must cover")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("csr_predict_bench needs a GPU; nothing was measured")
    from mmlspark_amd.ops.backend import _require_ext
    _require_ext()
    print(f"device: {torch.cuda.get_device_name(0)}  rows={args.rows} "
          f"nnz/row={NNZ} forest=100x63 rounds={args.rounds} "
          f"min window={args.min_ms:.0f} ms", flush=True)
    for nf in args.features:
        booster = synthetic_forest(nf)
        csr = synthetic_csr(args.rows, nf).to("cuda")
        paths = {"csr_kernel": lambda: booster.predict_raw(csr),
                 "densify_chunks_baseline":
                     lambda: densify_chunks_baseline(booster, csr)}
        # warm-up (code objects, allocator) + the results must agree exactly
        outs = {k: fn() for k, fn in paths.items()}
        torch.cuda.synchronize()
        same = torch.equal(outs["csr_kernel"],
                           outs["densify_chunks_baseline"])
        del outs
        reps = {}
        for k, fn in paths.items():
            once = timed_ms(fn, 1)
            reps[k] = max(1, int(np.ceil(args.min_ms / max(once, 1e-3))))
        ts = {k: [] for k in paths}
        for _ in range(args.rounds):  # alternate the two paths
            for k, fn in paths.items():
                ts[k].append(timed_ms(fn, reps[k]))
        print(f"shape {args.rows} x {nf}  (outputs bit-equal: {same})")
        med = {}
        for k in paths:
            med[k], lo, hi = summary(ts[k])
            print(f"  {k:<24} median {med[k]:10.3f} ms/call  "
                  f"min {lo:10.3f}  max {hi:10.3f}  "
                  f"({reps[k]} calls per sample)")
        print(f"  speedup (baseline median / csr median): "
              f"{med['densify_chunks_baseline'] / med['csr_kernel']:.2f}x",
              flush=True)
        if not same:
            sys.exit("CSR and densified scores differ")


if __name__ == "__main__":
    main()
