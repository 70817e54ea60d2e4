#!/usr/bin/env python3
"""TreeSHAP contributions of a CsrMatrix: the CSR kernel with its compact
result against the densify-then-dense-kernel loop it replaced.

Model and inputs are csr_predict_bench's: a seeded synthetic forest of 100
trees x 63 leaves (here with real cover counts: random leaf covers summed up
the tree) and seeded CSR rows with exactly 20 stored values, at widths 100
and 100,000.  The row count (default 8192) is one at which the baseline's
dense (n, nf + 1) result still fits in host memory at the wide width
(8192 x 100,001 float32 = 3.3 GB).

Three paths, each a whole Booster call including its host work:
  densify_baseline   what predict_contrib(CsrMatrix) did before: dense tiles
                     of up to 1 GB through tree_shap_k, dense result on host
  compact            predict_contrib_sparse: tree_shap_csr_k, (n, 1, U + 1)
                     left on the device
  dense_contract     predict_contrib(CsrMatrix) now: compact result
                     scattered into the dense (n, nf + 1) host matrix

Protocol: warm all paths up, then alternate them in this process --rounds
times; every sample is wall-clock between device synchronisations around
enough back-to-back calls to cover --min-ms.  Prints per-call median and
min-max and the ratios of medians.  Needs a GPU: there is no fallback.

  python tools/csr_shap_bench.py [--rows 8192] [--rounds 5]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from csr_predict_bench import NNZ, summary, synthetic_csr, synthetic_forest


def shap_forest(nf, seed=3):
    """csr_predict_bench's forest with cover counts a trained tree would
    have: random leaf covers, interior = sum of children."""
    booster = synthetic_forest(nf)
    rng = np.random.default_rng(seed)
    for t in booster.trees:
        leaf = t.feature < 0
        t.count[leaf] = rng.integers(20, 2000, size=int(leaf.sum()))
        for i in range(t.n_nodes - 1, -1, -1):  # children follow parents
            if not leaf[i]:
                t.count[i] = t.count[t.left[i]] + t.count[t.right[i]]
    booster.invalidate_cache()
    return booster


def densify_baseline(booster, csr):
    """Booster.predict_contrib on a CsrMatrix before the CSR kernel."""
    outs = [booster.predict_contrib(chunk) for _, chunk in csr.densify_chunks()]
    return np.concatenate(outs, axis=0)


def timed_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--features", type=int, nargs="+",
                    default=[100, 100_000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-ms", type=float, default=400.0,
                    help="wall time each timed sample must cover")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("csr_shap_bench needs a GPU; nothing was measured")
    from mmlspark_amd.ops.backend import _require_ext
    _require_ext()
    print(f"device: {torch.cuda.get_device_name(0)}  rows={args.rows} "
          f"nnz/row={NNZ} forest=100x63 rounds={args.rounds} "
          f"min window={args.min_ms:.0f} ms", flush=True)
    for nf in args.features:
        booster = shap_forest(nf)
        csr = synthetic_csr(args.rows, nf).to("cuda")
        paths = {"densify_baseline": lambda: densify_baseline(booster, csr),
                 "compact": lambda: booster.predict_contrib_sparse(csr),
                 "dense_contract": lambda: booster.predict_contrib(csr)}
        # warm-up (code objects, allocator, cached model arrays) + agreement
        outs = {k: fn() for k, fn in paths.items()}
        torch.cuda.synchronize()
        feats, values = outs["compact"]
        diff = max(float(np.abs(outs["densify_baseline"][s:s + 512]
                                - outs["dense_contract"][s:s + 512]).max())
                   for s in range(0, args.rows, 512))
        U = int(feats.size)
        v = values.cpu().numpy()[:, 0]
        # two runs of the float atomics: equal up to summation order
        diff_c = max(
            float(np.abs(outs["dense_contract"][:, feats] - v[:, :U]).max()),
            float(np.abs(outs["dense_contract"][:, nf] - v[:, U]).max()))
        unused = np.setdiff1d(np.arange(nf), feats)
        zeros = not outs["dense_contract"][:, unused].any()
        del outs, values, v
        reps = {}
        for k, fn in paths.items():
            once = timed_ms(fn, 1)
            reps[k] = max(1, int(np.ceil(args.min_ms / max(once, 1e-3))))
        ts = {k: [] for k in paths}
        for _ in range(args.rounds):  # alternate the paths
            for k, fn in paths.items():
                ts[k].append(timed_ms(fn, reps[k]))
        print(f"shape {args.rows} x {nf}  depth {booster._tree_depth()}  "
              f"used features U={U}  compact bytes/row {4 * (U + 1)}  "
              f"dense bytes/row {4 * (nf + 1)}")
        print(f"  max |baseline - dense_contract| {diff:.3e}  "
              f"max |dense_contract - compact scattered| {diff_c:.3e}  "
              f"(unused features exactly 0: {zeros})")
        med = {}
        for k in paths:
            med[k], lo, hi = summary(ts[k])
            print(f"  {k:<18} median {med[k]:10.3f} ms/call  "
                  f"min {lo:10.3f}  max {hi:10.3f}  "
                  f"({reps[k]} calls per sample)")
        for k in ("compact", "dense_contract"):
            print(f"  speedup (baseline median / {k} median): "
                  f"{med['densify_baseline'] / med[k]:.2f}x", flush=True)
        if max(diff, diff_c) > 1e-4 or not zeros:
            sys.exit("the paths disagree beyond float summation order")


if __name__ == "__main__":
    main()
