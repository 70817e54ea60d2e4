#!/usr/bin/env python3
"""KNN / ConditionalKNN search on the GPU: the fused kernels
(knn_partial_topk_k + knn_merge_k) against the torch path they replace
(distance tile + torch.topk, MMLSPARK_AMD_KNN_FUSED=0), at

  knn-200k      200k x 128 index, 50k queries, k = 10 (tools/bench_misc.py)
  cknn-2M-16    2M x 128, 16 labels, three allowed, 20k queries, k = 10
  cknn-2M-200   2M x 128, 200 labels, three allowed, --mask-queries queries
                (default 256): the torch path is the host-mask branch there,
                one (n_queries, 2M) bool matrix, so it gets fewer queries

For every shape it times KNNModel._search (conditioning inputs prepared
outside the clock) and whole transform calls.  Both paths are warmed up, then
alternated in this process; a sample is the host clock around one call, which
ends in a device-to-host copy, so in a synchronise.  Prints the median and
min-max of --samples samples per path, the achieved TFLOP/s of the distance
GEMM (2 n d n_q / t), whether the two ranges overlap, and how many of the
returned indices agree.

Kernel times come from a separate profiler run with --fused-only.
Needs a GPU: there is no fallback.

  python tools/knn_bench.py [--shapes knn-200k,cknn-2M-16] [--samples 5]
"""
import argparse
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

SWITCH = "MMLSPARK_AMD_KNN_FUSED"
DIM, K = 128, 10


def summary(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def timed_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def compare(paths, samples, flop):
    """Warm both up, alternate, print; True when fused beats torch with the
    ranges apart (or when only the fused path runs)."""
    outs, ts = {}, {name: [] for name in paths}
    for name, fn in paths.items():
        dt, outs[name] = timed_s(fn)
        print(f"    first call, {name}: {dt * 1e3:.1f} ms (warm-up, not a "
              "sample)", flush=True)
    for _ in range(samples):
        for name, fn in paths.items():
            ts[name].append(timed_s(fn)[0])
    stats = {}
    for name in paths:
        med, lo, hi = stats[name] = summary(ts[name])
        rate = f"  {flop / med / 1e12:6.1f} TFLOP/s" if flop else ""
        print(f"    {name:<6} median {med * 1e3:10.2f} ms  min {lo * 1e3:10.2f}"
              f"  max {hi * 1e3:10.2f}{rate}", flush=True)
    if len(paths) < 2:
        return True, outs
    apart = stats["fused"][2] < stats["torch"][1]
    print(f"    torch median / fused median: "
          f"{stats['torch'][0] / stats['fused'][0]:.1f}x; fused max below "
          f"torch min: {apart}", flush=True)
    return apart, outs


def with_switch(value, fn):
    def run():
        os.environ[SWITCH] = value
        return fn()
    return run


def bench_shape(name, args):
    from mmlspark_amd.models.knn import (ConditionalKNNModel, KNNModel,
                                         label_bitsets)
    n = 200_000 if name == "knn-200k" else 2_000_000
    n_labels = {"knn-200k": 0, "cknn-2M-16": 16, "cknn-2M-200": 200}[name]
    n_q = {"knn-200k": 50_000, "cknn-2M-16": 20_000,
           "cknn-2M-200": args.mask_queries}[name]
    rng = np.random.default_rng(len(name))
    X = rng.normal(size=(n, DIM)).astype(np.float32)
    Q = rng.normal(size=(n_q, DIM)).astype(np.float32)
    flop = 2.0 * n * DIM * n_q
    print(f"{name}: index {n} x {DIM}, {n_q} queries, k = {K}"
          + (f", {n_labels} labels, 3 allowed" if n_labels else ""),
          flush=True)
    query = pd.DataFrame({"features": list(Q)})
    if not n_labels:
        model = KNNModel(index=X, values=np.arange(n))
        search = {"fused": with_switch("1", lambda: model._search(Q)),
                  "torch": with_switch("0", lambda: model._search(Q))}
    else:
        labels = rng.integers(0, n_labels, size=n)
        conds = np.empty(n_q, dtype=object)
        conds[:] = [rng.choice(n_labels, size=3, replace=False).tolist()
                    for _ in range(n_q)]
        query["conditioner"] = conds
        model = ConditionalKNNModel(index=X, values=np.arange(n),
                                    labels=labels)
        uniq, lid = np.unique(labels, return_inverse=True)
        bits32 = label_bitsets(uniq, conds)
        search = {"fused": with_switch("1", lambda: model._search(
            Q, label_ids=lid, label_bits=bits32))}
        if not args.fused_only and n_labels <= 64:
            bits64 = np.zeros(n_q, dtype=np.int64)
            for i, c in enumerate(conds):
                for v in c:
                    bits64[i] |= 1 << v
            search["torch"] = with_switch("0", lambda: model._search(
                Q, cond_bits=bits64, label_ids=lid.astype(np.int64)))
        elif not args.fused_only:
            masks = np.stack([np.isin(labels, c) for c in conds])
            search["torch"] = with_switch("0", lambda: model._search(
                Q, masks))
    model.set("k", K)
    if args.fused_only:
        search.pop("torch", None)
    print("  _search:", flush=True)
    ok, outs = compare(search, args.samples, flop)
    if "torch" in outs:
        same = float((outs["fused"][0] == outs["torch"][0]).mean())
        gap = float(np.nanmax(np.abs(np.where(
            np.isfinite(outs["torch"][1]),
            outs["fused"][1] - outs["torch"][1], 0.0))))
        print(f"    indices equal: {same:.6f} of all slots; largest distance "
              f"gap {gap:.3g}", flush=True)
    if not args.skip_transform:
        print("  transform:", flush=True)
        paths = {"fused": with_switch("1", lambda: model.transform(query))}
        if not args.fused_only:
            paths["torch"] = with_switch("0", lambda: model.transform(query))
        compare(paths, args.transform_samples, 0)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="knn-200k,cknn-2M-16,cknn-2M-200")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--transform-samples", type=int, default=5)
    ap.add_argument("--mask-queries", type=int, default=256)
    ap.add_argument("--fused-only", action="store_true",
                    help="fused path only (profiler runs)")
    ap.add_argument("--skip-transform", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_bench needs a GPU; nothing was measured")
    from mmlspark_amd.ops.backend import _require_ext
    _require_ext()
    saved = os.environ.get(SWITCH)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    slow = [s for s in args.shapes.split(",") if not bench_shape(s, args)]
    if saved is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = saved
    if slow:
        sys.exit("fused _search does not beat the torch path with the ranges "
                 "apart at: " + ", ".join(slow))


if __name__ == "__main__":
    main()
