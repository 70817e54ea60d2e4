#!/usr/bin/env python3
"""LambdarankObjective.grad_hess and LightGBMRanker.fit on the GPU: the two
rank kernels (group_rank_k + lambdarank_grad_k, every query group in two
launches) against the per-group Python loop they replace
(MMLSPARK_AMD_LAMBDARANK=0).

(a) grad_hess per call on a seeded ranking set: --docs documents (default
    2M) in query groups of 20..200 documents, 5 label levels.  Both paths are
    warmed up, then alternated in this process; every sample is a host clock
    around calls that end in a device synchronise.  A kernel sample covers
    enough back-to-back calls for --min-ms of work; a loop sample is one
    call, which takes seconds (about 25 small launches and one host
    synchronisation per group), so there are fewer of them.  Prints medians
    and min-max, and how far the two results are apart.
(b) LightGBMRanker.fit on --fit-rows x 32 features (default 200k) for 10
    iterations with every fifth group held out for validation, both ways,
    alternated: ms per iteration and the share of the time spent in
    grad_hess (`grad_s`; host time inside the call, which for the kernel
    path is the enqueue only) and in evaluation (`eval_s`) from
    TrainingStats.

Kernel times come from a separate profiler run of --no-loop --skip-fit.
Needs a GPU: there is no fallback.

  python tools/ranker_bench.py [--docs 2000000] [--fit-rows 200000]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

SWITCH = "MMLSPARK_AMD_LAMBDARANK"


def group_sizes_for(n, rng, lo=20, hi=200):
    """Sizes uniform in [lo, hi] that sum to n (the last group is cut)."""
    sizes = rng.integers(lo, hi + 1, size=n // lo + 1)
    ends = np.cumsum(sizes)
    k = int(np.searchsorted(ends, n))
    sizes = sizes[:k + 1].copy()
    sizes[k] -= ends[k] - n
    return sizes[sizes > 0]


def ranking_set(n, seed):
    rng = np.random.default_rng(seed)
    sizes = group_sizes_for(n, rng)
    label = rng.integers(0, 5, size=n).astype(np.float32)
    # scores correlated with the labels, as a few boosting rounds leave them
    score = (0.5 * label + rng.normal(size=n)).astype(np.float32)
    return sizes, label, score


def ranker_frame(n, nf, seed):
    import pandas as pd
    rng = np.random.default_rng(seed)
    sizes = group_sizes_for(n, rng)
    X = rng.normal(size=(n, nf)).astype(np.float32)
    w = rng.normal(size=nf) / np.sqrt(nf)
    rel = np.clip(np.round(2 + 1.5 * (X @ w) + rng.normal(size=n) * 0.5),
                  0, 4).astype(np.float32)
    group = np.repeat(np.arange(sizes.size), sizes)
    return pd.DataFrame({"features": list(X), "label": rel, "group": group,
                         "isVal": group % 5 == 0})


def timed_call_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def summary(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def bench_grad_hess(args):
    from mmlspark_amd.models.gbdt.objectives import LambdarankObjective
    sizes, label, score = ranking_set(args.docs, seed=11)
    print(f"(a) grad_hess: {args.docs} documents, {sizes.size} groups of "
          f"{sizes.min()}..{sizes.max()}, 5 label levels", flush=True)
    obj = LambdarankObjective()
    obj.group_sizes = torch.from_numpy(sizes)
    preds = torch.from_numpy(score).to("cuda").unsqueeze(-1)
    y = torch.from_numpy(label).to("cuda")

    def run(switch):
        os.environ[SWITCH] = switch
        return obj.grad_hess(preds, y, None)

    paths = {"kernels": lambda: run("1")}
    if not args.no_loop:
        paths["loop"] = lambda: run("0")
    outs = {}
    for k, fn in paths.items():  # warm-up; the first kernel call also builds
        t0 = time.perf_counter()  # the per-fit inputs
        outs[k] = fn()
        torch.cuda.synchronize()
        print(f"  first call, {k}: {(time.perf_counter() - t0) * 1e3:.1f} ms "
              "(warm-up, not a sample)", flush=True)
    if "loop" in outs:
        gk, hk = outs["kernels"]
        gl, hl = outs["loop"]
        print("  loop vs kernels: max|dg| / max|g| = "
              f"{float((gk - gl).abs().max() / gl.abs().max()):.3g}, "
              "max|dh| / max|h| = "
              f"{float((hk - hl).abs().max() / hl.abs().max()):.3g}")
    del outs
    once = timed_call_ms(paths["kernels"], 3)
    reps = {"kernels": max(1, int(np.ceil(args.min_ms / max(once, 1e-3)))),
            "loop": 1}
    left = {"kernels": args.kernel_samples,
            "loop": 0 if args.no_loop else args.loop_samples}
    ts = {k: [] for k in paths}
    while any(left[k] for k in paths):  # alternate while both have samples
        for k, fn in paths.items():
            if left[k]:
                ts[k].append(timed_call_ms(fn, reps[k]))
                left[k] -= 1
    med = {}
    for k in paths:
        med[k], lo, hi = summary(ts[k])
        print(f"  {k:<8} median {med[k]:10.3f} ms/call  min {lo:10.3f}  "
              f"max {hi:10.3f}  ({len(ts[k])} samples of {reps[k]} calls)")
    if "loop" in med:
        ok = med["kernels"] < min(ts["loop"])
        print(f"  loop median / kernel median: "
              f"{med['loop'] / med['kernels']:.0f}x; kernel median below "
              f"the loop's minimum: {ok}", flush=True)
        return ok
    return True


def bench_fit(args):
    from mmlspark_amd.models.gbdt.estimators import LightGBMRanker
    df = ranker_frame(args.fit_rows, 32, seed=12)
    n_val = int(df["isVal"].sum())
    print(f"(b) LightGBMRanker.fit: {len(df)} x 32, "
          f"{df['group'].nunique()} groups, {n_val} validation rows, "
          f"{args.fit_iters} iterations, 63 leaves, evalAt=[5, 10]",
          flush=True)

    def fit(switch, iters):
        os.environ[SWITCH] = switch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = LightGBMRanker(numIterations=iters, numLeaves=63,
                           groupCol="group", evalAt=[5, 10],
                           validationIndicatorCol="isVal",
                           device="cuda").fit(df)
        torch.cuda.synchronize()
        return m._training_stats, time.perf_counter() - t0

    fit("1", 2)  # warm-up: code objects, allocator
    ways = [("kernels", "1")] + ([] if args.no_loop else [("loop", "0")])
    for rnd in range(args.fit_rounds):
        for name, switch in ways:
            st, wall = fit(switch, args.fit_iters)
            last = st.evals[-1]["valid_0"] if st.evals else {}
            print(f"  round {rnd} {name:<8} {st.total_s / st.iterations * 1e3:9.1f} "
                  f"ms/iteration  grad_s {st.grad_s / st.total_s:6.1%}  "
                  f"eval_s {st.eval_s / st.total_s:6.1%}  "
                  f"(train loop {st.total_s:.2f} s of fit {wall:.2f} s; "
                  f"last {last})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=2_000_000)
    ap.add_argument("--kernel-samples", type=int, default=5)
    ap.add_argument("--loop-samples", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=200.0,
                    help="work each kernel-path sample must cover")
    ap.add_argument("--fit-rows", type=int, default=200_000)
    ap.add_argument("--fit-iters", type=int, default=10)
    ap.add_argument("--fit-rounds", type=int, default=2)
    ap.add_argument("--no-loop", action="store_true",
                    help="kernel path only (profiler runs)")
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ranker_bench needs a GPU; nothing was measured")
    from mmlspark_amd.ops.backend import _require_ext
    _require_ext()
    saved = os.environ.get(SWITCH)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    ok = bench_grad_hess(args)
    if not args.skip_fit:
        bench_fit(args)
    if saved is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = saved
    if not ok:
        sys.exit("the kernel path's median is not below the loop's minimum")


if __name__ == "__main__":
    main()
