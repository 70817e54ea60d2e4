"""Explainers with fusedSampling on against off, at the same commit.

    python tools/explain_fused_bench.py                    # on an MI355X
    python tools/explain_fused_bench.py --out profiles/explain_fused_bench.txt
    rocprofv3 --kernel-trace --stats -- \\
        python tools/explain_fused_bench.py --trace-run    # launches only

Both paths of a pair are warmed up, then alternated in one process, five
samples each; a sample is a host clock around as many back-to-back transforms
as fill about half a second (counted on one transform with it off, the same
for both paths), each ending in device-to-host copies of the scores and the
host solve.  Times are per transform.  Medians, min-max:
  (a) bench_shap.py's configuration: TabularSHAP, 20 features, 10,000
      samples, 1,000 background rows, 100 trees, 16 rows in one chunk
  (b) TabularLIME on the same model at its default 1,000 samples
  (c) small m, whole background cycled: TabularSHAP, 5 features, 30
      coalitions x B = nb = 1,000 draws, 16 rows
Each pair also reports how far the fused explanations are from the sample
path's.  The trace run calls backend.coalition_values alone on the shapes of
(a), (b) and (c), 8 launches each, and prints the forest traversals per
launch for the traversals/s figure.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmlspark_amd.explainers.lime import TabularLIME  # noqa: E402
from mmlspark_amd.explainers.shap import TabularSHAP  # noqa: E402
from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier  # noqa: E402
from mmlspark_amd.ops import backend  # noqa: E402

_OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if _OUT is not None:
        _OUT.write(line + "\n")
        _OUT.flush()


def summary(name, samples, n_rows):
    med = statistics.median(samples)
    row = {"what": name, "median_s": round(med, 5),
           "min_s": round(min(samples), 5), "max_s": round(max(samples), 5),
           "explanations_per_s_at_median": round(n_rows / med, 1),
           "samples": len(samples)}
    emit(row)
    return row


def pair(name, make, rows, n_samples=5):
    off, on = make(False), make(True)
    a = np.stack(off.transform(rows)["explanation"].to_numpy())
    b = np.stack(on.transform(rows)["explanation"].to_numpy())
    emit({"what": name + ": fused vs sample-path explanations",
          "max_abs_diff": float(np.abs(a - b).max()),
          "max_abs_value": float(np.abs(a).max())})
    t0 = time.perf_counter()
    off.transform(rows)
    torch.cuda.synchronize()
    reps = max(1, round(0.5 / (time.perf_counter() - t0)))
    ta, tb = [], []
    for _ in range(n_samples):
        for ex, acc in ((off, ta), (on, tb)):
            t0 = time.perf_counter()
            for _ in range(reps):
                ex.transform(rows)
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / reps)
    ra = summary(name + ", fusedSampling off", ta, len(rows))
    rb = summary(name + ", fusedSampling on", tb, len(rows))
    emit({"what": name + ": off/on at the medians",
          "transforms_per_sample": reps,
          "value": round(ra["median_s"] / rb["median_s"], 3),
          "ranges_overlap": not (min(ta) > max(tb) or min(tb) > max(ta))})


def fit(nf, trees, n=50_000):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(n, nf)).astype(np.float32)
    y = ((X @ rng.normal(size=nf)) + rng.normal(size=n) * 0.5 > 0)
    cols = [f"c{i}" for i in range(nf)]
    df = pd.DataFrame(X, columns=cols)
    df["label"] = y.astype(np.float32)
    model = LightGBMClassifier(featureCols=cols, numIterations=trees,
                               numLeaves=31, device="cuda").fit(df)
    return model, df, cols


def trace_run(args, models):
    """coalition_values alone, 8 launches per shape, for a kernel trace."""
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    shapes = [("(a) SHAP 16 rows x 10000 coalitions x 1 draw, shared masks",
               0, 1, 10000, 1),
              ("(b) LIME 16 rows x 1000 states x 1 draw, per-row masks",
               0, 16, 1000, 1),
              ("(c) SHAP 16 rows x 30 coalitions x 1000 cycled draws",
               1, 1, 30, 1000)]
    for name, which, Rm, nZ, B in shapes:
        model, df, cols = models[which]
        b, nf = model.booster, len(cols)
        f = b._flat(dev)
        X = torch.from_numpy(df[cols].to_numpy(np.float32)[:args.rows]).to(dev)
        bg = torch.from_numpy(
            df[cols].to_numpy(np.float32)[:args.background]).to(dev)
        masks = torch.from_numpy(rng.integers(
            0, 1 << nf, size=(Rm, nZ, 1)).astype(np.int32)).to(dev)
        bidx = None if B > 1 else torch.from_numpy(rng.integers(
            0, len(bg), size=(args.rows, nZ, B)).astype(np.int32))
        base = torch.from_numpy(b.base_score[:1].copy()).to(dev)
        for _ in range(8):
            backend.coalition_values(
                f["feature"], f["threshold"], f["left"], f["right"],
                f["value"], f["offsets"], f["weights"], X, bg, masks, bidx, B,
                base, 1, "sigmoid", b.sigmoid, (1,))
        torch.cuda.synchronize()
        emit({"what": "trace shape, 8 launches in trace order", "shape": name,
              "trees": b.num_trees, "nodes": int(f["feature"].numel()),
              "forest_traversals_per_launch": args.rows * nZ * B})


def main():
    global _OUT
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--features", type=int, default=20)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--background", type=int, default=1000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--out", default=None, help="also append rows to a file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU timing says nothing about these paths")
    if args.out:
        _OUT = open(args.out, "a")
    models = [fit(args.features, args.trees), fit(5, args.trees)]
    if args.trace_run:
        trace_run(args, models)
        return
    model, df, cols = models[0]
    kw = dict(inputCols=cols, model=model, targetCol="probability",
              targetClasses=[1], backgroundData=df.head(args.background),
              rowBatch=args.rows)
    rows = df.head(args.rows)
    pair("(a) TabularSHAP %d features, %d samples, %d background, %d trees, "
         "%d rows" % (args.features, args.samples, args.background,
                      args.trees, args.rows),
         lambda f: TabularSHAP(numSamples=args.samples, fusedSampling=f, **kw),
         rows)
    pair("(b) TabularLIME %d features, 1000 samples, %d rows"
         % (args.features, args.rows),
         lambda f: TabularLIME(fusedSampling=f, **kw), rows)
    model, df, cols = models[1]
    kw.update(inputCols=cols, model=model,
              backgroundData=df.head(args.background))
    pair("(c) TabularSHAP 5 features, 30 coalitions x %d cycled draws, %d rows"
         % (args.background, args.rows),
         lambda f: TabularSHAP(numSamples=30 * args.background,
                               fusedSampling=f, **kw), df.head(args.rows))


if __name__ == "__main__":
    main()
