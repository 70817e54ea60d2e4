"""LIME explainers with fusedFit on against off, at the same commit.

    python tools/lime_fit_bench.py                    # on an MI355X
    python tools/lime_fit_bench.py --out profiles/lime_fit_bench.txt

Both paths of a pair are warmed up, then alternated in one process, five
samples each; a sample is a host clock around one transform ending in a
device synchronise.  Medians, min-max:
  (a) TabularLIME, 16 rows, 20 features, 1,000 samples, 100 trees,
      fusedSampling=True on both sides
  (b) VectorLIME, 16 rows, 70 features, 130 samples, fusedSampling=True on
      both sides
  (c) ImageLIME, one 224 x 224 x 3 uint8 image, ImageFeaturizer(ResNet50),
      cellSize 16, 512 samples, fusedSampling=True on both sides
Each pair also reports how far the fusedFit explanations and r2 are from the
host fit's (which rounds every coordinate update through float32).  Then
backend.lime_fit alone at the three shapes, between device events, ten
launches each after a warm-up.
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

from mmlspark_amd.explainers.lime import (ImageLIME, TabularLIME,  # noqa: E402
                                          VectorLIME)
from mmlspark_amd.explainers.sampler import lime_sample_states  # noqa: E402
from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier  # noqa: E402
from mmlspark_amd.models.image_featurizer import ImageFeaturizer  # noqa: E402
from mmlspark_amd.ops import backend  # noqa: E402

_OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if _OUT is not None:
        _OUT.write(line + "\n")
        _OUT.flush()


def summary(name, samples):
    row = {"what": name, "median_s": round(statistics.median(samples), 6),
           "min_s": round(min(samples), 6), "max_s": round(max(samples), 6),
           "samples": len(samples)}
    emit(row)
    return row


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def pair(name, make, df, n_samples=5):
    off, on = make(False), make(True)
    a, b = off.transform(df), on.transform(df)
    ea, eb = (np.stack(o["explanation"].to_numpy()) for o in (a, b))
    ra, rb = (np.stack(o["r2"].to_numpy()) for o in (a, b))
    emit({"what": name + ": fusedFit vs host fit",
          "max_abs_diff": float(np.abs(ea - eb).max()),
          "max_abs_value": float(np.abs(ea).max()),
          "r2_max_abs_diff": float(np.abs(ra - rb).max())})
    ta, tb = [], []
    for _ in range(n_samples):
        for ex, acc in ((off, ta), (on, tb)):
            acc.append(timed(lambda: ex.transform(df)))
    sa = summary(name + ", fusedFit off", ta)
    sb = summary(name + ", fusedFit on", tb)
    emit({"what": name + ": off/on at the medians",
          "value": round(sa["median_s"] / sb["median_s"], 3),
          "ranges_overlap": not (min(ta) > max(tb) or min(tb) > max(ta))})


def fit(nf, trees, n=50_000):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(n, nf)).astype(np.float32)
    y = ((X @ rng.normal(size=nf)) + rng.normal(size=n) * 0.5 > 0)
    cols = [f"c{i}" for i in range(nf)]
    df = pd.DataFrame(X, columns=cols)
    df["features"] = list(X)
    df["label"] = y.astype(np.float32)
    model = LightGBMClassifier(featureCols=cols, numIterations=trees,
                               numLeaves=31, device="cuda").fit(df)
    return model, df, cols


def kernel_alone(name, R, n, m, C=1, launches=10):
    rng = np.random.default_rng(0)
    S = np.stack([lime_sample_states(m, n, rng) for _ in range(R)])
    Y = S @ rng.normal(size=(m, C)) + 0.05 * rng.normal(size=(R, n, C))
    bits = torch.stack([backend.pack_states(s) for s in S]).cuda()
    y = torch.from_numpy(Y).cuda()
    sweeps = backend.lime_fit(bits, m, y, 0.75, 0.0)[3]
    ms = []
    for _ in range(launches):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        backend.lime_fit(bits, m, y, 0.75, 0.0)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / 1e3)
    row = summary("backend.lime_fit alone, " + name, ms)
    emit({"what": "shape of " + name, "R": R, "n": n, "m": m, "C": C,
          "sweeps_max": int(sweeps.max()),
          "fits_per_s_at_median": round(R * C / row["median_s"], 1)})


def main():
    global _OUT
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--skip-image", action="store_true")
    ap.add_argument("--out", default=None, help="also append rows to a file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU timing says nothing about these paths")
    if args.out:
        _OUT = open(args.out, "a")
    model, df, cols = fit(20, 100)
    kw = dict(model=model, targetCol="probability", targetClasses=[1],
              backgroundData=df.head(1000), rowBatch=args.rows,
              fusedSampling=True)
    pair("(a) TabularLIME %d rows, 20 features, 1000 samples" % args.rows,
         lambda f: TabularLIME(inputCols=cols, fusedFit=f, **kw),
         df.head(args.rows))
    model, df, cols = fit(70, 100)
    kw.update(model=model, backgroundData=df.head(1000))
    pair("(b) VectorLIME %d rows, 70 features, 130 samples" % args.rows,
         lambda f: VectorLIME(numSamples=130, fusedFit=f, **kw),
         df.head(args.rows))
    if not args.skip_image:
        rng = np.random.default_rng(0)
        yy, xx = np.mgrid[0:224, 0:224]
        img = 127 + 100 * np.sin((yy + 2 * xx) / 40.0)[..., None] \
            + rng.normal(0, 12, size=(224, 224, 3))
        one = pd.DataFrame({"image": [np.clip(img, 0, 255).astype(np.uint8)]})
        torch.manual_seed(0)
        feat = ImageFeaturizer(modelName="ResNet50", inputCol="image",
                               outputCol="features", device="cuda")
        pair("(c) ImageLIME 224x224, ResNet50, 512 samples",
             lambda f: ImageLIME(model=feat, inputCol="image",
                                 targetCol="features", targetClasses=[0],
                                 fusedSampling=True, fusedFit=f), one)
    kernel_alone("(a) 16 x 1000 x 20", 16, 1000, 20)
    kernel_alone("(b) 16 x 130 x 70", 16, 130, 70)
    kernel_alone("(c) 1 x 512 x 196", 1, 512, 196)


if __name__ == "__main__":
    main()
