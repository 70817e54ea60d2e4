"""fusedInteractions on and off: VowpalWabbitRegressor fit and transform with
-q crossings on MI355X.

  --shape q2x32   two namespaces a, b of 32 non-zeros each, `-q ab`:
                  64 stored entries and 1024 crossings per row
  --shape q3x16   three namespaces of 16 non-zeros each, `-q ::`: 48 stored
                  entries and 6 pairs x 256 crossings per row

Sparse-vector columns over 2^24 raw indices, so the materialised path takes
its per-row loop (the dense fast path of VowpalWabbitInteractions does not
apply).  Off: the crossings are materialised on the host and the device holds
the expanded CSR.  On: the device holds each column once and
vw_sgd_interact_k / vw_predict_interact_k generate the crossings.  Both sides
warmed up, alternated in one process, medians with min-max; wall times end in
a device synchronise.  Per side also the host featurisation time
(nativeIngestTimeNs), learnTimeNs as the estimator reports it (it contains
the per-minibatch host waits) and the device bytes of the batch; and one
trained table scored by both paths.  Prints text lines; the committed copy is
profiles/vw_interact_bench.txt."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pandas as pd
import torch

import mmlspark_amd
from mmlspark_amd.core.schema import SparseVector
from mmlspark_amd.models.vw.estimators import VowpalWabbitRegressor
from mmlspark_amd.ops import backend

SHAPES = {"q2x32": (("a", "b"), 32, "-q ab"),
          "q3x16": (("a", "b", "c"), 16, "-q ::")}
PASSES = 4


def frame(cols, nnz, n, seed=3):
    rng = np.random.default_rng(seed)
    data = {}
    for c in cols:
        idx = rng.integers(0, 1 << 24, (n, nnz)).astype(np.int32)
        val = (0.1 * rng.normal(size=(n, nnz))).astype(np.float32)
        data[c] = [SparseVector(1 << 30, i, v) for i, v in zip(idx, val)]
    data["label"] = rng.normal(size=n)
    return pd.DataFrame(data)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def report(name, values, unit="ms"):
    v = np.array(values)
    print("%-40s median %10.2f %s   min %10.2f   max %10.2f   (n=%d)"
          % (name, np.median(v), unit, v.min(), v.max(), len(v)), flush=True)


def compare(shape, n, rounds):
    cols, nnz, q = SHAPES[shape]
    df = frame(cols, nnz, n)
    print("shape %s: %d rows, namespaces %s x %d non-zeros, args '%s', "
          "%d passes, learning rate 0.05, numBits 22, batchSize 4096"
          % (shape, n, "/".join(cols), nnz, q, PASSES), flush=True)
    sides = {"off": False, "on": True}
    fit_t = {k: [] for k in sides}
    tr_t = {k: [] for k in sides}
    ingest = {k: [] for k in sides}
    learn = {k: [] for k in sides}
    stored = {}
    for rnd in range(rounds + 1):                # round 0 warms up
        for side, on in sides.items():
            est = VowpalWabbitRegressor(
                featuresCol=cols[0], additionalFeatures=list(cols[1:]),
                args=q + " --holdout_off", numPasses=PASSES, numBits=22,
                learningRate=0.05, fusedInteractions=on, device="cuda")
            dt_fit, model = timed(lambda: est.fit(df))
            dt_tr, out = timed(lambda: model.transform(df))
            st = model.getPerformanceStatistics().iloc[0]
            stored[side] = int(st["totalNumberOfFeatures"])
            pred = out["prediction"].to_numpy()
            if rnd:
                fit_t[side].append(dt_fit * 1e3)
                tr_t[side].append(dt_tr * 1e3)
                ingest[side].append(st["nativeIngestTimeNs"] / 1e6)
                learn[side].append(st["learnTimeNs"] / 1e6)
    for side in sides:
        report("%s fit, fused %s" % (shape, side), fit_t[side])
        report("%s   host featurisation" % shape, ingest[side])
        report("%s   learnTimeNs" % shape, learn[side])
        report("%s transform, fused %s" % (shape, side), tr_t[side])
        offsets = n * (len(cols) + 1) if side == "on" else n + 1
        print("%s   device batch, fused %s: %d stored entries, %.2f MB"
              % (shape, side, stored[side],
                 (stored[side] * 8 + offsets * 8) / 1e6), flush=True)
    # the last model is the fused one: score its table by the other path
    model.set("fusedInteractions", False)
    ref = model.transform(df)["prediction"].to_numpy()
    print("%s: one table scored by both paths: max |on - off| %.3e (largest "
          "prediction %.3e); the order of the float32 sum and the pre-summed "
          "collisions of the materialised path are the difference"
          % (shape, np.abs(pred - ref).max(), np.abs(ref).max()), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=tuple(SHAPES) + ("all",), default="all")
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available() and backend.hip_available()
    mmlspark_amd._register_all()
    for s in (tuple(SHAPES) if args.shape == "all" else (args.shape,)):
        compare(s, args.rows, args.rounds)
