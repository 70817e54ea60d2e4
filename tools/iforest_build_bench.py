#!/usr/bin/env python3
"""IsolationForest.fit on the GPU machine: fusedBuild=True (iforest_build_k,
one block per tree) against the host builder it stands beside, at

  20k-100x256     20k x 16 rows, 100 trees x 256 samples (tools/bench_misc.py)
  2M-100x256      2M x 16, 100 x 256
  2M-1000x4096    2M x 16, 1000 x 4096, maxFeatures = 0.5

Both paths are warmed up once, then alternated in this process; a sample is
the host clock around one fit (contamination = 0, so a fit is the build and
nothing else; the fused fit ends in device-to-host copies, so in a
synchronise).  The host builder gets --host-samples samples and no warm-up at
the last shape, where one fit takes about a minute.  Also times backend.iforest_build alone with
device events, X already on the device.  Prints medians with [min-max].
Needs a GPU: there is no fallback.

  python tools/iforest_build_bench.py [--shapes 20k-100x256] [--samples 5]
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

NF = 16
SHAPES = {  # name -> (rows, trees, maxSamples, maxFeatures)
    "20k-100x256": (20_000, 100, 256, 1.0),
    "2M-100x256": (2_000_000, 100, 256, 1.0),
    "2M-1000x4096": (2_000_000, 1000, 4096, 0.5),
}


def fmt(ts):
    ts = sorted(ts)
    return "%10.2f ms [%.2f-%.2f] n=%d" % (
        ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3, len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "iforest_build_bench needs a GPU"
    from mmlspark_amd.models.iforest import IsolationForest
    from mmlspark_amd.ops import backend

    cols = ["f%d" % i for i in range(NF)]
    for name in args.shapes.split(","):
        n, trees, ms, mf = SHAPES[name]
        X = np.random.default_rng(7).normal(size=(n, NF)).astype(np.float32)
        df = pd.DataFrame(X, columns=cols)
        print(f"{name}: {n} x {NF}, {trees} trees x {ms}, maxFeatures {mf}",
              flush=True)

        def fit(fused):
            est = IsolationForest(featureCols=cols, numEstimators=trees,
                                  maxSamples=ms, maxFeatures=mf,
                                  fusedBuild=fused)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = est.fit(df)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, len(
                m.get("forestArrays")["feature"])

        big = name == "2M-1000x4096"     # no host warm-up either: pure numpy
        n_host = args.host_samples if big else args.samples
        ts = {True: [], False: []}
        for fused in ((True,) if big else (True, False)):
            dt, nodes = fit(fused)
            print(f"    first fit, fused={fused}: {dt * 1e3:.1f} ms, {nodes} "
                  "nodes (warm-up, not a sample)", flush=True)
        for i in range(args.samples):
            ts[True].append(fit(True)[0])
            if i < n_host:
                ts[False].append(fit(False)[0])
        print("    fit fused " + fmt(ts[True]), flush=True)
        print("    fit host  " + fmt(ts[False]), flush=True)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        apart = min(ts[False]) > max(ts[True]) or \
            min(ts[True]) > max(ts[False])
        print("    host / fused = %.1fx, ranges %s" % (
            med(ts[False]) / med(ts[True]),
            "apart" if apart else "overlap"), flush=True)

        Xt = torch.from_numpy(X).cuda()
        n_feat = max(1, int(mf * NF))
        ev = []
        for i in range(args.samples + 1):
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            backend.iforest_build(Xt, trees, ms, n_feat, False, i)
            b.record()
            b.synchronize()
            ev.append(a.elapsed_time(b) * 1e-3)
        print("    backend.iforest_build alone (device events, first call "
              "dropped) " + fmt(ev[1:]), flush=True)
        del Xt


if __name__ == "__main__":
    main()
