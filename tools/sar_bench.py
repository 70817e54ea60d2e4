"""Sparse against dense SAR on MI355X.

  --shape a      the bench_misc shape (50k users, 5k items, 1M interactions):
                 fit and _recommend_arrays(None, 10, True), sparse against
                 dense (the baseline), both warmed up, alternated in one
                 process, medians of 5 with min-max
  --shape sweep  item-tile sweep of the two tiled kernels at shape a
  --shape b      a shape the dense path cannot hold (2M users, 200k items,
                 40M interactions), sparse only, with the peak device memory
                 and the CSR byte counts
  --shape trace  one sparse fit + recommend + transform at shape a, for a
                 separate `rocprofv3 --kernel-trace --stats -- python
                 tools/sar_bench.py --shape trace` run

Prints text lines; the committed copies are profiles/sar_bench.txt and
profiles/sar_kernel_stats.txt."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pandas as pd
import torch

from mmlspark_amd.models.sar import SAR
from mmlspark_amd.ops import backend


def frame(n_users, n_items, n_inter, skew, seed=2):
    rng = np.random.default_rng(seed)
    r = rng.random(n_inter)
    item = (n_items * r ** skew).astype(np.int64) if skew != 1 \
        else rng.integers(0, n_items, n_inter)
    return pd.DataFrame({
        "user": rng.integers(0, n_users, n_inter),
        "item": np.minimum(item, n_items - 1),
        "rating": rng.random(n_inter).astype(np.float32) * 5,
        "timestamp": rng.integers(1_600_000_000, 1_700_000_000, n_inter),
    })


def estimator(matrix_type):
    return SAR(userCol="user", itemCol="item", ratingCol="rating",
               timeCol="timestamp", matrixType=matrix_type)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def report(name, times):
    ms = np.array(times) * 1e3
    print("%-34s median %9.2f ms   min %9.2f   max %9.2f   (n=%d)"
          % (name, np.median(ms), ms.min(), ms.max(), len(ms)), flush=True)


def csr_bytes(d):
    return {k: int(v.nbytes) for k, v in d.items()}


def shape_a(rounds=5):
    df = frame(50_000, 5_000, 1_000_000, 1)
    print("shape a: 50000 users x 5000 items, 1000000 interactions "
          "(uniform), k=10, remove_seen", flush=True)
    kinds = ("dense", "sparse")
    models = {k: estimator(k).fit(df) for k in kinds}          # warm-up
    for k in kinds:
        models[k]._recommend_arrays(None, 10, True)
    fit_t = {k: [] for k in kinds}
    rec_t = {k: [] for k in kinds}
    for _ in range(rounds):
        for k in kinds:
            dt, models[k] = timed(lambda: estimator(k).fit(df))
            fit_t[k].append(dt)
        for k in kinds:
            models[k]._recommend_arrays(None, 10, True)   # uploads its arrays
            dt, _ = timed(lambda: models[k]._recommend_arrays(None, 10, True))
            rec_t[k].append(dt)
    for k in kinds:
        report("fit, %s" % k, fit_t[k])
    for k in kinds:
        report("_recommend_arrays, %s" % k, rec_t[k])
    d = models["sparse"].get("sarArrays")
    print("sparse sarArrays bytes: %d (similarity nnz %d, affinity nnz %d); "
          "dense sarArrays bytes: %d"
          % (sum(csr_bytes(d).values()), len(d["similarity_col"]),
             len(d["affinity_col"]),
             sum(csr_bytes(models["dense"].get("sarArrays")).values())),
          flush=True)
    return models["sparse"]


def sweep(rounds=5):
    model = estimator("sparse").fit(frame(50_000, 5_000, 1_000_000, 1))
    dev = torch.device("cuda")
    csr = model._csr_on(dev)
    print("tile sweep at shape a (device time of the backend call, no "
          "host copies)", flush=True)
    tiles = (512, 1024, 2048, 4096, 5056, 8192)
    times = {t: [] for t in tiles}
    for r in range(rounds + 1):
        for t in tiles:
            dt, _ = timed(lambda: backend.sar_recommend(
                *csr, None, 10, True, tile=t, check=False))
            if r:
                times[t].append(dt)
    for t in tiles:
        report("sar_recommend tile %d" % t, times[t])
    a_indptr, a_col, a_val = csr[:3]
    seen = a_val > 0
    rows = torch.repeat_interleave(
        torch.arange(a_indptr.numel() - 1, device=dev),
        a_indptr[1:] - a_indptr[:-1])[seen]
    cols = a_col[seen]
    order = torch.sort(cols.long() * 50_000 + rows).indices
    b_indptr = torch.zeros(50_001, dtype=torch.int64, device=dev)
    b_indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=50_000), 0)
    bt_indptr = torch.zeros(5_001, dtype=torch.int64, device=dev)
    bt_indptr[1:] = torch.cumsum(torch.bincount(cols, minlength=5_000), 0)
    bt_col = rows[order].to(torch.int32).contiguous()
    times = {t: [] for t in tiles}
    for r in range(rounds + 1):
        for t in tiles:
            dt, _ = timed(lambda: backend.sar_cooccurrence(
                b_indptr, cols.contiguous(), bt_indptr, bt_col, 4, "jaccard",
                tile=t, check=False))
            if r:
                times[t].append(dt)
    for t in tiles:
        report("sar_cooccurrence tile %d" % t, times[t])


def shape_b():
    n_users, n_items, n_inter = 2_000_000, 200_000, 40_000_000
    print("shape b: %d users x %d items, %d interactions (item = "
          "floor(items * r^2), r uniform), sparse only; dense affinity alone "
          "would be %.0f GB" % (n_users, n_items, n_inter,
                                n_users * n_items * 4 / 1e9), flush=True)
    df = frame(n_users, n_items, n_inter, 2)
    torch.cuda.reset_peak_memory_stats()
    dt, model = timed(lambda: estimator("sparse").fit(df))
    print("fit, sparse                        %9.2f s   peak device memory "
          "%.1f MB" % (dt, torch.cuda.max_memory_allocated() / 1e6),
          flush=True)
    d = model.get("sarArrays")
    for k, v in csr_bytes(d).items():
        print("  %-18s %12d bytes" % (k, v), flush=True)
    print("  total %d bytes; similarity nnz %d, affinity nnz %d"
          % (sum(csr_bytes(d).values()), len(d["similarity_col"]),
             len(d["affinity_col"])), flush=True)
    torch.cuda.reset_peak_memory_stats()
    dt, (items, scores) = timed(
        lambda: model._recommend_arrays(None, 10, True))
    print("_recommend_arrays(None, 10, True)  %9.2f s   peak device memory "
          "%.1f MB (first call: includes upload and the structure check)"
          % (dt, torch.cuda.max_memory_allocated() / 1e6), flush=True)
    dt, _ = timed(lambda: model._recommend_arrays(None, 10, True))
    print("_recommend_arrays, second call     %9.2f s" % dt, flush=True)
    assert items.shape == (n_users, 10) and (items[:, 0] >= 0).all()
    csr = model._csr_on(torch.device("cuda"))
    for t in (4096, 8192, 16384):
        dt, _ = timed(lambda: backend.sar_recommend(
            *csr, None, 10, True, tile=t, check=False))
        print("sar_recommend tile %-5d             %9.2f s" % (t, dt),
              flush=True)


def trace():
    df = frame(50_000, 5_000, 1_000_000, 1)
    model = estimator("sparse").fit(df)
    model._recommend_arrays(None, 10, True)
    model.transform(df[["user", "item"]].head(200_000))
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("a", "b", "sweep", "trace"),
                    default="a")
    args = ap.parse_args()
    assert torch.cuda.is_available() and backend.hip_available()
    {"a": shape_a, "b": shape_b, "sweep": sweep, "trace": trace}[args.shape]()
