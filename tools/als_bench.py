"""Fused ALS against the torch formulation on MI355X.

  --shape small  20k users x 5k resources, 500k interactions
  --shape large  200k users x 50k resources, 6M interactions
                 one tenant's factorisation at rank 10 and rank 64, 3
                 iterations: models.cyber._als_csr (als_kernels.hip) against
                 models.cyber._als(..., device="cuda") (the parent formulation:
                 nnz x rank x rank outer products and index_add_), the same
                 explicit triples, both warmed up, alternated in one process,
                 medians with min-max.  Where torch cannot allocate its
                 temporaries the line says so instead of a time.  Implicit mode
                 has no torch counterpart and is timed alone.  Complement
                 sampling and the data frame work of AccessAnomaly.fit are host
                 code common to both and are left out.
  --shape trace  one fused fit of each mode at the small shape and one scoring
                 launch, for a separate `rocprofv3 --kernel-trace --stats --
                 python tools/als_bench.py --shape trace` run

Resources are drawn as floor(n_res * r^2), r uniform: a power-law head, so a
few resource rows are heavy.  Prints text lines; the committed copies are
profiles/als_bench.txt and profiles/als_kernel_stats.txt."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from mmlspark_amd.models.cyber import _als, _als_csr
from mmlspark_amd.ops import backend

SHAPES = {"small": (20_000, 5_000, 500_000), "large": (200_000, 50_000, 6_000_000)}
ITERS = 3


def triples(n_u, n_r, nnz, seed=2):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_u, nnz)
    r = np.minimum((n_r * rng.random(nnz) ** 2).astype(np.int64), n_r - 1)
    u[:n_u], r[:n_r] = np.arange(n_u), np.arange(n_r)   # no id is unused
    return u, r, np.ones(nnz)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def report(name, times):
    ms = np.array(times) * 1e3
    print("%-44s median %10.2f ms   min %10.2f   max %10.2f   (n=%d)"
          % (name, np.median(ms), ms.min(), ms.max(), len(ms)), flush=True)


def compare(shape, rounds):
    n_u, n_r, nnz = SHAPES[shape]
    u, r, y = triples(n_u, n_r, nnz)
    deg = np.bincount(r, minlength=n_r)
    print("shape %s: %d users x %d resources, %d interactions, %d iterations; "
          "largest resource row %d entries, %d rows above the heavy threshold "
          "%d" % (shape, n_u, n_r, nnz, ITERS, deg.max(),
                  (deg > backend._require_ext().als_heavy_degree()).sum(),
                  backend._require_ext().als_heavy_degree()), flush=True)
    for rank in (10, 64):
        def fused(implicit=False):
            return _als_csr(n_u, n_r, u, r, y, rank=rank, iters=ITERS,
                            device="cuda", implicit=implicit)

        def parent():
            return _als(n_u, n_r, u, r, y, rank=rank, iters=ITERS,
                        device="cuda")

        runs = {"fused explicit": fused, "fused implicit": lambda: fused(True),
                "torch explicit (parent)": parent}
        print("rank %d: torch temporaries %.1f GB (nnz x rank x rank floats)"
              % (rank, nnz * rank * rank * 4 / 1e9), flush=True)
        times = {k: [] for k in runs}
        out = {}
        for rnd in range(rounds + 1):            # round 0 warms up
            for name, fn in runs.items():
                if times[name] is None:
                    continue
                try:
                    dt, out[name] = timed(fn)
                except torch.OutOfMemoryError as e:
                    times[name] = None
                    torch.cuda.empty_cache()
                    print("%-44s could not allocate: %s"
                          % ("rank %d, %s" % (rank, name),
                             str(e).split(".")[0]), flush=True)
                    continue
                if rnd:
                    times[name].append(dt)
        for name, t in times.items():
            if t:
                report("rank %d, %s" % (rank, name), t)
        if times["torch explicit (parent)"]:
            a, b = out["fused explicit"], out["torch explicit (parent)"]
            print("rank %d: max |fused - torch| over both factor tables %.3e "
                  "(largest factor %.3e)"
                  % (rank, max(float((a[i] - b[i]).abs().max()) for i in (0, 1)),
                     max(float(b[i].abs().max()) for i in (0, 1))), flush=True)
        out.clear()
        torch.cuda.empty_cache()


def trace():
    n_u, n_r, nnz = SHAPES["small"]
    u, r, y = triples(n_u, n_r, nnz)
    for rank in (10, 64):
        for implicit in (False, True):
            U, V = _als_csr(n_u, n_r, u, r, y, rank=rank, iters=ITERS,
                            device="cuda", implicit=implicit)
    dev = U.device
    zero = torch.zeros(1, dtype=torch.float64, device=dev)
    backend.als_score_pairs(
        U, V, torch.as_tensor(u, dtype=torch.int32, device=dev),
        torch.as_tensor(r, dtype=torch.int32, device=dev),
        torch.zeros(nnz, dtype=torch.int32, device=dev),
        torch.tensor([0, n_u], device=dev), torch.tensor([0, n_r], device=dev),
        zero, zero + 1)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("small", "large", "trace"),
                    default="small")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available() and backend.hip_available()
    if args.shape == "trace":
        trace()
    else:
        compare(args.shape, args.rounds)
