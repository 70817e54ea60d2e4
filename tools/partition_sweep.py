#!/usr/bin/env python3
"""Sweep the arena partition's launch policy (rows per block x plane groups)
over leaf sizes, to set PART_CHUNK_DEFAULT / PART_SPLIT_PLANES_BELOW in
ops/hip/gbdt_kernels.hip.  Prints one line per (m, chunk, groups): median
microseconds of count + scatter and the achieved payload rate at 256 B per
row moved (124 B read + 124 B written + the split plane read by the count).

  python tools/partition_sweep.py [--npairs 13] [--n-arena 10000000]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npairs", type=int, default=13)
    ap.add_argument("--n-arena", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--chunks", type=int, nargs="+",
                    default=[1024, 2048, 4096, 8192])
    ap.add_argument("--groups", type=int, nargs="+", default=None,
                    help="plane-group counts (default 1 2 4 npairs)")
    ap.add_argument("--sizes", type=int, nargs="+", default=None)
    args = ap.parse_args()
    from mmlspark_amd.ops import _hip_grower
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")
    n, npairs = args.n_arena, args.npairs
    torch.manual_seed(0)
    src = (torch.randint(0, 2**62, (npairs, n), device=dev, dtype=torch.int64),
           torch.randint(0, 2**40, (n, 2), device=dev, dtype=torch.int64),
           torch.arange(n, device=dev, dtype=torch.int32))
    dst = tuple(torch.empty_like(t) for t in src)
    sizes = args.sizes or [1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22, n]
    chunks = args.chunks
    groups = args.groups or sorted({1, 2, 4, npairs})
    for m in sizes:
        m = min(m, n)
        best = None
        for chunk in [0] + chunks:
            for g in ([0] if chunk == 0 else groups):
                def run():
                    _hip_grower.partition_arena(*src, *dst, 0, m, 17, 127,
                                                None, chunk, g)
                run()
                torch.cuda.synchronize()
                ts = []
                for _ in range(args.iters):
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                us = sorted(ts)[len(ts) // 2]
                tbs = m * 256 / (us * 1e-6) / 1e12
                tag = "policy" if chunk == 0 else f"chunk={chunk} groups={g}"
                print(f"m={m:>9} {tag:<24} {us:9.1f} us  {tbs:5.2f} TB/s",
                      flush=True)
                if chunk and (best is None or us < best[0]):
                    best = (us, tag)
        print(f"m={m:>9} best: {best[1]} ({best[0]:.1f} us)", flush=True)


if __name__ == "__main__":
    main()
