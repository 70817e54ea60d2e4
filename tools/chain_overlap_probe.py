#!/usr/bin/env python3
"""Go/no-go probe for running independent split chains of the native GBDT
grower on parallel streams: does one leaf's LDS-atomic-bound histogram
(hist_pair_range_k) overlap with another leaf's HBM-bound partition
(part_arena_count_k + part_arena_scatter_k)?

On one arena it builds the histogram of rows [0, m) and partitions rows
[m, 2m), once back to back on one stream and once on two streams from the
torch pool, for several m.  Device events bracket the work of both streams;
the variants are alternated within every repeat and medians are reported,
with each kernel's time alone and the spread (p10..p90) of every figure:

  python tools/chain_overlap_probe.py [--n-arena 10000000] [--features 100]

With --hist-only M... it times the histogram alone; --threads, --chunk,
--order and --layout force its block width, rows per block, block order and
LDS cell layout (0 / 0 / -1 / -1 leave each to the launcher's policy); with
several --layout values they are alternated within every repeat.  With
--hist-sweep M... it alternates, within every repeat, the policy and every
combination of --sweep-threads, --sweep-chunks, --sweep-orders and --layout,
one JSON line per size and combination:

  python tools/chain_overlap_probe.py --hist-sweep 262144 10000000

With --trace CSV (a rocprofv3 --kernel-trace `*_kernel_trace.csv` of a
training run) it measures nothing and instead reports for how long intervals
of the two kernels overlapped in that run:

  python tools/chain_overlap_probe.py --trace out_kernel_trace.csv --trees 13
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

HIST = "hist_pair_range_k"
SCATTER = "part_arena_scatter_k"


def overlap_ns(a, b):
    """Total length of the intersection of two lists of (start, end)
    intervals; overlaps within one list are merged first."""
    def merged(iv):
        out = []
        for s, e in sorted(iv):
            if out and s <= out[-1][1]:
                out[-1][1] = max(out[-1][1], e)
            else:
                out.append([s, e])
        return out
    a, b = merged(a), merged(b)
    i = j = 0
    total = 0
    while i < len(a) and j < len(b):
        lo, hi = max(a[i][0], b[j][0]), min(a[i][1], b[j][1])
        if hi > lo:
            total += hi - lo
        if a[i][1] < b[j][1]:
            i += 1
        else:
            j += 1
    return total


def trace_report(path, trees):
    iv = {HIST: [], SCATTER: []}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            for k in iv:
                # template instances are named "void hist_pair_range_k<2>(…"
                if name.startswith(k) or name.startswith("void " + k):
                    iv[k].append((int(row["Start_Timestamp"]),
                                  int(row["End_Timestamp"])))
    busy = {k: sum(e - s for s, e in v) for k, v in iv.items()}
    both = overlap_ns(iv[HIST], iv[SCATTER])
    out = {"trace": os.path.basename(path), "trees": trees,
           "hist_calls": len(iv[HIST]), "scatter_calls": len(iv[SCATTER]),
           "hist_ms_per_tree": busy[HIST] / trees / 1e6,
           "scatter_ms_per_tree": busy[SCATTER] / trees / 1e6,
           "hist_scatter_overlap_ms_per_tree": both / trees / 1e6}
    print(json.dumps(out))
    return out


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-arena", type=int, default=10_000_000)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--n-bins", type=int, default=255)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--sizes", type=int, nargs="+",
                    default=[1 << 16, 1 << 18, 1 << 20, 5_000_000])
    ap.add_argument("--hist-only", type=int, nargs="*", default=None,
                    metavar="M", help="only time the histogram alone over "
                    "[0, M) for each M (kernel A/B between two builds)")
    ap.add_argument("--threads", type=int, default=0,
                    help="histogram block width: 256, 512, 1024; 0 = policy")
    ap.add_argument("--chunk", type=int, default=0,
                    help="histogram rows per block; 0 = policy")
    ap.add_argument("--order", type=int, default=-1,
                    help="histogram block order: 0 = (chunks, planes) grid, "
                    "1 = planes of a chunk on one XCD; -1 = policy")
    ap.add_argument("--layout", type=int, nargs="+", default=[-1],
                    help="histogram LDS layout(s): 0 = feature-major, 1 = "
                    "rotated bin-major, 2 = rotated, two copies; -1 = policy")
    ap.add_argument("--hist-sweep", type=int, nargs="*", default=None,
                    metavar="M", help="sweep width x rows per block x order "
                    "of the histogram alone over [0, M) for each M")
    ap.add_argument("--sweep-threads", type=int, nargs="+",
                    default=[256, 512, 1024])
    ap.add_argument("--sweep-chunks", type=int, nargs="+",
                    default=[4096, 16384, 65536])
    ap.add_argument("--sweep-orders", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--trace", default=None,
                    help="rocprofv3 kernel-trace CSV to analyse instead")
    ap.add_argument("--trees", type=int, default=13,
                    help="trees grown in the traced run (warmup + steps)")
    args = ap.parse_args()
    if args.trace:
        trace_report(args.trace, args.trees)
        return

    import torch
    from mmlspark_amd.ops import _hip_grower
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")
    n, nf, nb = args.n_arena, args.features, args.n_bins
    npairs = (nf + 7) // 8
    tail = nf - (npairs - 1) * 8
    torch.manual_seed(0)
    pair = torch.empty(npairs, n, dtype=torch.int64, device=dev)
    for p in range(npairs):  # plane by plane: no (npairs, n, 8) i64 temporary
        pair[p] = torch.randint(0, nb, (n, 8), device=dev,
                                dtype=torch.uint8).view(torch.int64).squeeze(1)
    ghq = torch.stack([
        torch.randint(-2**40, 2**40, (n,), device=dev, dtype=torch.int64),
        torch.randint(0, 2**24, (n,), device=dev, dtype=torch.int64)
        | (1 << 44)], dim=1).contiguous()
    rowid = torch.arange(n, device=dev, dtype=torch.int32)
    dst = (torch.empty_like(pair), torch.empty_like(ghq),
           torch.empty_like(rowid))
    hist = torch.zeros(npairs * 8, nb, 3, dtype=torch.int64, device=dev)
    s_main = torch.cuda.current_stream()
    s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()

    def run_hist(m, threads=args.threads, chunk=args.chunk,
                 order=args.order, layout=args.layout[0]):
        _hip_grower.hist_pair_range(pair, ghq, 0, m, hist, nb, tail,
                                    chunk=chunk, threads=threads, order=order,
                                    layout=layout)

    def run_part(m):
        # threshold at the middle bin of feature 17: about half go left
        _hip_grower.partition_arena(pair, ghq, rowid, *dst, m, m, 17, nb // 2)

    def timed(fn):
        """ms between an event before and an event after fn's device work,
        both on the main stream; fn joins its side streams into it."""
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(s_main)
        fn()
        e1.record(s_main)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def concurrent(m):
        s_a.wait_stream(s_main)
        s_b.wait_stream(s_main)
        with torch.cuda.stream(s_a):
            run_hist(m)
        with torch.cuda.stream(s_b):
            run_part(m)
        s_main.wait_stream(s_a)
        s_main.wait_stream(s_b)

    def on_side_stream(run, m):
        # the same fork/join as `concurrent`, with one of the two kernels
        s_a.wait_stream(s_main)
        with torch.cuda.stream(s_a):
            run(m)
        s_main.wait_stream(s_a)

    if args.hist_only is not None:
        for m in args.hist_only or [1 << 16, n]:
            m = min(m, n)
            for lay in args.layout:
                run_hist(m, layout=lay)
            torch.cuda.synchronize()
            ts = {lay: [] for lay in args.layout}
            for _ in range(args.iters):  # alternate the layouts
                for lay in args.layout:
                    ts[lay].append(
                        timed(lambda: run_hist(m, layout=lay)) * 1e3)
            for lay, v in ts.items():
                print(json.dumps({"m": m, "threads": args.threads,
                                  "chunk": args.chunk, "order": args.order,
                                  "layout": lay,
                                  "hist_alone_us": pct(v, 0.5),
                                  "p10": pct(v, 0.1), "p90": pct(v, 0.9)}),
                      flush=True)
        return

    if args.hist_sweep is not None:
        combos = [(0, 0, -1, -1)] + [
            (t, c, o, lay) for lay in args.layout
            for t in args.sweep_threads for c in args.sweep_chunks
            for o in args.sweep_orders]
        for m in args.hist_sweep or [1 << 18, n]:
            m = min(m, n)
            for cfg in combos:  # warm up every combination
                run_hist(m, *cfg)
            torch.cuda.synchronize()
            ts = {cfg: [] for cfg in combos}
            for _ in range(args.iters):  # alternate them in every repeat
                for cfg in combos:
                    ts[cfg].append(timed(lambda: run_hist(m, *cfg)) * 1e3)
            for (t, c, o, lay), v in ts.items():
                print(json.dumps({
                    "m": m, "threads": t, "chunk": c, "order": o,
                    "layout": lay,
                    "hist_alone_us": round(pct(v, 0.5), 1),
                    "p10": round(pct(v, 0.1), 1),
                    "p90": round(pct(v, 0.9), 1)}), flush=True)
        return

    for m in args.sizes:
        m = min(m, n // 2)
        variants = {
            "hist_alone": lambda: run_hist(m),
            "part_alone": lambda: run_part(m),
            "serial": lambda: (run_hist(m), run_part(m)),
            "hist_side": lambda: on_side_stream(run_hist, m),
            "part_side": lambda: on_side_stream(run_part, m),
            "concurrent": lambda: concurrent(m),
        }
        for fn in variants.values():  # warm up every variant
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in variants}
        for _ in range(args.iters):  # alternate the variants in every repeat
            for k, fn in variants.items():
                ts[k].append(timed(fn) * 1e3)
        out = {"m": m}
        for k, v in ts.items():
            out[k + "_us"] = round(pct(v, 0.5), 1)
            out[k + "_p10_p90"] = [round(pct(v, 0.1), 1),
                                   round(pct(v, 0.9), 1)]
        out["concurrent_over_serial"] = round(
            out["concurrent_us"] / out["serial_us"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
