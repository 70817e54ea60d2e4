#!/usr/bin/env python3
"""Where a boosting step's time goes at the two ends of its tree, from a
rocprofv3 --kernel-trace CSV (`*_kernel_trace.csv`) of a bench.py run:

  rocprofv3 --kernel-trace -d out -o run -- python bench.py --steps 12 --warmup 3
  python tools/tree_ends_trace.py out/*/run_kernel_trace.csv --label parent

Every tree ends with exactly one apply_leaf_values_k, so the kernels of tree
t are those that start after tree t-1's apply_leaf_values_k ended, up to and
including its own.  The first tree of the trace is dropped: its window would
begin somewhere in the data set-up.  Per tree, in microseconds:

  step        first kernel of the step to the first kernel of the next
  busy        union over all streams of the time some kernel is running
  head        first kernel of the step to the start of the first
              part_arena_count_k (the root split's)
  head_busy   busy time inside the head
  tail        end of the last chain kernel (count, scatter, histogram,
              scan) to the first kernel of the next step
  idle_before_apply / idle_after_apply
              time inside the tail with no kernel running, before
              apply_leaf_values_k starts and after it ends
  hist, scan, gather, sum_long
              calls (and time) of hist_pair_range_k, sibling_scan_k,
              arena_gather_k and torch's int64 sum reduction in the tree

One JSON line per tree with --per-tree, then one line of medians.
"""
import argparse
import csv
import json
import os
import statistics

CHAIN = ("part_arena_count_k", "part_arena_scatter_k", "hist_pair_range_k",
         "sibling_scan_k")
APPLY = "apply_leaf_values_k"
COUNT = "part_arena_count_k"


def is_kernel(name, k):
    # template instances are named "void hist_pair_range_k<2>(…"
    return name.startswith(k) or name.startswith("void " + k)


def busy_ns(iv, lo=None, hi=None):
    """Length of the union of (start, end) intervals, clipped to [lo, hi]."""
    total, cur_s, cur_e = 0, None, None
    for s, e in sorted(iv):
        if lo is not None:
            s = max(s, lo)
        if hi is not None:
            e = min(e, hi)
        if e <= s:
            continue
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                total += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    if cur_e is not None:
        total += cur_e - cur_s
    return total


def load(path):
    ks = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            ks.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]),
                       row["Kernel_Name"]))
    ks.sort()
    return ks


def tree_windows(ks):
    """Kernel lists per tree, split after every apply_leaf_values_k."""
    trees, cur = [], []
    for k in ks:
        cur.append(k)
        if is_kernel(k[2], APPLY):
            trees.append(cur)
            cur = []
    return trees[1:], cur  # first window starts in the set-up; drop it


def tree_report(tree, next_start):
    t0 = tree[0][0]
    iv = [(s, e) for s, e, _ in tree]
    apply_s, apply_e, _ = tree[-1]
    counts = [k for k in tree if is_kernel(k[2], COUNT)]
    chain_end = max((e for s, e, n in tree
                     if any(is_kernel(n, c) for c in CHAIN)), default=t0)
    out = {"step_us": (next_start - t0) / 1e3,
           "busy_us": busy_ns(iv) / 1e3,
           "tail_us": (next_start - chain_end) / 1e3,
           "idle_before_apply_us":
               (apply_s - chain_end - busy_ns(iv, chain_end, apply_s)) / 1e3,
           "apply_us": (apply_e - apply_s) / 1e3,
           "idle_after_apply_us": (next_start - apply_e) / 1e3}
    if counts:
        head_end = counts[0][0]
        out["head_us"] = (head_end - t0) / 1e3
        out["head_busy_us"] = busy_ns(iv, t0, head_end) / 1e3
    for key, name in (("hist", "hist_pair_range_k"),
                      ("scan", "sibling_scan_k"),
                      ("gather", "arena_gather_k"),
                      ("sum_long", "sum_functor<long")):
        sel = [(s, e) for s, e, n in tree
               if (name in n if "<" in name else is_kernel(n, name))]
        out[key + "_calls"] = len(sel)
        out[key + "_us"] = sum(e - s for s, e in sel) / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace", help="rocprofv3 kernel-trace CSV")
    ap.add_argument("--label", default=None,
                    help="recorded in every line (e.g. parent, result)")
    ap.add_argument("--per-tree", action="store_true")
    args = ap.parse_args()

    trees, rest = tree_windows(load(args.trace))
    # the last tree's window needs the first kernel of a following step
    reports = []
    for i, tree in enumerate(trees):
        nxt = trees[i + 1] if i + 1 < len(trees) else rest
        if not nxt:
            break
        reports.append(tree_report(tree, nxt[0][0]))
    base = {"trace": os.path.basename(args.trace)}
    if args.label:
        base["label"] = args.label
    if args.per_tree:
        for i, r in enumerate(reports):
            print(json.dumps({**base, "tree": i + 1,
                              **{k: round(v, 1) for k, v in r.items()}}))
    keys = sorted({k for r in reports for k in r})
    med = {k: round(statistics.median(r[k] for r in reports if k in r), 1)
           for k in keys}
    print(json.dumps({**base, "trees": len(reports), "median": med}))


if __name__ == "__main__":
    main()
