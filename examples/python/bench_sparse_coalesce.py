#!/usr/bin/env python3
"""Worker-side coalescing of a sparse message: ops.sparse_coalesce (path B,
csrc/sparse_coalesce.hip, preallocated outputs) against the torch path the
embedding example used before it (path A: torch.unique with the inverse,
then index_add_ into a zero tensor).

One process, seeded inputs, row_len 64. Each shape is warmed up, then the
two paths alternate; a call is timed with device events around work that
ends in a synchronise. Prints the median and the spread of each path, the
kernel launches of path B (counted from n and the tile size, not traced)
and the largest relative difference between the two sums: A adds with
atomics in whatever order they land, B in ascending occurrence index.

Needs one MI355X.  Run:  python examples/python/bench_sparse_coalesce.py
"""
import argparse
import json
import sys

sys.path.insert(0, __file__.rsplit("/examples/", 1)[0])
import ps_lite_amd as ps  # noqa: E402
from ps_lite_amd import ops  # noqa: E402

ROW_LEN, TABLE = 64, 1 << 20


def launches(n):
    """kernel launches of one sparse_coalesce with gradients (csrc/sparse_coalesce.hip)"""
    tiles = -(-n // ps._core.coalesce_tile)
    if tiles == 1:
        return 2  # the one-tile kernel, the row sums
    return 1 + (tiles - 1).bit_length() + 3 + 1  # sort, merges, count + scan + emit, row sums


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 65536, 1 << 20])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sparse_coalesce: no GPU")
    gen = torch.Generator().manual_seed(11)
    results = []
    for n in args.sizes:
        for dist in ("uniform", "skewed"):
            u = torch.rand(n, generator=gen, dtype=torch.float64)
            ids = (TABLE * (u if dist == "uniform" else u ** 4)).long().clamp_(max=TABLE - 1).cuda()
            grad = torch.randn(n, ROW_LEN, generator=gen).cuda()
            keys = torch.empty(n, dtype=torch.int64, device="cuda")
            sums = torch.empty(n, ROW_LEN, device="cuda")
            scratch = torch.empty(ps._core.sparse_coalesce_workspace_bytes(n), dtype=torch.uint8,
                                  device="cuda")

            def path_a():
                uniq, inverse = torch.unique(ids, return_inverse=True)
                out = torch.zeros(uniq.numel(), ROW_LEN, device="cuda")
                out.index_add_(0, inverse, grad)
                return uniq, out, inverse

            def path_b():
                return ops.sparse_coalesce(ids, grad, out_keys=keys, out_sums=sums,
                                           workspace=scratch)

            def timed(fn):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                got = fn()
                stop.record()
                torch.cuda.synchronize()
                return start.elapsed_time(stop) * 1e3, got  # microseconds

            for _ in range(args.warmup):
                timed(path_a), timed(path_b)
            ta, tb = [], []
            for _ in range(args.rounds):
                us, a = timed(path_a)
                ta.append(us)
                us, b = timed(path_b)
                tb.append(us)
            same_index = bool(torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]))
            scale = torch.maximum(a[1].abs(), b[1].abs()).clamp_(min=1e-30)
            rel = float(((a[1] - b[1]).abs() / scale).max())
            row = dict(n=n, ids=dist, unique=int(b[0].numel()), launches_b=launches(n),
                       keys_and_inverse_equal=same_index, max_rel_diff_sums=rel)
            for name, t in (("a", sorted(ta)), ("b", sorted(tb))):
                row.update({name + "_us_median": round(t[len(t) // 2], 1),
                            name + "_us_min": round(t[0], 1), name + "_us_max": round(t[-1], 1)})
            results.append(row)
            print("n %8d %-7s unique %7d | A torch %9.1f us [%9.1f, %9.1f] | B hip %9.1f us "
                  "[%9.1f, %9.1f] | B launches %2d | keys+inverse equal %s | max rel diff %.2e"
                  % (n, dist, row["unique"], row["a_us_median"], row["a_us_min"], row["a_us_max"],
                     row["b_us_median"], row["b_us_min"], row["b_us_max"], row["launches_b"],
                     same_index, rel), flush=True)
    print(json.dumps(dict(bench="sparse_coalesce", row_len=ROW_LEN, tile=ps._core.coalesce_tile,
                          rounds=args.rounds, results=results)))


if __name__ == "__main__":
    main()
