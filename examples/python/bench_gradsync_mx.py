#!/usr/bin/env python3
"""Step-level A/B of PSGradSync(compress="mxfp8"): worker-side quantize and
dequantize batched (one launch per 64 buckets) against one launch per
bucket. One scheduler plus one joint worker+server process on GPU 0; the
parameters have the sizes of ResNet-50 (--params small: a four-entry list
that runs in a second). Two PSGradSync objects on disjoint keys take turns:
3 warm-up steps each, then 20 timed steps each, alternating. A step is
allreduce() plus torch.cuda.synchronize() under time.perf_counter.

This is a one-GPU number: what the worker pays per step around the
messages. It says nothing about the format's gain on a link between GPUs.

Run:  python examples/python/bench_gradsync_mx.py [--params rn50|small]
"""
import argparse
import statistics
import sys
import threading
import time

sys.path.insert(0, __file__.rsplit("/examples/", 1)[0])

SMALL = (1000, 37, 513, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", choices=("rn50", "small"), default="rn50")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--port", type=int, default=32900)
    args = ap.parse_args()

    import torch

    import ps_lite_amd as ps
    from ps_lite_amd.models.resnet50_buckets import resnet50_param_sizes
    from ps_lite_amd.parallel.dp import PSGradSync

    if not torch.cuda.is_available():
        sys.exit("bench_gradsync_mx.py needs a GPU")
    sizes = SMALL if args.params == "small" else tuple(resnet50_param_sizes())

    ps.setup_env(1, 1, root_port=args.port, XPS_DEV_ID=0, XPS_POOL_GB=4)
    roles = (("scheduler", -1), ("joint", 0))
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=d)) for r, d in roles]
    [t.start() for t in ths]
    [t.join() for t in ths]
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="reduce", dtype="mxfp8")
        worker = ps.KVWorker(0, 0)
        g = torch.Generator().manual_seed(1)
        params = [torch.nn.Parameter(torch.zeros(n, device="cuda:0")) for n in sizes]
        for p in params:
            p.grad = torch.randn(p.numel(), generator=g).to("cuda:0")
        syncs = {}
        for i, batched in enumerate((True, False)):
            syncs[batched] = PSGradSync(ps, worker, params, num_workers=1, device=0,
                                        compress="mxfp8", mx_batched=batched,
                                        key_base=(1 + i) << 20)
        times = {True: [], False: []}
        launches = {}
        for step in range(args.warmup + args.steps):
            for batched in (True, False):
                sync = syncs[batched]
                before = sync.mx_launches
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sync.allreduce()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                launches[batched] = sync.mx_launches - before
                if step >= args.warmup:
                    times[batched].append(dt * 1e3)
        nb = len(syncs[True].buckets)
        print(f"# {args.params}: {len(sizes)} params, {nb} buckets, {args.steps} timed steps "
              f"each after {args.warmup} warm-up, alternating")
        for batched in (True, False):
            t = times[batched]
            print(f"mx_batched={str(batched):5s}  allreduce median {statistics.median(t):8.3f} ms  "
                  f"range {min(t):8.3f} .. {max(t):8.3f} ms  "
                  f"mx_launches per step {launches[batched]}")
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r, _ in roles]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()


if __name__ == "__main__":
    main()
