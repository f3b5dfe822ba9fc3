#!/usr/bin/env python3
"""Embedding-bag regression with the optimizer on the server: the table
lives in the sparse handler, the optimizer step (row-wise Adagrad unless
--optimizer names another) runs there, and a training step is ONE fused
zpushpull_ptr.

Each sample is a bag of row ids whose embeddings are summed and regressed
onto the sum of a hidden table's rows. A step's message carries the
gradients of the current batch and, with zero gradients (a zero step), the
rows the next batch will read; the response is those rows after the
update, so the next forward pass needs no pull of its own. The handler
wants sorted unique rows in a message: one sparse_coalesce per step turns
the ids of both batches and the per-occurrence gradients into the keys,
the summed rows (written straight into the pool tensor) and the slot of
every occurrence, and one sparse_gather turns the response back into
per-occurrence rows.

Needs one MI355X.  Run:  python examples/python/train_embedding.py
                        [--optimizer rowwise_adagrad|adagrad|lazy_adam|rowwise_lazy_adam]
                        [--table-dtype f32|bf16] [--wire-dtype f32|bf16]
--table-dtype bf16 keeps the table in bf16 (half the bytes per row) with
stochastic rounding on every store; the messages stay fp32 unless
--wire-dtype bf16 (needs the bf16 table) halves them too: sparse_coalesce
rounds the summed gradients into the pushed tensor, the response is the
table's bf16 rows, and sparse_gather widens them per occurrence.
"""
import argparse
import sys
import threading

import numpy as np

sys.path.insert(0, __file__.rsplit("/examples/", 1)[0])
import ps_lite_amd as ps  # noqa: E402
from ps_lite_amd import ops  # noqa: E402

ROWS, DIM, BATCH, BAG, STEPS = 512, 32, 256, 4, 60
# learning rates at which the loss falls well within STEPS: Adam's step is
# about lr per element whatever the gradient's scale
LR = {"adagrad": 0.1, "rowwise_adagrad": 0.1, "lazy_adam": 0.05, "rowwise_lazy_adam": 0.05}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--optimizer", default="rowwise_adagrad", choices=sorted(LR))
    ap.add_argument("--table-dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--wire-dtype", default="f32", choices=["f32", "bf16"])
    args = ap.parse_args()
    if args.wire_dtype == "bf16" and args.table_dtype != "bf16":
        ap.error("--wire-dtype bf16 needs --table-dtype bf16")
    optimizer = args.optimizer
    ps.setup_env(1, 1, root_port=9310, XPS_DEV_ID=0, XPS_POOL_GB=1)
    roles = (("scheduler", -1), ("joint", 0))
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=d)) for r, d in roles]
    [t.start() for t in ths]
    [t.join() for t in ths]
    server = ps.KVServer(0)
    server.set_gpu_sparse_handle(ROWS, DIM, optimizer=optimizer, lr=LR[optimizer], eps=1e-8,
                                 table_dtype=args.table_dtype, wire_dtype=args.wire_dtype)
    worker = ps.KVWorker(0, 0)

    gen = torch.Generator().manual_seed(3)
    hidden = torch.randn(ROWS, DIM, generator=gen).cuda()
    bags = torch.randint(0, ROWS, (STEPS + 1, BATCH, BAG), generator=gen).cuda()
    cap = 2 * BATCH * BAG  # rows of two batches at the most
    wire16 = args.wire_dtype == "bf16"
    pool = [ps.pool_tensor((cap, DIM), "int16" if wire16 else "float32") for _ in range(2)]
    # a 16-bit wire: bf16 views of pool tensors of half the bytes (`pool` keeps them alive)
    vals, out = (p.view(torch.bfloat16) for p in pool) if wire16 else pool
    row_bytes = DIM * vals.element_size()

    keys_buf = torch.empty(cap, dtype=torch.int64, device="cuda")
    scratch = torch.empty(ps._core.sparse_coalesce_workspace_bytes(cap), dtype=torch.uint8,
                          device="cuda")

    def round_trip(ids, cmd=0):
        """push vals[:n] for the n sorted unique ids, return their rows afterwards"""
        n = ids.numel()
        torch.cuda.synchronize()
        keys = ids.cpu().numpy().astype(np.uint64)
        lens = np.full(n, row_bytes // 4, dtype=np.int32)  # lens count floats
        worker.wait(worker.zpushpull_ptr(keys, vals.data_ptr(), out.data_ptr(), n * row_bytes, 0,
                                         lens, cmd=cmd))
        return out[:n].clone()

    vals[:ROWS] = 0.1 * torch.randn(ROWS, DIM, generator=gen).cuda()
    round_trip(torch.arange(ROWS, device="cuda"), cmd=1)  # initial weights
    ids, _, at = ops.sparse_coalesce(bags[0], out_keys=keys_buf, workspace=scratch)
    vals[:ids.numel()] = 0.0
    rows = round_trip(ids)  # a zero step: a pull
    losses = []
    for step in range(STEPS):
        bag = bags[step]
        # `at`: where each occurrence's row sits in `rows`
        err = ops.sparse_gather(rows, at).view(BATCH, BAG, DIM).sum(dim=1) - hidden[bag].sum(dim=1)
        losses.append(float((err * err).mean()))
        # d loss / d row, one term per occurrence of this batch; the message
        # names the ids of this batch and the next, coalesced per unique id
        per_use = ((2.0 / err.numel()) * err)[:, None, :].expand(BATCH, BAG, DIM).reshape(-1, DIM)
        ids, _, inverse = ops.sparse_coalesce(bags[step:step + 2], grad=per_use, out_keys=keys_buf,
                                              out_sums=vals, workspace=scratch)
        at = inverse[BATCH * BAG:]  # the next batch's occurrences
        rows = round_trip(ids)
        if step % 10 == 0 or step == STEPS - 1:
            print("step %2d  loss %.4f" % (step, losses[-1]))

    ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r, _ in roles]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert losses[-1] < 0.5 * losses[0], "the loss did not fall"
    print("loss %.4f -> %.4f with %s on the server, %s table, %s wire"
          % (losses[0], losses[-1], optimizer, args.table_dtype, args.wire_dtype))


if __name__ == "__main__":
    main()
