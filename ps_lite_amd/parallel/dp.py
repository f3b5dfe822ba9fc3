"""Data-parallel gradient synchronization through the parameter server
(the BytePS training pattern, BASELINE config #4).

Each worker pushes its gradient buckets (tensors split into
<= partition_bytes chunks, the reference's BYTEPS_PARTITION_BYTES
mechanism) and pulls back the cross-worker reduction, then scales by
1/num_workers.

Two server modes:
  * "reduce" (GPU, recommended): servers run the dense handler in
    reduce mode — pulls are held until every worker's push of the round
    arrived, so NO barrier is needed and pushes/pulls of all buckets
    overlap fully.
  * "sum" (CPU demo / default handler): the store accumulates forever,
    so keys rotate every step and a worker barrier separates the push
    and pull phases.
"""

import numpy as np


class PSGradSync:
    def __init__(self, ps, worker, params, num_workers, device=-1,
                 partition_bytes=4 << 20, mode=None, key_base=1 << 20, compress=None,
                 mx_batched=True):
        if compress not in (None, "mxfp8"):
            raise ValueError(f"unknown compress={compress!r} (None or 'mxfp8')")
        if compress and (device < 0 or (mode or "reduce") != "reduce"):
            raise ValueError("compress='mxfp8' needs a GPU (device >= 0) and reduce mode")
        self.compress = compress
        # compress="mxfp8" only: quantize and dequantize all buckets in one
        # launch per 64 (True) or one launch per bucket (False, the A/B)
        self.mx_batched = bool(mx_batched)
        # worker-side quantize and dequantize launches so far
        self.mx_launches = 0
        self.ps = ps
        self.worker = worker
        self.params = list(params)
        self.num_workers = num_workers
        self.device = device
        self.mode = mode or ("reduce" if device >= 0 else "sum")
        self.key_base = key_base
        self.step_count = 0

        # bucket layout: (param_idx, elem_offset, elems)
        self.buckets = []
        max_elems = partition_bytes // 4
        for pi, p in enumerate(self.params):
            n = p.numel()
            off = 0
            while off < n:
                take = min(max_elems, n - off)
                self.buckets.append((pi, off, take))
                off += take
        self.bufs = []
        self.pull_bufs = []
        # direct mode (decided on first allreduce): when .grad tensors
        # are pool-resident (ps.use_torch_pool_allocator()), push/pull
        # straight from grad memory — no staging buffers, no copies
        self.direct = None
        for _, _, elems in self.buckets:
            if compress:
                # packed push and pull buffers (servers: dtype="mxfp8");
                # grads are quantized from and dequantized into .grad
                nbytes = ps._core.mxfp8_packed_nbytes(elems)
                self.bufs.append(ps.pool_alloc(nbytes))
                self.pull_bufs.append(ps.pool_alloc(nbytes))
            elif device >= 0:
                self.bufs.append(ps.pool_alloc(elems * 4))
                self.pull_bufs.append(ps.pool_alloc(elems * 4))
            else:
                self.bufs.append(np.zeros(elems, dtype=np.float32))
                self.pull_bufs.append(np.zeros(elems, dtype=np.float32))

    def _keys(self):
        if self.mode == "reduce":
            base = self.key_base
        else:
            base = self.key_base + self.step_count * len(self.buckets)
        return [base + i for i in range(len(self.buckets))]

    def _ptr(self, buf):
        return buf.ptr if self.device >= 0 else buf.ctypes.data

    def _grad_view(self, b):
        pi, off, elems = self.buckets[b]
        return self.params[pi].grad.detach().reshape(-1)[off:off + elems]

    def _allreduce_mxfp8(self):
        """The reduce round on MXFP8 payloads (528 bytes per 512 elements
        each way): quantize from .grad, push and pull packed bytes,
        dequantize into .grad with the 1/num_workers scale folded in.
        The servers run set_gpu_dense_handle(mode="reduce", dtype="mxfp8")."""
        core = self.ps._core
        keys = self._keys()
        nb = len(self.buckets)
        if self.mx_batched:
            # grads may be reallocated between steps: pointers are read now
            gptrs = [self._grad_view(b).data_ptr() for b in range(nb)]
            self.mx_launches += core.k_batched_mx_quantize(
                [(gptrs[b], self.bufs[b].ptr, self.buckets[b][2]) for b in range(nb)])
        tss = []
        for b, k in enumerate(keys):
            elems = self.buckets[b][2]
            nbytes = core.mxfp8_packed_nbytes(elems)
            if not self.mx_batched:
                core.k_mx_quantize(self._grad_view(b).data_ptr(), elems, self.bufs[b].ptr)
                self.mx_launches += 1
            ka = np.array([k], dtype=np.uint64)
            lens = np.array([nbytes // 4], dtype=np.int32)
            tss.append(self.worker.zpush_ptr(ka, self.bufs[b].ptr, nbytes, self.device, lens,
                                             cmd=2))
            tss.append(self.worker.zpull_ptr(ka, self.pull_bufs[b].ptr, nbytes, self.device,
                                             lens))
        for ts in tss:
            self.worker.wait(ts)
        inv = 1.0 / self.num_workers
        if self.mx_batched:
            self.mx_launches += core.k_batched_mx_dequantize(
                [(gptrs[b], self.pull_bufs[b].ptr, self.buckets[b][2]) for b in range(nb)], inv)
        else:
            for b in range(nb):
                elems = self.buckets[b][2]
                core.k_mx_dequantize(self.pull_bufs[b].ptr, elems, self._grad_view(b).data_ptr(),
                                     inv)
                self.mx_launches += 1
        self.step_count += 1

    def allreduce(self):
        """Average .grad across workers, in place. Call after backward."""
        import torch

        if self.compress:
            self._allreduce_mxfp8()
            return
        if self.direct is None:
            # direct (zero-staging) mode needs every grad bucket inside
            # the zero-copy pool window AND reduce-mode servers (pulls
            # write grads in place)
            self.direct = (self.device >= 0 and self.mode == "reduce" and
                           all(self.ps._core.pool_contains(self._grad_view(b).data_ptr())
                               for b in range(len(self.buckets))))
        keys = self._keys()
        # stage grads into the push buffers (skipped in direct mode)
        if not self.direct:
            for b, (pi, off, elems) in enumerate(self.buckets):
                g = self._grad_view(b)
                if self.device >= 0:
                    # pool buffer <- device grad (same GPU)
                    self.ps._core.k_dense_assign(self.bufs[b].ptr, g.data_ptr(), elems * 4)
                else:
                    self.bufs[b][:] = g.cpu().numpy()
        tss = []
        for b, k in enumerate(keys):
            ka = np.array([k], dtype=np.uint64)
            elems = self.buckets[b][2]
            lens = np.array([elems], dtype=np.int32)
            if self.direct:
                gptr = self._grad_view(b).data_ptr()
                tss.append(self.worker.zpush_ptr(ka, gptr, elems * 4, self.device, lens,
                                                 cmd=2))
                # the reduction is written straight back into .grad
                tss.append(self.worker.zpull_ptr(ka, gptr, elems * 4, self.device, lens))
                continue
            tss.append(self.worker.zpush_ptr(ka, self._ptr(self.bufs[b]), elems * 4,
                                             self.device, lens, cmd=2))
            if self.mode == "reduce":
                tss.append(self.worker.zpull_ptr(ka, self._ptr(self.pull_bufs[b]), elems * 4,
                                                 self.device, lens))
        if self.mode != "reduce":
            for ts in tss:
                self.worker.wait(ts)
            tss = []
            self.ps.barrier("worker", self.ps.WORKER_GROUP)
            for b, k in enumerate(keys):
                ka = np.array([k], dtype=np.uint64)
                elems = self.buckets[b][2]
                lens = np.array([elems], dtype=np.int32)
                tss.append(self.worker.zpull_ptr(ka, self._ptr(self.pull_bufs[b]), elems * 4,
                                                 self.device, lens))
        for ts in tss:
            self.worker.wait(ts)
        # scale to the average (direct mode: the reduction already sits
        # in .grad — the pull wrote it in place over xGMI)
        inv = 1.0 / self.num_workers
        for b, (pi, off, elems) in enumerate(self.buckets):
            g = self._grad_view(b)
            if self.direct:
                g.mul_(inv)
            elif self.device >= 0:
                self.ps._core.k_dense_assign(g.data_ptr(), self.pull_bufs[b].ptr, elems * 4)
                g.mul_(inv)
            else:
                g.copy_(torch.from_numpy(self.pull_bufs[b] * inv))
        self.step_count += 1
