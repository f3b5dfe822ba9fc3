"""Arguments the sparse optimizer refuses with ValueError before any GPU call: no GPU and
no HBM pool exist here."""
import threading

import pytest

import ps_lite_amd as ps

_ROLES = ("scheduler", "server", "worker")


def test_adagrad_kernel_rejects_bad_rates():
    for lr, eps in [(0.0, 1e-8), (-0.1, 1e-8), (0.1, 0.0), (0.1, -1e-8)]:
        with pytest.raises(ValueError):
            ps._core.k_sparse_adagrad_f32(0, 0, 0, 1, 4, 0, 0, lr, eps, True)


def test_sparse_handle_rejects_bad_optimizer_arguments():
    ps.setup_env(1, 1, root_port=30950)
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=-1)) for r in _ROLES]
    [t.start() for t in ths]
    [t.join() for t in ths]
    try:
        server = ps.KVServer(0)
        for bad in [dict(optimizer="adam"), dict(optimizer="adagrad", lr=0.0),
                    dict(optimizer="adagrad", lr=-1.0), dict(optimizer="rowwise_adagrad", eps=0.0),
                    dict(optimizer="rowwise_adagrad", eps=-1e-8),
                    dict(optimizer="adagrad", init_acc=-0.5)]:
            with pytest.raises(ValueError):
                server.set_gpu_sparse_handle(64, 4, **bad)
        server.set_default_handle()
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r in _ROLES]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()
