"""Arguments the bf16-table kernels and their handler refuse with ValueError before any GPU
call: no GPU and no HBM pool exist here."""
import threading

import pytest

import ps_lite_amd as ps

_ROLES = ("scheduler", "server", "worker")


@pytest.mark.parametrize("lr,beta1,beta2,eps,state,rounding", [
    (0.0, 0.9, 0.999, 1e-8, 0, "nearest"), (0.1, 0.9, 0.999, 0.0, 0, "stochastic"),
    (0.1, 1.0, 0.999, 1e-8, 0, "nearest"), (0.1, 0.9, -0.1, 1e-8, 0, "stochastic"),
    (0.1, 0.9, 0.999, 1e-8, 8, "nearest"), (0.1, 0.9, 0.999, 1e-8, 0, "up")])
def test_bf16_kernels_reject_bad_arguments(lr, beta1, beta2, eps, state, rounding):
    with pytest.raises(ValueError):
        ps._core.k_sparse_lazy_adam_bf16(0, state, 0, 1, 8, 0, 0, lr, beta1, beta2, eps, True,
                                         rounding=rounding, seed=1)
    if beta1 == 0.9 and beta2 == 0.999 and state == 0:  # what Adagrad shares
        with pytest.raises(ValueError):
            ps._core.k_sparse_adagrad_bf16(0, 0, 0, 1, 8, 0, 0, lr, eps, True, rounding=rounding)
    if rounding == "up":
        with pytest.raises(ValueError):
            ps._core.k_sparse_scatter_add_bf16(0, 0, 1, 8, 0, rounding=rounding)


def test_sparse_handle_rejects_bad_bf16_arguments():
    ps.setup_env(1, 1, root_port=30978)
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=-1)) for r in _ROLES]
    [t.start() for t in ths]
    [t.join() for t in ths]
    try:
        server = ps.KVServer(0)
        for bad in [dict(table_dtype="bf16"), dict(table_dtype="bf16", optimizer=None, seed=3),
                    dict(table_dtype="fp16", optimizer="adagrad"),
                    dict(table_dtype="bf16", optimizer="adagrad", rounding="up"),
                    dict(optimizer="adagrad", rounding="nearest"), dict(optimizer="lazy_adam", seed=1),
                    dict(table_dtype="f32", seed=1), dict(table_dtype="bf16", optimizer="adagrad", lr=0.0)]:
            with pytest.raises(ValueError):
                server.set_gpu_sparse_handle(64, 8, **bad)
        server.set_default_handle()
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r in _ROLES]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()
