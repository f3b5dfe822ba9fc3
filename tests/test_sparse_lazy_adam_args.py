"""Arguments the lazy-Adam step and its handler refuse with ValueError before any GPU call: no
GPU and no HBM pool exist here."""
import threading

import pytest

import ps_lite_amd as ps

_ROLES = ("scheduler", "server", "worker")


@pytest.mark.parametrize("lr,beta1,beta2,eps,state", [
    (0.0, 0.9, 0.999, 1e-8, 0), (-0.1, 0.9, 0.999, 1e-8, 0), (0.1, 0.9, 0.999, 0.0, 0),
    (0.1, 0.9, 0.999, -1e-8, 0), (0.1, 1.0, 0.999, 1e-8, 0), (0.1, -0.1, 0.999, 1e-8, 0),
    (0.1, 0.9, 1.0, 1e-8, 0), (0.1, 0.9, -0.1, 1e-8, 0), (0.1, 0.9, 0.999, 1e-8, 8)])
def test_lazy_adam_kernel_rejects_bad_arguments(lr, beta1, beta2, eps, state):
    with pytest.raises(ValueError):
        ps._core.k_sparse_lazy_adam_f32(0, state, 0, 1, 4, 0, 0, lr, beta1, beta2, eps, True)


def test_lazy_adam_state_floats():
    assert ps._core.sparse_lazy_adam_state_floats(64, 5, False) == 64 * 14
    assert ps._core.sparse_lazy_adam_state_floats(64, 5, True) == 64 * 9


def test_sparse_handle_rejects_bad_lazy_adam_arguments():
    ps.setup_env(1, 1, root_port=30964)
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=-1)) for r in _ROLES]
    [t.start() for t in ths]
    [t.join() for t in ths]
    try:
        server = ps.KVServer(0)
        for bad in [dict(optimizer="lazy_adam", beta1=1.0), dict(optimizer="lazy_adam", beta2=-0.1),
                    dict(optimizer="lazy_adam", init_acc=0.5), dict(optimizer="lazy_adam", lr=0.0),
                    dict(optimizer="rowwise_lazy_adam", eps=0.0)]:
            with pytest.raises(ValueError):
                server.set_gpu_sparse_handle(64, 4, **bad)
        server.set_default_handle()
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r in _ROLES]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()
