"""The SGD entry points of the C ABI and the host side of vae2.optim.FusedSGD: symbols,
host-side argument validation (-22 before any launch), constructor checks and the poly
learning-rate schedule.  No compute calls: runs without a GPU."""
import ctypes

import pytest
import torch

from helpers import GOLDEN  # noqa: F401  (puts the package on sys.path via conftest)

SYMS = ("vae2_sgd_coeffs", "vae2_sgd_step_dev", "vae2_sgd_step")
P = ctypes.c_void_p(16)  # dummy non-null pointer: validation fails before it is used


def test_sgd_symbols_typed_and_exported():
    from vae2 import _lib
    lib = _lib.load()
    for name in SYMS:
        assert name in _lib.exported_symbols()
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes
    assert _lib.ABI_VERSION >= 13 and lib.vae2_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("n,buf,momentum,nesterov,what", [
    (-1, P, 0.9, 0, b"bad arguments"),
    (8, P, 0.0, 1, b"nesterov"),
    (8, None, 0.9, 0, b"momentum buffer"),
])
def test_sgd_step_dev_rejects_bad_arguments(n, buf, momentum, nesterov, what):
    from vae2 import _lib
    lib = _lib.load()
    # (p, g, buf, n, coeffs, momentum, weight_decay, nesterov, stream)
    rc = lib.vae2_sgd_step_dev(P, P, buf, n, P, momentum, 0.0, nesterov, None)
    assert rc == -22
    err = lib.vae2_last_error()
    assert b"vae2_sgd_step_dev" in err and what in err, err


def test_sgd_nesterov_with_dampening_rejected():
    from vae2 import _lib
    lib = _lib.load()
    # (state, momentum, dampening, nesterov, coeffs, stream)
    rc = lib.vae2_sgd_coeffs(P, 0.9, 0.1, 1, P, None)
    assert rc == -22
    assert b"vae2_sgd_coeffs" in lib.vae2_last_error() and b"nesterov" in lib.vae2_last_error()
    # (p, g, buf, n, lr, momentum, dampening, weight_decay, nesterov, first_step, stream)
    rc = lib.vae2_sgd_step(P, P, P, 8, 0.1, 0.9, 0.1, 0.0, 1, 0, None)
    assert rc == -22
    assert b"vae2_sgd_step" in lib.vae2_last_error() and b"nesterov" in lib.vae2_last_error()
    # negative momentum / weight decay, in every form
    assert lib.vae2_sgd_step(P, P, P, 8, 0.1, -0.5, 0.0, 0.0, 0, 0, None) == -22
    assert lib.vae2_sgd_step(P, P, P, 8, 0.1, 0.5, 0.0, -1.0, 0, 0, None) == -22
    assert lib.vae2_sgd_step_dev(P, P, P, 8, P, 0.5, -1.0, 0, None) == -22
    assert lib.vae2_sgd_coeffs(P, -0.5, 0.0, 0, P, None) == -22


@pytest.mark.parametrize("kw,msg", [
    (dict(lr=0.1, momentum=0.0, nesterov=True), "Nesterov"),
    (dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True), "Nesterov"),
    (dict(lr=-0.1), "learning rate"),
    (dict(lr=0.1, momentum=-0.9), "momentum"),
    (dict(lr=0.1, weight_decay=-1e-4), "weight_decay"),
])
def test_fused_sgd_constructor_validation(kw, msg):
    from vae2.optim import FusedSGD
    with pytest.raises(ValueError, match=msg):
        FusedSGD(torch.nn.Linear(3, 2), **kw)
    with pytest.raises(ValueError, match=msg):  # torch's own rule, same message
        torch.optim.SGD(torch.nn.Linear(3, 2).parameters(), **kw)


def test_adjust_learning_rate_poly_schedule():
    import os
    import sys
    lib_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "vae-2_amd", "lib")
    if lib_dir not in sys.path:
        sys.path.insert(0, lib_dir)
    from utils.utils import adjust_learning_rate  # the drop-in surface
    from vae2 import trainer
    assert adjust_learning_rate is trainer.adjust_learning_rate
    opt = torch.optim.SGD(torch.nn.Linear(3, 2).parameters(), lr=1.0)
    lr = adjust_learning_rate(opt, 0.01, 200, 50)
    assert lr == 0.01 * (1 - 50 / 200) ** 0.9
    assert opt.param_groups[0]["lr"] == lr
    assert adjust_learning_rate(opt, 0.01, 200, 0) == 0.01
    assert adjust_learning_rate(opt, 0.01, 200, 100, power=2.0) == 0.01 * 0.25
