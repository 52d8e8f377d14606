"""The weight-EMA entry points of the C ABI (ABI 15) and the host side of ema_decay in
vae2.optim: symbols, host-side argument validation (-22 before any launch), constructor
checks and the MI355X.EMA_DECAY / MI355X.EVAL_EMA config keys.  No compute calls: runs
without a GPU."""
import ctypes
import os
import re
import sys

import pytest
import torch

from helpers import GOLDEN  # noqa: F401  (puts the package on sys.path via conftest)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("vae2_ema_coeffs", "vae2_ema_update_dev", "vae2_ema_update")
P = ctypes.c_void_p(16)  # dummy non-null pointers: validation fails before they are used
Q = ctypes.c_void_p(32)
INF, NAN = float("inf"), float("nan")


def _lib():
    from vae2 import _lib
    return _lib.load()


def test_ema_symbols_typed_exported_and_declared():
    from vae2 import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vae2_hip.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMS:
        assert name in _lib.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes
        assert fn.restype is ctypes.c_int
        assert re.search(r"\b%s\s*\(" % name, decls), name
    assert _lib.ABI_VERSION >= 15 and lib.vae2_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define VAE2_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION


def _rejected(rc, lib, fn):
    assert rc == -22
    err = lib.vae2_last_error()
    assert fn.encode() in err, err


@pytest.mark.parametrize("state,decay,coeffs", [
    (None, 0.9, P), (P, 0.9, None),
    (P, NAN, Q), (P, -0.1, Q), (P, 1.0, Q), (P, 1.5, Q), (P, INF, Q), (P, -INF, Q),
])
def test_ema_coeffs_rejects_bad_arguments(state, decay, coeffs):
    lib = _lib()
    _rejected(lib.vae2_ema_coeffs(state, decay, coeffs, None), lib, "vae2_ema_coeffs")


@pytest.mark.parametrize("ema,p,n,coeffs", [
    (P, Q, -1, P), (None, Q, 8, P), (P, None, 8, P), (P, Q, 8, None), (P, P, 8, Q),
])
def test_ema_update_dev_rejects_bad_arguments(ema, p, n, coeffs):
    lib = _lib()
    _rejected(lib.vae2_ema_update_dev(ema, p, n, coeffs, None), lib, "vae2_ema_update_dev")


@pytest.mark.parametrize("ema,p,n,decay", [
    (P, Q, -1, 0.9), (None, Q, 8, 0.9), (P, None, 8, 0.9), (P, P, 8, 0.9),
    (P, Q, 8, NAN), (P, Q, 8, -0.1), (P, Q, 8, 1.0), (P, Q, 8, INF),
])
@pytest.mark.parametrize("first", [0, 1])
def test_ema_update_rejects_bad_arguments(ema, p, n, decay, first):
    lib = _lib()
    _rejected(lib.vae2_ema_update(ema, p, n, decay, first, None), lib, "vae2_ema_update")


def test_ema_update_of_nothing_launches_nothing():
    """n == 0 returns 0 before any launch (no device is needed for it)."""
    lib = _lib()
    assert lib.vae2_ema_update_dev(P, Q, 0, P, None) == 0
    assert lib.vae2_ema_update(P, Q, 0, 0.5, 0, None) == 0


@pytest.mark.parametrize("bad", [1.0, -0.1, NAN, INF])
def test_optimizer_constructors_reject_bad_ema_decay(bad):
    from vae2.optim import FusedAdam, FusedSGD
    with pytest.raises(ValueError, match="ema_decay"):
        FusedSGD(torch.nn.Linear(3, 2), lr=0.1, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdam(torch.nn.Linear(3, 2), lr=0.1, ema_decay=bad)


@pytest.mark.parametrize("good", [None, 0.0, 0.999])
def test_optimizer_constructors_accept_ema_decay(good):
    from vae2.optim import FusedAdam, FusedSGD
    for cls in (FusedSGD, FusedAdam):
        lin = torch.nn.Linear(3, 2)
        opt = cls(lin, lr=0.1, ema_decay=good)
        assert opt.ema_decay == good
        # the decay is configuration, not state: torch's keys exactly
        assert "ema_decay" not in opt.param_groups[0]
        ref = (torch.optim.SGD if cls is FusedSGD else torch.optim.Adam)(lin.parameters(), lr=0.1)
        assert set(opt.state_dict()["param_groups"][0]) <= set(ref.state_dict()["param_groups"][0])
        if good is None:
            assert opt.ema is None
            with pytest.raises(RuntimeError, match="ema_decay"):
                with opt.swap_ema():
                    pass
        else:
            # allocated by the constructor, one buffer per flat parameter buffer
            assert [e.shape for e in opt.ema] == [f.data.shape for f in opt.flats]
            assert all(e.data_ptr() != f.data.data_ptr() for e, f in zip(opt.ema, opt.flats))


def test_update_config_accepts_ema_keys():
    sys.path.insert(0, os.path.join(ROOT, "vae-2_amd", "lib"))
    from config.default import _C, update_config
    cfg = _C.clone()
    assert cfg.MI355X.EMA_DECAY == 0.0 and cfg.MI355X.EVAL_EMA is False  # off by default

    class A:
        cfg = os.path.join(ROOT, "vae-2_amd", "experiments", "vae2_w18_small_v2_128x256.yaml")
        opts = ["MI355X.EMA_DECAY", "0.999", "MI355X.EVAL_EMA", "True"]

    update_config(cfg, A)
    assert cfg.MI355X.EMA_DECAY == 0.999 and cfg.MI355X.EVAL_EMA is True
