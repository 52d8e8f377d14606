"""The gradient-clipping entry points of the C ABI (ABI 14) and the host side of
max_grad_norm in vae2.optim: symbols, host-side argument validation (-22 before any launch),
constructor checks and the MI355X.CLIP_GRAD_NORM config key.  No compute calls: runs without
a GPU."""
import ctypes
import os
import re
import sys

import pytest
import torch

from helpers import GOLDEN  # noqa: F401  (puts the package on sys.path via conftest)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("vae2_grad_norm_ws_size", "vae2_grad_sumsq", "vae2_clip_coeffs",
        "vae2_sgd_step_dev_clip", "vae2_adam_step_dev_clip", "vae2_scale_dev")
P = ctypes.c_void_p(16)  # dummy non-null pointer: validation fails before it is used
INF, NAN = float("inf"), float("nan")


def _lib():
    from vae2 import _lib
    return _lib.load()


def test_clip_symbols_typed_exported_and_declared():
    from vae2 import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vae2_hip.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMS:
        assert name in _lib.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes
        assert fn.restype is (ctypes.c_int64 if name.endswith("ws_size") else ctypes.c_int)
        assert re.search(r"\b%s\s*\(" % name, decls), name
    assert _lib.ABI_VERSION >= 14 and lib.vae2_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define VAE2_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION


def test_ws_size_is_at_least_one_capped_and_a_function_of_n():
    lib = _lib()
    sizes = [lib.vae2_grad_norm_ws_size(n) for n in (0, 1, 1023, 1024, 1025, 10 ** 6, 10 ** 9,
                                                     2 ** 40)]
    assert all(s >= 1 for s in sizes)
    assert sizes == sorted(sizes) and sizes[-1] == sizes[-2]  # a fixed cap on the block count
    assert sizes == [lib.vae2_grad_norm_ws_size(n) for n in (0, 1, 1023, 1024, 1025, 10 ** 6,
                                                             10 ** 9, 2 ** 40)]


def _rejected(rc, lib, fn):
    assert rc == -22
    err = lib.vae2_last_error()
    assert fn.encode() in err, err


@pytest.mark.parametrize("g,n,partials", [(P, -1, P), (None, 8, P), (P, 8, None)])
def test_grad_sumsq_rejects_bad_arguments(g, n, partials):
    lib = _lib()
    _rejected(lib.vae2_grad_sumsq(g, n, partials, None), lib, "vae2_grad_sumsq")


@pytest.mark.parametrize("partials,count,max_norm,clip", [
    (P, 0, 1.0, P), (P, -3, 1.0, P), (None, 1, 1.0, P), (P, 1, 1.0, None),
    (P, 1, 0.0, P), (P, 1, -1.0, P), (P, 1, NAN, P), (P, 1, -INF, P),
])
def test_clip_coeffs_rejects_bad_arguments(partials, count, max_norm, clip):
    lib = _lib()
    _rejected(lib.vae2_clip_coeffs(partials, count, max_norm, clip, None), lib,
              "vae2_clip_coeffs")


@pytest.mark.parametrize("x,n,clip", [(P, -1, P), (None, 8, P), (P, 8, None)])
def test_scale_dev_rejects_bad_arguments(x, n, clip):
    lib = _lib()
    _rejected(lib.vae2_scale_dev(x, n, clip, None), lib, "vae2_scale_dev")


@pytest.mark.parametrize("p,g,buf,n,coeffs,clip,momentum,wd,nesterov,what", [
    (P, P, P, -1, P, P, 0.9, 0.0, 0, b"bad arguments"),
    (P, None, P, 8, P, P, 0.9, 0.0, 0, b"bad arguments"),
    (P, P, P, 8, P, None, 0.9, 0.0, 0, b"bad arguments"),   # null clip
    (P, P, P, 8, None, P, 0.9, 0.0, 0, b"bad arguments"),
    # what vae2_sgd_step_dev rejects
    (P, P, P, 8, P, P, 0.0, 0.0, 1, b"nesterov"),
    (P, P, None, 8, P, P, 0.9, 0.0, 0, b"momentum buffer"),
    (P, P, P, 8, P, P, -0.5, 0.0, 0, b"momentum"),
    (P, P, P, 8, P, P, 0.5, -1.0, 0, b"weight_decay"),
])
def test_sgd_step_dev_clip_rejects_bad_arguments(p, g, buf, n, coeffs, clip, momentum, wd,
                                                 nesterov, what):
    lib = _lib()
    rc = lib.vae2_sgd_step_dev_clip(p, g, buf, n, coeffs, clip, momentum, wd, nesterov, None)
    _rejected(rc, lib, "vae2_sgd_step_dev_clip")
    assert what in lib.vae2_last_error()


@pytest.mark.parametrize("null", ["p", "g", "m", "v", "coeffs", "clip", "n"])
def test_adam_step_dev_clip_rejects_bad_arguments(null):
    lib = _lib()
    a = dict(p=P, g=P, m=P, v=P, n=8, coeffs=P, clip=P)
    a[null] = -1 if null == "n" else None
    rc = lib.vae2_adam_step_dev_clip(a["p"], a["g"], a["m"], a["v"], a["n"], a["coeffs"],
                                     a["clip"], 0.9, 0.999, 1e-8, 0.0, None)
    _rejected(rc, lib, "vae2_adam_step_dev_clip")


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, NAN, -INF])
def test_optimizer_constructors_reject_bad_max_grad_norm(bad):
    from vae2.optim import FusedAdam, FusedSGD
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedSGD(torch.nn.Linear(3, 2), lr=0.1, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam(torch.nn.Linear(3, 2), lr=0.1, max_grad_norm=bad)


@pytest.mark.parametrize("good", [None, INF, 2.5])
def test_optimizer_constructors_accept_max_grad_norm(good):
    from vae2.optim import FusedAdam, FusedSGD
    for cls in (FusedSGD, FusedAdam):
        opt = cls(torch.nn.Linear(3, 2), lr=0.1, max_grad_norm=good)
        assert opt.max_grad_norm == good
        # the threshold is configuration, not state: torch's keys exactly
        assert "max_grad_norm" not in opt.param_groups[0]
        if good is None:
            with pytest.raises(RuntimeError, match="max_grad_norm"):
                opt.grad_norm()


def test_clip_grad_norm_rejects_bad_max_norm():
    from vae2.optim import clip_grad_norm_
    for bad in (0.0, -1.0, NAN, None):
        with pytest.raises(ValueError, match="max_norm"):
            clip_grad_norm_([], bad)


def test_update_config_accepts_clip_grad_norm():
    sys.path.insert(0, os.path.join(ROOT, "vae-2_amd", "lib"))
    from config.default import _C, update_config
    cfg = _C.clone()
    assert cfg.MI355X.CLIP_GRAD_NORM == 0.0  # off by default

    class A:
        cfg = os.path.join(ROOT, "vae-2_amd", "experiments", "vae2_w18_small_v2_128x256.yaml")
        opts = ["MI355X.CLIP_GRAD_NORM", "2.5"]

    update_config(cfg, A)
    assert cfg.MI355X.CLIP_GRAD_NORM == 2.5
    A.opts = ["MI355X.CLIP_GRAD_NORM", "1"]  # an int is accepted for the float key
    update_config(cfg, A)
    assert cfg.MI355X.CLIP_GRAD_NORM == 1.0 and isinstance(cfg.MI355X.CLIP_GRAD_NORM, float)
