"""The SSIM-loss entry points of the C ABI (vae2_ssim_loss_ws_size / _fwd / _bwd, additions
within ABI 15): symbols, types, and the host-side argument rules (-22 before any launch, the
function's name in vae2_last_error()), one violated rule per call.  No compute calls: runs
without a GPU."""
import ctypes
import os
import re

import pytest

from helpers import GOLDEN  # noqa: F401  (puts the package on sys.path via conftest)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("vae2_ssim_loss_ws_size", "vae2_ssim_loss_fwd", "vae2_ssim_loss_bwd")
P = ctypes.c_void_p(16)  # dummy non-null pointer: validation fails before it is used
INF, NAN = float("inf"), float("nan")
C1, C2 = 1e-4, 9e-4


def _mod():
    from vae2 import _lib
    return _lib


def _act(n=2, h=16, w=16, c=9, ps=None):
    return _mod().Act(n, h, w, c, c if ps is None else ps)


def test_symbols_typed_exported_and_declared():
    from test_abi import declared
    _lib = _mod()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vae2_hip.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMS:
        assert name in _lib.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes
        assert fn.restype is (ctypes.c_int64 if name.endswith("ws_size") else ctypes.c_int)
        assert re.search(r"\b%s\s*\(" % name, decls), name
    assert len(lib.vae2_ssim_loss_fwd.argtypes) == 12
    assert len(lib.vae2_ssim_loss_bwd.argtypes) == 14
    assert lib.vae2_ssim_loss_fwd.argtypes[10] is ctypes.c_void_p
    # binding == header, as test_abi.py asks
    assert sorted(_lib.exported_symbols()) == declared()


def test_abi_version_is_still_15():
    _lib = _mod()
    header = open(os.path.join(ROOT, "include", "vae2_hip.h")).read()
    assert _lib.ABI_VERSION == 15 and _lib.load().vae2_abi_version() == 15
    assert int(re.search(r"#define VAE2_ABI_VERSION (\d+)", header).group(1)) == 15


def test_ws_size_is_at_least_one():
    lib = _mod().load()
    for act in (_act(), _act(1, 11, 11, 1), _act(8, 128, 256, 9), _act(1, 5, 5, 3),
                _act(0, 0, 0, 0), _act(2, 16, 16, 9, 4)):
        assert lib.vae2_ssim_loss_ws_size(ctypes.byref(act)) >= 1
    assert lib.vae2_ssim_loss_ws_size(None) >= 1
    big, small = _act(8, 128, 256, 9), _act(1, 11, 11, 1)
    assert lib.vae2_ssim_loss_ws_size(ctypes.byref(big)) > \
        lib.vae2_ssim_loss_ws_size(ctypes.byref(small)) == 1


def _fwd(p=P, pd=None, t=P, td=None, a=None, b=None, c1=C1, c2=C2, scale=0.5, ws=P, out=P):
    pd = _act() if pd is None else pd
    td = _act() if td is None else td
    return _mod().load().vae2_ssim_loss_fwd(p, ctypes.byref(pd), t, ctypes.byref(td), a, b, c1,
                                            c2, scale, ws, out, None)


def _bwd(p=P, pd=None, t=P, td=None, a=None, b=None, c1=C1, c2=C2, gout=P, scale=0.5, dp=P,
         dpd=None, beta=0.0):
    pd = _act() if pd is None else pd
    td = _act() if td is None else td
    dpd = _act() if dpd is None else dpd
    return _mod().load().vae2_ssim_loss_bwd(p, ctypes.byref(pd), t, ctypes.byref(td), a, b, c1,
                                            c2, gout, scale, dp, ctypes.byref(dpd), beta, None)


# one violated rule per entry: (keyword arguments, a fragment of the message)
COMMON = [
    (dict(p=None), "null pointer"),
    (dict(t=None), "null pointer"),
    (dict(a=P), "a and b must be given together"),
    (dict(b=P), "a and b must be given together"),
    (dict(pd=_act(h=10), td=_act(h=10)), ">= 11"),
    (dict(pd=_act(w=10), td=_act(w=10)), ">= 11"),
    (dict(td=_act(n=3)), "shape mismatch"),
    (dict(td=_act(h=17)), "shape mismatch"),
    (dict(td=_act(w=17)), "shape mismatch"),
    (dict(td=_act(c=8)), "shape mismatch"),
    (dict(pd=_act(ps=8)), "pixel stride"),
    (dict(td=_act(ps=8)), "pixel stride"),
    (dict(pd=_act(1, 2 ** 15, 2 ** 15, 2), td=_act(1, 2 ** 15, 2 ** 15, 2)), "2^31"),
    (dict(c1=0.0), "c1 and c2"),
    (dict(c1=-1e-4), "c1 and c2"),
    (dict(c1=NAN), "c1 and c2"),
    (dict(c2=INF), "c1 and c2"),
    (dict(c2=0.0), "c1 and c2"),
    # n * ceil(c / 3) = 70000 workgroup planes: past the grid's 65535
    (dict(pd=_act(70000, 11, 11, 1), td=_act(70000, 11, 11, 1)), "too many planes"),
    (dict(pd=_act(35000, 11, 11, 4), td=_act(35000, 11, 11, 4)), "too many planes"),
]


def _check(rc, fn, fragment):
    lib = _mod().load()
    assert rc == -22
    err = lib.vae2_last_error().decode()
    assert fn in err and fragment in err, err


@pytest.mark.parametrize("kw,fragment", COMMON + [(dict(ws=None), "null pointer"),
                                                  (dict(out=None), "null pointer")])
def test_fwd_rejects(kw, fragment):
    _check(_fwd(**kw), "vae2_ssim_loss_fwd", fragment)


def _for_bwd(kw):
    # dp follows p's shape unless the case is about the operands themselves
    kw = dict(kw)
    if "pd" in kw and "dpd" not in kw and kw["pd"].ps >= kw["pd"].c:
        pd = kw["pd"]
        kw["dpd"] = _act(pd.n, pd.h, pd.w, pd.c)
    return kw


@pytest.mark.parametrize("kw,fragment", COMMON + [
    (dict(gout=None), "null pointer"),
    (dict(dp=None), "null pointer"),
    (dict(dpd=_act(c=8)), "dp shape mismatch"),
    (dict(dpd=_act(h=17)), "dp shape mismatch"),
    (dict(dpd=_act(ps=8)), "pixel stride"),
    (dict(beta=0.5), "beta"),
])
def test_bwd_rejects(kw, fragment):
    _check(_bwd(**_for_bwd(kw)), "vae2_ssim_loss_bwd", fragment)
