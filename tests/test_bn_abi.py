"""Shape checks of the BatchNorm entry points: operands of one call that disagree in n, h, w
or c are rejected on the host with -22 and a message, before any launch (include/vae2_hip.h,
Conventions).  Dummy pointers are enough; runs without a GPU."""
import ctypes

import pytest

from helpers import GOLDEN  # noqa: F401  (puts the package on sys.path via conftest)

P = ctypes.c_void_p(4096)  # a 16-byte aligned dummy address, never dereferenced
N, H, W, C, PS = 2, 5, 7, 20, 24
FIELDS = ["n", "h", "w", "c"]


def _act(**kw):
    from vae2 import _lib
    d = dict(n=N, h=H, w=W, c=C, ps=PS)
    d.update(kw)
    return _lib.Act(d["n"], d["h"], d["w"], d["c"], d["ps"])


def _off(field):
    """One field of the descriptor made smaller than x's (the operand would be read or
    written past its end)."""
    return {field: {"n": N, "h": H, "w": W, "c": C}[field] - 1}


def _rejected(lib, rc, *words):
    msg = lib.vae2_last_error()
    assert rc == -22, (rc, msg)
    assert any(w.encode() in msg for w in words), msg


@pytest.mark.parametrize("field", FIELDS)
def test_bn_apply_rejects_a_mismatching_operand(field):
    from vae2 import _lib
    lib = _lib.load()
    x, bad = _act(), _act(**_off(field))
    r = ctypes.byref
    rc = lib.vae2_bn_apply(P, r(x), P, P, r(bad), P, r(x), 1, None)
    _rejected(lib, rc, "residual shape mismatch")
    rc = lib.vae2_bn_apply(P, r(x), P, None, r(x), P, r(bad), 1, None)
    _rejected(lib, rc, "x / y shape mismatch")


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("operand", ["dy", "y"])
def test_bn_relu_bwd_reduce_rejects_a_mismatching_operand(operand, field):
    from vae2 import _lib
    lib = _lib.load()
    d = {k: _act() for k in ("dy", "y")}
    d[operand] = _act(**_off(field))
    r = ctypes.byref
    rc = lib.vae2_bn_relu_bwd_reduce(P, r(d["dy"]), P, r(d["y"]), P, r(_act()), P, 1, P, None)
    _rejected(lib, rc, f"{operand} / x shape mismatch")


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("operand", ["dy", "y", "dx", "dres"])
def test_bn_relu_bwd_apply_rejects_a_mismatching_operand(operand, field):
    from vae2 import _lib
    lib = _lib.load()
    d = {k: _act() for k in ("dy", "y", "dx", "dres")}
    d[operand] = _act(**_off(field))
    r = ctypes.byref
    rc = lib.vae2_bn_relu_bwd_apply(P, r(d["dy"]), P, r(d["y"]), P, r(_act()), P, P, P, 70.0, 1,
                                    P, r(d["dx"]), P, r(d["dres"]), None)
    _rejected(lib, rc, f"{operand} / x shape mismatch")


def _layer(**kw):
    """A backward-complete layer of dummy pointers; kw replaces fields."""
    from vae2 import _lib
    l = _lib.BnLayer()
    l.x = l.a = l.o = l.dy = l.dres = l.save = l.gamma = l.partials = l.sums = P.value
    l.xd, l.ad, l.od, l.dyd, l.dresd = _act(), _act(), _act(), _act(), _act()
    l.count, l.relu = float(N * H * W), 1
    for k, v in kw.items():
        setattr(l, k, v)
    return l


MULTI_BAD = {
    "dyd.c": dict(dyd=_off("c")), "dyd.n": dict(dyd=_off("n")),
    "dresd.n": dict(dresd=_off("n")), "dresd.h": dict(dresd=_off("h")),
    "dresd.w": dict(dresd=_off("w")), "dresd.c": dict(dresd=_off("c")),
    "ad.n": dict(ad=_off("n")), "ad.h": dict(ad=_off("h")), "ad.w": dict(ad=_off("w")),
    "ad.c": dict(ad=_off("c")), "od.c": dict(od=_off("c")), "od.w": dict(od=_off("w")),
}


@pytest.mark.parametrize("which", list(MULTI_BAD))
@pytest.mark.parametrize("entry", ["vae2_bn_multi_bwd_reduce", "vae2_bn_multi_bwd_apply"])
def test_bn_multi_bwd_rejects_a_mismatching_layer(entry, which):
    from vae2 import _lib
    lib = _lib.load()
    bad = _layer(**{k: _act(**v) for k, v in MULTI_BAD[which].items()})
    arr = (_lib.BnLayer * 2)(_layer(), bad)  # the first layer is fine: no launch before the check
    rc = getattr(lib, entry)(2, arr, None)
    _rejected(lib, rc, "matching shapes")


@pytest.mark.parametrize("which", ["ad.n", "ad.h", "ad.w", "ad.c", "od.c", "od.w"])
def test_bn_multi_apply_rejects_a_mismatching_layer(which):
    from vae2 import _lib
    lib = _lib.load()
    bad = _layer(**{k: _act(**v) for k, v in MULTI_BAD[which].items()})
    rc = lib.vae2_bn_multi_apply(2, (_lib.BnLayer * 2)(_layer(), bad), None)
    _rejected(lib, rc, "matching shapes")


UNALIGNED = [(e, h) for e in ("vae2_bn_multi_apply", "vae2_bn_multi_bwd_reduce",
                               "vae2_bn_multi_bwd_apply")
             for h in ("x + 4 bytes", "x ps odd", "dy + 4 bytes", "o ps odd")
             if not (e == "vae2_bn_multi_apply" and h.startswith("dy"))]  # the forward takes no dy


@pytest.mark.parametrize("entry,how", UNALIGNED)
def test_bn_multi_rejects_an_unaligned_layer(entry, how):
    from vae2 import _lib
    lib = _lib.load()
    kw = {"x + 4 bytes": dict(x=P.value + 4), "x ps odd": dict(xd=_act(ps=PS + 1)),
          "dy + 4 bytes": dict(dy=P.value + 4), "o ps odd": dict(od=_act(ps=PS + 1))}[how]
    rc = getattr(lib, entry)(2, (_lib.BnLayer * 2)(_layer(), _layer(**kw)), None)
    _rejected(lib, rc, "16-byte aligned")
