"""Host-side argument validation of the loss, sampler, ReLU-backward, copy, code-map tile,
layout-conversion and pool-backward entry points of the C ABI: operands of one call must
agree in shape, and a kernel that counts elements in 32 bits rejects 2^31 or more of them
(FastDiv's __umulhi(n, m) + n can overflow from n = 2^31 on).  Every call must return -22
before any launch, with a vae2_last_error() that names the function.  The pointers are
dummies and are never dereferenced: runs without a GPU."""
import ctypes

import pytest

from helpers import GOLDEN  # noqa: F401  (puts the package on sys.path via conftest)

P = ctypes.c_void_p(16)  # dummy non-null pointer: validation fails before it is used
BIG = (1, 65536, 32768, 1)  # 2^31 elements: the first rejected size


def _lib():
    from vae2 import _lib
    return _lib, _lib.load()


def _act(n, h, w, c, ps=None):
    from vae2._lib import Act
    return Act(n, h, w, c, c if ps is None else ps)


def _ref(a):
    return ctypes.byref(a)


def _rejected(lib, name, rc, what):
    err = lib.vae2_last_error()
    assert rc == -22, (name, rc, err)
    assert name.encode() in err and what in err, err


def test_symbols_typed_and_exported():
    mod, lib = _lib()
    for name in ("vae2_l1_fwd", "vae2_l1_bwd", "vae2_lsgan_fwd", "vae2_lsgan_bwd",
                 "vae2_reparam_kl_fwd", "vae2_reparam_kl_bwd", "vae2_weighted_sum",
                 "vae2_nonfinite_check", "vae2_relu_bwd", "vae2_relu_bwd_dual", "vae2_copy_act",
                 "vae2_codemap_tile_fwd", "vae2_codemap_tile_bwd", "vae2_nchw_to_nhwc",
                 "vae2_nhwc_to_nchw", "vae2_global_avgpool_fwd", "vae2_global_avgpool_bwd",
                 "vae2_weighted_avgpool_fwd", "vae2_weighted_avgpool_bwd"):
        assert name in mod.exported_symbols()
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes
    # validation only: no signature changed, so the ABI version did not move
    assert mod.ABI_VERSION == 15 and lib.vae2_abi_version() == 15


# one field of the (2, 5, 7, 3) descriptor changed at a time
SHAPE = (2, 5, 7, 3)
OFF_BY_ONE = [(3, 5, 7, 3), (2, 6, 7, 3), (2, 5, 8, 3), (2, 5, 7, 4)]


@pytest.mark.parametrize("bad", OFF_BY_ONE)
@pytest.mark.parametrize("which", ["t", "dp"])
def test_l1_bwd_rejects_mismatched_operands(which, bad):
    _, lib = _lib()
    pd = _act(*SHAPE, ps=27)
    td = _act(*(bad if which == "t" else SHAPE), ps=9)
    dpd = _act(*(bad if which == "dp" else SHAPE), ps=12)
    # (p, pd, t, td, gout, scale, dp, dpd, beta, stream)
    rc = lib.vae2_l1_bwd(P, _ref(pd), P, _ref(td), P, 0.5, P, _ref(dpd), 0.0, None)
    _rejected(lib, "vae2_l1_bwd", rc, b"shape mismatch")


def test_l1_fwd_still_rejects_mismatched_target():
    _, lib = _lib()
    for bad in OFF_BY_ONE:
        rc = lib.vae2_l1_fwd(P, _ref(_act(*SHAPE)), P, _ref(_act(*bad)), 1.0, P, P, None)
        _rejected(lib, "vae2_l1_fwd", rc, b"shape mismatch")


def test_lsgan_bwd_still_rejects_mismatched_dx():
    _, lib = _lib()
    for bad in OFF_BY_ONE:
        # (x, xd, target, gout, scale, dx, dxd, beta, stream)
        rc = lib.vae2_lsgan_bwd(P, _ref(_act(*SHAPE)), 1.0, P, 1.0, P, _ref(_act(*bad)), 0.0, None)
        _rejected(lib, "vae2_lsgan_bwd", rc, b"shape mismatch")


ZSHAPE = (2, 8, 16, 4)
NHW_OFF = [(3, 8, 16), (2, 9, 16), (2, 8, 17)]


@pytest.mark.parametrize("nhw", NHW_OFF)
@pytest.mark.parametrize("which", ["m", "e", "z"])
def test_reparam_kl_fwd_rejects_mismatched_nhw(which, nhw):
    _, lib = _lib()
    n, h, w, zc = ZSHAPE
    md = _act(*(nhw if which == "m" else (n, h, w)), 2 * zc, ps=12)
    ed = _act(*(nhw if which == "e" else (n, h, w)), zc)
    zd = _act(*(nhw if which == "z" else (n, h, w)), zc)
    # (muvar, md, eps, ed, z, zd, prior, scale, kl_out, accumulate, ws, stream)
    rc = lib.vae2_reparam_kl_fwd(P, _ref(md), P, _ref(ed), P, _ref(zd), 0, 1.0, P, 0, P, None)
    _rejected(lib, "vae2_reparam_kl_fwd", rc, b"mismatch")


def test_reparam_kl_fwd_rejects_mismatched_channels():
    _, lib = _lib()
    n, h, w, zc = ZSHAPE
    for mc, ec in ((2 * zc + 1, zc), (2 * zc, zc + 1), (zc, zc)):
        rc = lib.vae2_reparam_kl_fwd(P, _ref(_act(n, h, w, mc)), P, _ref(_act(n, h, w, ec)), P,
                                     _ref(_act(n, h, w, zc)), 0, 1.0, P, 0, P, None)
        _rejected(lib, "vae2_reparam_kl_fwd", rc, b"channel mismatch")


def _kl_bwd(lib, md, ed, dzd, dmd, dz=P):
    # (muvar, md, eps, ed, dz, dzd, gkl, scale, dmuvar, dmd, stream)
    return lib.vae2_reparam_kl_bwd(P, _ref(md), P, _ref(ed), dz, _ref(dzd), P, 1.0, P, _ref(dmd),
                                   None)


def test_reparam_kl_bwd_rejects_mismatched_operands():
    _, lib = _lib()
    n, h, w, zc = ZSHAPE
    md, ed = _act(n, h, w, 2 * zc, ps=12), _act(n, h, w, zc)
    dzd, dmd = _act(n, h, w, zc, ps=6), _act(n, h, w, 2 * zc, ps=16)
    # muvar must hold 2 * zc channels
    for mc in (2 * zc - 1, 2 * zc + 1, zc):
        bad = _act(n, h, w, mc, ps=12)
        _rejected(lib, "vae2_reparam_kl_bwd", _kl_bwd(lib, bad, ed, dzd, bad), b"channel mismatch")
    for nhw in NHW_OFF:
        # muvar against eps
        bad_m = _act(*nhw, 2 * zc, ps=12)
        _rejected(lib, "vae2_reparam_kl_bwd", _kl_bwd(lib, bad_m, ed, dzd, bad_m), b"mismatch")
        bad_e = _act(*nhw, zc)
        _rejected(lib, "vae2_reparam_kl_bwd", _kl_bwd(lib, md, bad_e, dzd, dmd), b"mismatch")
        # dmuvar against muvar
        _rejected(lib, "vae2_reparam_kl_bwd",
                  _kl_bwd(lib, md, ed, dzd, _act(*nhw, 2 * zc, ps=16)), b"dmuvar shape mismatch")
        # dz against eps, only when dz is set
        _rejected(lib, "vae2_reparam_kl_bwd",
                  _kl_bwd(lib, md, ed, _act(*nhw, zc, ps=6), dmd), b"dz shape mismatch")
    _rejected(lib, "vae2_reparam_kl_bwd",
              _kl_bwd(lib, md, ed, dzd, _act(n, h, w, 2 * zc - 1, ps=16)), b"dmuvar shape mismatch")
    _rejected(lib, "vae2_reparam_kl_bwd",
              _kl_bwd(lib, md, ed, _act(n, h, w, zc + 1, ps=6), dmd), b"dz shape mismatch")
    # a NULL dz makes its descriptor irrelevant: the next failing rule is dmuvar's
    rc = _kl_bwd(lib, md, ed, _act(n, h + 1, w, zc + 1, ps=6), _act(n, h, w + 1, 2 * zc, ps=16),
                 dz=None)
    _rejected(lib, "vae2_reparam_kl_bwd", rc, b"dmuvar shape mismatch")


def _too_large_calls(lib):
    """name -> the call with every activation of 2^31 elements (shapes consistent, so that
    only the size rule can fail)."""
    b = _act(*BIG)
    n, h, w, _ = BIG
    b1, b2 = _act(n, h, w, 1), _act(n, h, w, 2)  # eps / z and muvar
    v = _act(1, 1, 1, 1)  # the pooled (n, 1, 1, c) side of a pool backward
    r = _ref
    return {
        "vae2_l1_fwd": lambda: lib.vae2_l1_fwd(P, r(b), P, r(b), 1.0, P, P, None),
        "vae2_l1_bwd": lambda: lib.vae2_l1_bwd(P, r(b), P, r(b), P, 1.0, P, r(b), 0.0, None),
        "vae2_lsgan_fwd": lambda: lib.vae2_lsgan_fwd(P, r(b), 1.0, 1.0, P, P, None),
        "vae2_lsgan_bwd": lambda: lib.vae2_lsgan_bwd(P, r(b), 1.0, P, 1.0, P, r(b), 0.0, None),
        "vae2_reparam_kl_fwd": lambda: lib.vae2_reparam_kl_fwd(P, r(b2), P, r(b1), P, r(b1), 0,
                                                               1.0, P, 0, P, None),
        "vae2_reparam_kl_bwd": lambda: lib.vae2_reparam_kl_bwd(P, r(b2), P, r(b1), P, r(b1), P,
                                                               1.0, P, r(b2), None),
        "vae2_relu_bwd": lambda: lib.vae2_relu_bwd(P, r(b), P, r(b), P, r(b), None),
        "vae2_relu_bwd_dual": lambda: lib.vae2_relu_bwd_dual(P, r(b), P, r(b), P, r(b), P, r(b),
                                                             0.0, None),
        "vae2_copy_act": lambda: lib.vae2_copy_act(P, r(b), P, r(b), 0.0, None),
        "vae2_codemap_tile_fwd": lambda: lib.vae2_codemap_tile_fwd(P, 1, P, r(b), None),
        "vae2_nchw_to_nhwc": lambda: lib.vae2_nchw_to_nhwc(P, P, r(b), 0.0, None),
        "vae2_nhwc_to_nchw": lambda: lib.vae2_nhwc_to_nchw(P, r(b), P, 0.0, None),
        "vae2_global_avgpool_bwd": lambda: lib.vae2_global_avgpool_bwd(P, r(v), P, r(b), 0.0,
                                                                       None),
        "vae2_weighted_avgpool_bwd": lambda: lib.vae2_weighted_avgpool_bwd(P, r(v), P, P, 1.0, P,
                                                                           r(b), 0.0, None),
    }


TOO_LARGE = ["vae2_l1_fwd", "vae2_l1_bwd", "vae2_lsgan_fwd", "vae2_lsgan_bwd",
             "vae2_reparam_kl_fwd", "vae2_reparam_kl_bwd", "vae2_relu_bwd", "vae2_relu_bwd_dual",
             "vae2_copy_act", "vae2_codemap_tile_fwd", "vae2_nchw_to_nhwc", "vae2_nhwc_to_nchw",
             "vae2_global_avgpool_bwd", "vae2_weighted_avgpool_bwd"]


@pytest.mark.parametrize("name", TOO_LARGE)
def test_two_to_the_31_elements_rejected(name):
    _, lib = _lib()
    calls = _too_large_calls(lib)
    assert sorted(calls) == sorted(TOO_LARGE)
    _rejected(lib, name, calls[name](), b"2^31")


def test_too_large_in_another_axis():
    """The limit is on the element count, whichever axes make it up."""
    _, lib = _lib()
    for shape in ((32768, 1, 1, 65536), (2, 32768, 32768, 1), (1, 46341, 46341, 1)):
        a = _act(*shape)
        assert shape[0] * shape[1] * shape[2] * shape[3] >= 2 ** 31
        _rejected(lib, "vae2_copy_act", lib.vae2_copy_act(P, _ref(a), P, _ref(a), 0.0, None),
                  b"2^31")
        _rejected(lib, "vae2_lsgan_fwd", lib.vae2_lsgan_fwd(P, _ref(a), 0.0, 1.0, P, P, None),
                  b"2^31")


def test_header_documents_the_limit():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vae2_hip.h")) as f:
        head = f.read().split("#ifndef VAE2_HIP_H")[0]
    assert "2^31" in head and "tensor too large" in head
