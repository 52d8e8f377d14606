"""The yardstick of the SSIM-loss kernels (tests/ssim_ref.py) against the project's oracle and
against torch.autograd, the kernel file's window literals, and the MI355X.SSIM_LAMBDA config
key.  Runs without a GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN  # noqa: F401  (puts the package on sys.path via conftest)

import ssim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 11, 11, 3), (1, 12, 37, 9), (2, 45, 77, 9)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["near", "indep"])
def test_fp64_forward_is_the_oracles_ssim_map_summed(shape, kind):
    from oracle import metrics_ref
    p, t = ssim_ref.make_inputs(shape, kind, seed=11)
    win = ssim_ref.window(torch.float32).numpy()
    K = (0.01, 0.03)
    X, Y = (x.permute(0, 3, 1, 2).numpy() for x in (p, t))
    mean_ssim, _ = metrics_ref._ssim(X, Y, 1.0, win, K)  # [n][c] means of the valid map
    count = (shape[1] - 10) * (shape[2] - 10)
    want = float((mean_ssim * count).sum())
    m = ssim_ref.ssim_map(p, t, c1=K[0] ** 2, c2=K[1] ** 2, exact_consts=True)
    assert m.shape == (shape[0], shape[1] - 10, shape[2] - 10, shape[3])
    got = float(m.sum())
    print(f"{shape} {kind}: sum ssim = {got!r}, oracle {want!r}")
    assert abs(got - want) <= 1e-12 * abs(want)
    # and the loss is scale * (count - that sum)
    loss = float(ssim_ref.loss(p, t, 0.5))
    ref = 0.5 * (count * shape[0] * shape[3] - float(ssim_ref.ssim_map(p, t).sum()))
    assert abs(loss - ref) <= 1e-12 * abs(ref)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("affine", [False, True])
def test_closed_form_gradient_is_autograds(shape, affine):
    p, t = ssim_ref.make_inputs(shape, "near", seed=5)
    a, b = ssim_ref.coeffs(shape[3]) if affine else (None, None)
    want = ssim_ref.grad_autograd(p, t, 0.5, a, b, gout=1.25)
    got = ssim_ref.grad_closed_form(p, t, 0.5, a, b, gout=1.25)
    err = float((got - want).abs().max())
    top = float(want.abs().max())
    print(f"{shape} affine={affine}: max|grad| = {top:.3e}, max err = {err:.3e}")
    assert top > 0 and err <= 1e-12 * top


def test_identical_inputs_give_exactly_zero_in_fp32_and_fp64():
    p, _ = ssim_ref.make_inputs((1, 12, 37, 9), "near", seed=2)
    for dtype in (torch.float32, torch.float64):
        assert float(ssim_ref.loss(p, p, 1.0, dtype=dtype)) == 0.0


def test_kernel_window_literals_are_the_metrics_window():
    src = open(os.path.join(ROOT, "vae-2_amd", "csrc", "ssim_loss.hip")).read()
    body = re.search(r"kWindow = \{\{(.*?)\}\}", src, flags=re.S).group(1)
    taps = [float.fromhex(x.rstrip("f")) for x in re.findall(r"0x[0-9a-f.]+p[-+]?\d+f", body)]
    want = ssim_ref.window(torch.float32)
    assert len(taps) == 11
    assert np.array_equal(np.asarray(taps, dtype=np.float32), want.numpy())
    assert [float(x) for x in want] == taps  # exact fp32 values, not rounded decimals


def test_update_config_accepts_ssim_lambda():
    sys.path.insert(0, os.path.join(ROOT, "vae-2_amd", "lib"))
    from config.default import _C, update_config
    cfg = _C.clone()
    assert cfg.MI355X.SSIM_LAMBDA == 0.0  # off by default

    class A:
        cfg = os.path.join(ROOT, "vae-2_amd", "experiments", "vae2_w18_small_v2_128x256.yaml")
        opts = ["MI355X.SSIM_LAMBDA", "0.5"]

    update_config(cfg, A)
    assert cfg.MI355X.SSIM_LAMBDA == 0.5
    A.opts = ["MI355X.SSIM_LAMBDA", "1"]  # an int is accepted for the float key
    update_config(cfg, A)
    assert cfg.MI355X.SSIM_LAMBDA == 1.0 and isinstance(cfg.MI355X.SSIM_LAMBDA, float)


def test_model_and_criterion_take_the_new_argument():
    from vae2.criterion import SSIMLoss
    from vae2.model import FullModel_encdec
    fm = FullModel_encdec(None, None, None, None, None, None, None)
    assert fm.ssim_lambda == 0.0 and fm.ssim_terms is None
    fm = FullModel_encdec(None, None, None, None, None, None, None, ssim_lambda=0.5)
    assert fm.ssim_lambda == 0.5
    with pytest.raises(ValueError, match="ssim_lambda"):
        FullModel_encdec(None, None, None, None, None, None, None, ssim_lambda=-1.0)
    sys.path.insert(0, os.path.join(ROOT, "vae-2_amd", "lib"))
    from core import criterion
    assert criterion.SSIMLoss is SSIMLoss
