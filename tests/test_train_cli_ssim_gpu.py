"""The drop-in CLI (vae-2_amd/tools/train.py) with MI355X.SSIM_LAMBDA: one epoch trains with
the SSIM terms on and logs them; a negative weight is refused before any file is written; a
default run does not mention them.  64x32 frames, batch 2, 4 synthetic clips (2 iterations
per epoch), ELBO only."""
import logging
import math
import os
import re

import pytest

from test_train_cli_ema_gpu import BASE, _load, _out, _train

pytestmark = pytest.mark.gpu
H, W = 32, 64


def test_train_cli_trains_with_the_ssim_terms(tmp_path, caplog):
    with caplog.at_level(logging.INFO):
        out = _train(tmp_path, *BASE, "MI355X.SSIM_LAMBDA", "0.5")
    ck = _load(out, "checkpoint_encdec.pth.tar")
    assert set(ck) == {"epoch", "state_dict", "optimizer_encdec"} and ck["epoch"] == 1
    assert os.path.isfile(os.path.join(out, "model_encdec_final_state.pth"))
    lines = [r.getMessage() for r in caplog.records if "_ssim" in r.getMessage()
             and r.getMessage().startswith("loss_")]
    assert len(lines) == 2, caplog.text  # PRINT_FREQ 1, two iterations
    top = 9 * (H - 10) * (W - 10) * 2
    for line in lines:
        vals = dict(re.findall(r"(loss_x[23]?t_ssim): (\S+)", line))
        assert sorted(vals) == ["loss_x2t_ssim", "loss_x3t_ssim", "loss_xt_ssim"], line
        for v in vals.values():
            assert math.isfinite(float(v)) and 0.0 <= float(v) <= top, line


def test_train_cli_rejects_a_negative_weight(tmp_path):
    with pytest.raises(ValueError, match="SSIM_LAMBDA"):
        _train(tmp_path, *BASE, "MI355X.SSIM_LAMBDA", "-1")
    assert not os.path.exists(os.path.join(_out(tmp_path), "checkpoint_encdec.pth.tar"))
    assert not os.path.exists(os.path.join(_out(tmp_path), "models"))


def test_default_run_logs_no_ssim_text(tmp_path, caplog):
    with caplog.at_level(logging.INFO):
        _train(tmp_path, *BASE)
    epoch_lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Epoch:")]
    assert len(epoch_lines) == 2
    # no SSIM value anywhere (the config dump names the key itself, as `SSIM_LAMBDA: 0.0`)
    texts = [r.getMessage() for r in caplog.records]
    assert not [m for m in texts if re.search(r"_ssim\b|ssim:", m)]
    assert not [m for m in texts if m.startswith("loss_")]
    assert [m for m in texts if "SSIM_LAMBDA: 0.0" in m]
