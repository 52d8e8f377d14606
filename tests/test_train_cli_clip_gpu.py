"""The drop-in CLI (vae-2_amd/tools/train.py) with MI355X.CLIP_GRAD_NORM: plain SGD at a
learning rate of 1, which without clipping overflows at once, takes steps of length
lr * max_norm, and the trainer checks and logs the gradient norms at PRINT_FREQ points."""
import logging
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "vae-2_amd", "tools")
YAML = os.path.join(ROOT, "vae-2_amd", "experiments", "vae2_w18_small_v2_128x256.yaml")

pytestmark = pytest.mark.gpu

LR, MAX_NORM = 1.0, 1.0
CLIPPED_SGD = ("TRAIN.OPTIMIZER", "sgd", "TRAIN.MOMENTUM", "0.0", "TRAIN.WD", "0.0",
               "TRAIN.LR", str(LR), "MI355X.CLIP_GRAD_NORM", str(MAX_NORM))


def _train(tmp_path, *opts, cfg=YAML, size="[64, 32]"):
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import train  # vae-2_amd/tools/train.py
    from config import config
    config.defrost()
    config.merge_from_file(cfg)  # reset anything a previous run merged
    config.freeze()
    before = config.clone()
    argv = ["--cfg", cfg, "OUTPUT_DIR", str(tmp_path / "output"), "LOG_DIR", str(tmp_path / "log"),
            "TRAIN.IMAGE_SIZE", size, "TRAIN.BATCH_SIZE_PER_GPU", "2",
            "MI355X.SYNTHETIC_CLIPS", "4", "PRINT_FREQ", "1", "MI355X.DEFER_CHECKS", "True",
            "TRAIN.END_EPOCH", "1", *opts]
    try:
        train.main(argv)
    finally:  # keys the YAML does not hold (the threshold, MOMENTUM, WD) would stay merged in
        # the process-wide config: later runs in this process start from the state before
        config.defrost()
        config.merge_from_other_cfg(before)
        config.freeze()
    return os.path.join(str(tmp_path / "output"), "cityscapessequence",
                        os.path.basename(cfg).split(".")[0])


def _load(out, name):
    return torch.load(os.path.join(out, name), map_location="cpu", weights_only=True)


def _finite(ck):
    return all(torch.isfinite(v).all() for v in ck["state_dict"].values()
               if v.is_floating_point())


def test_train_cli_clipped_sgd_takes_steps_of_length_lr_times_max_norm(tmp_path, monkeypatch,
                                                                       caplog):
    """Every step: grad_norm() > max_norm, and with t the norm the update is the gradient
    scaled to the norm max_norm * t / (t + 1e-6) (a few fp32 roundings: 2^-20 covers them) times
    lr, each stored parameter adding at most half an ulp of its own rounding:
    0.99 * lr * max_norm <= ||dp|| <= lr * max_norm * (1 + 2^-20) + 2^-23 * ||p_before||."""
    from vae2.optim import FusedSGD
    seen = []
    step = FusedSGD.step

    def spy(self):
        before = torch.cat([f.data for f in self.flats]).double().cpu()
        step(self)
        after = torch.cat([f.data for f in self.flats]).double().cpu()
        seen.append((self.max_grad_norm, self.grad_norm().item(), float((after - before).norm()),
                     float(before.norm())))
    monkeypatch.setattr(FusedSGD, "step", spy)
    with caplog.at_level(logging.INFO):
        out = _train(tmp_path, *CLIPPED_SGD, "MI355X.ELBO_ONLY", "True")
    assert len(seen) == 2  # 4 clips, batch 2, one epoch
    for max_norm, t, dp, p_norm in seen:
        print(f"grad_norm={t!r} ||dp||={dp!r} ||p||={p_norm!r}")
        assert max_norm == MAX_NORM
        assert math.isfinite(t) and t > 1
        assert 0.99 * LR * MAX_NORM <= dp <= LR * MAX_NORM * (1 + 2.0 ** -20) + 2.0 ** -23 * p_norm
    ck = _load(out, "checkpoint_encdec.pth.tar")
    assert ck["epoch"] == 1 and _finite(ck)
    # torch's keys exactly: the threshold is configuration, not optimizer state
    assert "max_grad_norm" not in ck["optimizer_encdec"]["param_groups"][0]
    lines = [r.getMessage() for r in caplog.records if "grad_norm_encdec:" in r.getMessage()]
    assert len(lines) == 2, caplog.text
    for line, (_, t, _, _) in zip(lines, seen):
        m = re.fullmatch(r"grad_norm_encdec: (\S+)", line)  # no discriminator: one norm
        assert m and abs(float(m.group(1)) - t) <= 1e-6 * t + 1e-6
    # the reference's own log line is still there, one per iteration, as it was
    assert sum("Loss_encdec_ave:" in r.getMessage() for r in caplog.records) == 2


def test_train_cli_clipped_gan_run_logs_both_norms(tmp_path, caplog):
    with caplog.at_level(logging.INFO):
        out = _train(tmp_path, *CLIPPED_SGD, "MI355X.ELBO_ONLY", "False",
                     "TRAIN.GAN_LAMBDA", "1.0")
    lines = [r.getMessage() for r in caplog.records if "grad_norm_encdec:" in r.getMessage()]
    assert len(lines) == 2, caplog.text
    for line in lines:
        m = re.fullmatch(r"grad_norm_encdec: (\S+) grad_norm_D: (\S+)", line)
        assert m, line
        assert all(math.isfinite(float(v)) and float(v) > 0 for v in m.groups())
    ck, ckd = _load(out, "checkpoint_encdec.pth.tar"), _load(out, "checkpoint_D.pth.tar")
    assert ck["epoch"] == ckd["epoch"] == 1
    assert _finite(ck) and _finite(ckd)


def test_train_cli_rejects_negative_threshold(tmp_path):
    with pytest.raises(ValueError, match="CLIP_GRAD_NORM"):
        _train(tmp_path, "TRAIN.OPTIMIZER", "sgd", "MI355X.ELBO_ONLY", "True",
               "MI355X.CLIP_GRAD_NORM", "-1.0")
