"""The drop-in CLIs with MI355X.EMA_DECAY / MI355X.EVAL_EMA: tools/train.py keeps the weight
average inside the fused step, writes it into the checkpoint and resumes it; tools/inference.py
evaluates it.  64x32 frames, batch 2, 4 synthetic clips (2 iterations per epoch), ELBO only.

The saved average after one epoch at decay 0.5 is p1 + 0.5 * (p2 - p1) of the parameters after
the two steps, within the K = 2 case of the bound derived in tests/test_ema_gpu.py:
|got - ref| <= K * 2^-21 * max(|p1|, |p2|) per element."""
import logging
import os
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "vae-2_amd", "tools")
YAML = os.path.join(ROOT, "vae-2_amd", "experiments", "vae2_w18_small_v2_128x256.yaml")

pytestmark = pytest.mark.gpu

DECAY = 0.5
BASE = ("MI355X.ELBO_ONLY", "True")
EMA = BASE + ("MI355X.EMA_DECAY", str(DECAY))


def _restoring_config(fn, cfg=YAML):
    """Run fn() on the process-wide config reset to the YAML, and put the config back after."""
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import train  # noqa: F401  (vae-2_amd/tools/train.py: puts lib/ on sys.path)
    from config import config
    config.defrost()
    config.merge_from_file(cfg)  # reset anything a previous run merged
    config.freeze()
    before = config.clone()
    try:
        return fn()
    finally:  # keys the YAML does not hold (EMA_DECAY, EVAL_EMA) would stay merged
        config.defrost()
        config.merge_from_other_cfg(before)
        config.freeze()


def _common(path):
    return ["--cfg", YAML, "OUTPUT_DIR", str(path / "output"), "LOG_DIR", str(path / "log"),
            "TRAIN.IMAGE_SIZE", "[64, 32]", "TRAIN.BATCH_SIZE_PER_GPU", "2",
            "MI355X.SYNTHETIC_CLIPS", "4"]


def _out(path):
    return os.path.join(str(path / "output"), "cityscapessequence",
                        os.path.basename(YAML).split(".")[0])


def _train(path, *opts, end_epoch=1):
    def run():
        import train  # vae-2_amd/tools/train.py
        train.main(_common(path) + ["PRINT_FREQ", "1", "MI355X.DEFER_CHECKS", "True",
                                    "TRAIN.END_EPOCH", str(end_epoch), *opts])
    _restoring_config(run)
    return _out(path)


def _infer(path, *opts):
    def run():
        import inference  # vae-2_amd/tools/inference.py
        return inference.main(_common(path) + ["TRAIN.RESUME", "True", "MI355X.EVAL_SAMPLES", "2",
                                               *opts])
    return _restoring_config(run)


def _load(out, name):
    return torch.load(os.path.join(out, name), map_location="cpu", weights_only=True)


def _is_buffer(key):
    return "running_" in key or "num_batches_tracked" in key


def _flat(sd):
    """The parameters of a state_dict as one fp64 vector in the optimizer's flat order:
    encz_model, then encdec_model (tools/train.py builds FusedAdam([encz_model,
    encdec_model])), each module's parameters in state_dict order."""
    params = [k for k in sd if not _is_buffer(k)]
    encz = [k for k in params if k.startswith("encz_model.")]
    ed = [k for k in params if k.startswith("encdec_model.")]
    assert len(encz) + len(ed) == len(params) and encz and ed
    return torch.cat([sd[k].reshape(-1).double() for k in encz + ed])


TORCH_ADAM_KEYS = set(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])
                      .state_dict()["param_groups"][0])


@pytest.fixture(scope="module")
def ema_run(tmp_path_factory):
    """One epoch with the average on: (directory, output directory, the flat parameter buffers
    after each step in fp64, the checkpoint)."""
    from vae2.optim import FusedAdam
    path = tmp_path_factory.mktemp("ema_run")
    seen = []
    step = FusedAdam.step

    def spy(self):
        step(self)
        assert self.ema_decay == DECAY  # ELBO only: the generator optimizer is the only one
        seen.append([f.data.double().cpu() for f in self.flats])
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(FusedAdam, "step", spy)
        out = _train(path, *EMA)
    return path, out, seen, _load(out, "checkpoint_encdec.pth.tar")


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """One epoch with the defaults (the average off)."""
    path = tmp_path_factory.mktemp("plain_run")
    out = _train(path, *BASE)
    return path, out, _load(out, "checkpoint_encdec.pth.tar")


def test_train_cli_writes_the_average(ema_run):
    path, out, seen, ck = ema_run
    assert len(seen) == 2  # 4 clips, batch 2, one epoch
    assert set(ck) == {"epoch", "state_dict", "optimizer_encdec", "ema_state_dict", "ema_updates"}
    assert ck["epoch"] == 1
    assert ck["ema_updates"] == 2 and isinstance(ck["ema_updates"], int)
    live, ema = ck["state_dict"], ck["ema_state_dict"]
    assert list(ema) == list(live)
    assert all(ema[k].shape == live[k].shape and ema[k].dtype == live[k].dtype for k in live)
    assert all(torch.isfinite(v).all() for v in ema.values() if v.is_floating_point())
    bufs = [k for k in live if _is_buffer(k)]
    assert bufs
    for k in bufs:  # running statistics are not averaged: the live ones
        assert torch.equal(ema[k], live[k]), k
    p1, p2 = torch.cat(seen[0]), torch.cat(seen[1])
    # the live weights are those after the second step (and _flat's order is the optimizer's)
    assert torch.equal(_flat(live), p2)
    got = _flat(ema)
    ref = p1 + DECAY * (p2 - p1)
    err = (got - ref).abs()
    bound = 2 * 2.0 ** -21 * torch.maximum(p1.abs(), p2.abs())
    print(f"max err = {float(err.max()):.3e}, max err/bound = "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert not torch.equal(got, p2)  # an average, not a copy of the live weights
    assert os.path.isfile(os.path.join(out, "model_encdec_final_state_ema.pth"))
    final = _load(out, "model_encdec_final_state_ema.pth")
    assert list(final) == list(ema) and all(torch.equal(final[k], ema[k]) for k in ema)
    final_live = _load(out, "model_encdec_final_state.pth")
    assert all(torch.equal(final_live[k], live[k]) for k in live)
    # torch's keys only: the decay is configuration, not optimizer state
    opt = ck["optimizer_encdec"]
    assert set(opt) == {"state", "param_groups"}
    assert set(opt["param_groups"][0]) <= TORCH_ADAM_KEYS
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in opt["state"].values())


def test_train_cli_resumes_the_average(ema_run, tmp_path, caplog, monkeypatch):
    from vae2.optim import FusedAdam
    path, _, _, ck1 = ema_run
    shutil.copytree(str(path / "output"), str(tmp_path / "output"))
    seen = []
    step = FusedAdam.step

    def spy(self):
        step(self)
        seen.append(torch.cat([f.data.double().cpu() for f in self.flats]))
    monkeypatch.setattr(FusedAdam, "step", spy)
    with caplog.at_level(logging.INFO):
        out = _train(tmp_path, *EMA, "TRAIN.RESUME", "True", end_epoch=2)
    assert any("=> loaded checkpoint (epoch 1)" in r.getMessage() for r in caplog.records)
    assert not any("no EMA weights" in r.getMessage() for r in caplog.records)
    ck2 = _load(out, "checkpoint_encdec.pth.tar")
    assert ck2["epoch"] == 2 and ck2["ema_updates"] == 4
    assert int(float(ck2["optimizer_encdec"]["state"][0]["step"])) == 4
    # the loaded average went on from its saved value (not re-seeded from the live weights):
    # two more updates of it, within the K = 2 bound
    assert len(seen) == 2 and torch.equal(_flat(ck2["state_dict"]), seen[1])
    e1, got = _flat(ck1["ema_state_dict"]), _flat(ck2["ema_state_dict"])
    ref = e1 + DECAY * (seen[0] - e1)
    ref = ref + DECAY * (seen[1] - ref)
    err = (got - ref).abs()
    bound = 2 * 2.0 ** -21 * torch.stack([e1.abs(), seen[0].abs(), seen[1].abs()]).max(0).values
    print(f"max err = {float(err.max()):.3e}, max err/bound = "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    for k in ck2["state_dict"]:  # the buffers are still the live ones
        if _is_buffer(k):
            assert torch.equal(ck2["ema_state_dict"][k], ck2["state_dict"][k]), k


def test_default_run_has_todays_files_and_keys(plain_run):
    _, out, ck = plain_run
    assert set(ck) == {"epoch", "state_dict", "optimizer_encdec"}
    assert not os.path.exists(os.path.join(out, "model_encdec_final_state_ema.pth"))
    assert os.path.isfile(os.path.join(out, "model_encdec_final_state.pth"))


def test_resume_without_saved_average_starts_it_at_the_first_update(plain_run, tmp_path, caplog):
    path, _, _ = plain_run
    shutil.copytree(str(path / "output"), str(tmp_path / "output"))
    with caplog.at_level(logging.INFO):
        out = _train(tmp_path, *EMA, "TRAIN.RESUME", "True", end_epoch=2)
    assert sum("no EMA weights" in r.getMessage() for r in caplog.records) == 1
    ck = _load(out, "checkpoint_encdec.pth.tar")
    assert ck["epoch"] == 2 and ck["ema_updates"] == 2
    assert all(torch.isfinite(v).all() for v in ck["ema_state_dict"].values()
               if v.is_floating_point())


@pytest.mark.parametrize("bad", ["1.0", "-0.1"])
def test_train_cli_rejects_a_decay_outside_the_range(tmp_path, bad):
    with pytest.raises(ValueError, match="EMA_DECAY"):
        _train(tmp_path, *BASE, "MI355X.EMA_DECAY", bad)
    assert not os.path.exists(os.path.join(_out(tmp_path), "checkpoint_encdec.pth.tar"))


def test_inference_cli_evaluates_the_average(ema_run, caplog):
    path, out, _, ck = ema_run
    with caplog.at_level(logging.INFO):
        res = _infer(path, *BASE, "MI355X.EVAL_EMA", "True")
    lines = [r.getMessage() for r in caplog.records if "loaded EMA weights" in r.getMessage()]
    assert lines == ["=> loaded EMA weights (epoch 1, 2 updates)"], caplog.text
    assert not any("=> loaded checkpoint" in r.getMessage() for r in caplog.records)
    assert len(res) == 2  # 4 clips, batch 2
    for _, per in res:
        for tag in ("x2t", "x3t"):
            m = per[tag]  # [samples][frames][recon, ssim, msssim, psnr]
            assert m.shape == (2, 3, 4)
            # MS-SSIM is written as nan below its size bound (vae2.evaluate): not at 32x64
            assert np.isfinite(m[..., [0, 1, 3]]).all()


def test_inference_cli_needs_the_average_in_the_checkpoint(plain_run):
    path, _, _ = plain_run
    with pytest.raises(ValueError, match="EVAL_EMA"):
        _infer(path, *BASE, "MI355X.EVAL_EMA", "True")
