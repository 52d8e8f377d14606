"""The drop-in CLI (vae-2_amd/tools/train.py) with TRAIN.OPTIMIZER sgd: the reference's
default optimizer (config/default.py: MOMENTUM 0.9, WD 0.0001, NESTEROV False) trains,
writes torch.optim.SGD-format optimizer checkpoints and resumes from them."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "vae-2_amd", "tools")
YAML = os.path.join(ROOT, "vae-2_amd", "experiments", "vae2_w18_small_v2_128x256.yaml")

pytestmark = pytest.mark.gpu


def _train(tmp_path, *opts, cfg=YAML, size="[64, 32]"):
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import train  # vae-2_amd/tools/train.py
    from config import config
    config.defrost()
    config.merge_from_file(cfg)  # reset anything a previous run merged
    config.freeze()
    argv = ["--cfg", cfg, "OUTPUT_DIR", str(tmp_path / "output"), "LOG_DIR", str(tmp_path / "log"),
            "TRAIN.IMAGE_SIZE", size, "TRAIN.BATCH_SIZE_PER_GPU", "2",
            "MI355X.SYNTHETIC_CLIPS", "4", "PRINT_FREQ", "1", "MI355X.DEFER_CHECKS", "True",
            *opts]
    train.main(argv)
    return os.path.join(str(tmp_path / "output"), "cityscapessequence",
                        os.path.basename(cfg).split(".")[0])


def _load(out, name):
    return torch.load(os.path.join(out, name), map_location="cpu", weights_only=True)


def _check_sgd_state(opt_sd, n_params):
    st = opt_sd["state"]
    assert sorted(st) == list(range(n_params))
    for s in st.values():
        assert set(s) == {"momentum_buffer"}
        assert torch.isfinite(s["momentum_buffer"]).all()
    grp = opt_sd["param_groups"][0]
    assert grp["momentum"] == 0.9 and grp["weight_decay"] == 0.0001
    assert grp["nesterov"] is False and grp["dampening"] == 0.0 and grp["maximize"] is False
    assert grp["params"] == list(range(n_params))


def test_train_cli_sgd_elbo_checkpoint_and_resume(tmp_path, monkeypatch):
    sgd = ("TRAIN.OPTIMIZER", "sgd", "MI355X.ELBO_ONLY", "True")
    out = _train(tmp_path, "TRAIN.END_EPOCH", "1", *sgd)
    ck = _load(out, "checkpoint_encdec.pth.tar")
    assert ck["epoch"] == 1
    keys = [k for k in ck["state_dict"] if not any(s in k for s in ("running_", "num_batches"))]
    _check_sgd_state(ck["optimizer_encdec"], len(keys))
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())
    assert any(float(s["momentum_buffer"].abs().max()) > 0
               for s in ck["optimizer_encdec"]["state"].values())
    # resume: one more epoch; the reloaded momentum buffers are in use (the optimizer's device
    # step counter says "not the first step" after the load, so buf = g is not taken again)
    from vae2.optim import FusedSGD
    seen = []
    load = FusedSGD.load_state_dict

    def spy(self, sd):
        load(self, sd)
        seen.append((self.step_count, self.momentum, self.weight_decay,
                     [m.cpu().clone() for m in self.momentum_buffer]))
    monkeypatch.setattr(FusedSGD, "load_state_dict", spy)
    _train(tmp_path, "TRAIN.END_EPOCH", "2", "TRAIN.RESUME", "True", *sgd)
    assert len(seen) == 1
    steps, momentum, wd, bufs = seen[0]
    assert steps >= 1 and momentum == 0.9 and wd == 0.0001
    saved = torch.cat([ck["optimizer_encdec"]["state"][i]["momentum_buffer"].reshape(-1)
                       for i in range(len(keys))])
    assert torch.equal(torch.cat(bufs), saved)
    ck2 = _load(out, "checkpoint_encdec.pth.tar")
    assert ck2["epoch"] == 2
    _check_sgd_state(ck2["optimizer_encdec"], len(keys))
    w1 = ck["state_dict"]["encdec_model.conv1.weight"]
    w2 = ck2["state_dict"]["encdec_model.conv1.weight"]
    assert not torch.equal(w1, w2)
    assert all(torch.isfinite(v).all() for v in ck2["state_dict"].values()
               if v.is_floating_point())


def test_train_cli_sgd_gan_step(tmp_path):
    out = _train(tmp_path, "TRAIN.END_EPOCH", "1", "TRAIN.OPTIMIZER", "sgd",
                 "TRAIN.GAN_LAMBDA", "1.0", "MI355X.ELBO_ONLY", "False")
    ckd = _load(out, "checkpoint_D.pth.tar")
    assert ckd["epoch"] == 1
    d_keys = [k for k in ckd["state_dict"] if not any(s in k for s in ("running_", "num_batches"))]
    _check_sgd_state(ckd["optimizer_D"], len(d_keys))
    ck = _load(out, "checkpoint_encdec.pth.tar")
    assert "momentum_buffer" in ck["optimizer_encdec"]["state"][0]


def test_train_cli_rejects_unknown_optimizer(tmp_path):
    with pytest.raises(ValueError, match="Only Support SGD and ADAM optimizer"):
        _train(tmp_path, "TRAIN.END_EPOCH", "1", "TRAIN.OPTIMIZER", "rmsprop",
               "MI355X.ELBO_ONLY", "True")
