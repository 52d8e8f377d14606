"""bench.py's command line: a plain run is the headline line only, --full brings the
profiled phases back, --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_and_full_arguments(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--profile-json", "p.json", "--dump-outputs", "d")
    assert a.full and a.profile_json == "p.json" and a.dump_outputs == "d"
    assert not a.full_step  # --full is its own option, not a prefix of --full-step
    for bad in (["--steps", "0"], ["--profile-json", "p.json"]):
        with pytest.raises(SystemExit):
            _parse(monkeypatch, *bad)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    g = torch.Generator().manual_seed(0)
    t = {"a": torch.randn(3, 5, 7, generator=g), "s": torch.randn((), generator=g),
         "h": torch.randn(4, 6, generator=g).to(torch.bfloat16)}
    bench.dump_outputs(str(tmp_path / "whole"), t)
    for k, v in t.items():
        a = np.load(tmp_path / "whole" / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.float().numpy())
    # over the budget: the same seeded sample of every array on each call, within the budget
    monkeypatch.setattr(bench, "DUMP_BYTES", 200)
    bench.dump_outputs(str(tmp_path / "s1"), t)
    bench.dump_outputs(str(tmp_path / "s2"), t)
    total = 0
    for k, v in t.items():
        a, b = (np.load(tmp_path / d / (k + ".npy")) for d in ("s1", "s2"))
        assert a.dtype == np.float32 and np.array_equal(a, b)
        assert 1 <= a.size <= v.numel()
        assert np.isin(a, v.float().numpy()).all()
        total += a.nbytes
    assert total <= 200
    assert np.load(tmp_path / "s1" / "a.npy").size < t["a"].numel()


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_outputs(tmp_path):
    """A plain run at a small geometry: the result line carries the headline fields and none
    of the --full phases, --steps is the number of timed steps, and the dumped arrays are
    the step's loss terms and predicted clips in float32."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "2", "--warmup", "1", "--height", "32", "--width", "32",
                        "--batch", "2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "frames/s"
    assert d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(2 * 9 / (d["ms_per_step"] / 1e3), rel=1e-3)
    assert not {"roofline", "families", "cpu_baseline"} & set(d)
    names = {"loss_all", "xt_recon", "x2t_recon", "x3t_recon", "z_kl", "xt_hat", "x2t_hat",
             "x3t_hat"}
    assert {f[:-4] for f in os.listdir(out)} == names
    arrs = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    for n in ("xt_hat", "x2t_hat", "x3t_hat"):
        assert arrs[n].shape == (2, 9, 32, 32)
    assert float(arrs["loss_all"].reshape(-1)[0]) == pytest.approx(d["last_loss"], rel=1e-6)
