"""Microbenchmark of the reconstruction-loss kernels on one prediction / target pair of the
benchmark geometry: NHWC (8, 128, 256, 9), ps = 9 (or --shape N H W C).

    python vae-2_amd/tools/loss_bench.py [--iters 100] [--warmup 10] [--shape N H W C]
        [--train-iters K] [--json out.json]

Times, alternating, each call between its own pair of HIP events (a forward is two launches,
the tile kernel and the one-block sum):
  vae2_l1_fwd / vae2_l1_bwd                the yardstick: the L1 term every run already pays
  vae2_ssim_loss_fwd / vae2_ssim_loss_bwd  the SSIM term of MI355X.SSIM_LAMBDA (with the
                                           model's a, b coefficients)
  vae2_ssim                                the evaluation kernel on the same data as N * C
                                           NCHW planes (no affine, no gradient)
and prints the medians with the algorithmic bytes (a forward reads p and t, a backward reads
p and t and writes dp: 4 B per element each) and the fused multiply-adds of the window
filters, counted from the shapes and the kernels' tiles (csrc/ssim_loss.hip: a forward tile is
16 x 32 of the valid map with a 26-row halo; a backward tile is 16 x 16 of dp, the five
filtered maps on 36 x 26, the three derivative maps on 26 x 26).  Tensors of this size stay
resident in the 256 MiB Infinity Cache between launches, so the byte rates are not HBM rates.

--train-iters K (K >= 50) also runs tools/train.py for one epoch of K iterations at the
YAML's geometry on synthetic clips, ELBO only, with MI355X.SSIM_LAMBDA 0 and 0.5 alternated
(0, 0.5, 0, 0.5; each run a fresh process) and records the logged per-iteration `Time` values
of every PRINT_FREQ line.
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

import torch

import _init_paths  # noqa: F401

from vae2 import metrics, ops  # noqa: E402
from vae2._lib import Act, call, load  # noqa: E402
from vae2.ops import ptr, stream_ptr  # noqa: E402

from optim_bench import YAML, time_launches  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TAPS = 11


def fma_counts(n, h, w, c):
    """Window-filter FMAs of the two SSIM-loss kernels and of vae2_ssim (16 x 64 tiles)."""
    def tiles(a, b, th, tw):
        return -(-a // th) * -(-b // tw)
    ho, wo = h - 10, w - 10
    fwd = n * c * tiles(ho, wo, 16, 32) * (26 * 32 + 16 * 32) * 5 * TAPS
    bwd = n * c * tiles(h, w, 16, 16) * ((36 * 26 + 26 * 26) * 5 * TAPS
                                         + (26 * 16 + 16 * 16) * 3 * TAPS)
    ev = n * c * tiles(ho, wo, 16, 64) * (26 * 64 + 16 * 64) * 5 * TAPS
    return {"vae2_ssim_loss_fwd": fwd, "vae2_ssim_loss_bwd": bwd, "vae2_ssim": ev}


def train_times(iters, lambdas=(0.0, 0.5, 0.0, 0.5)):
    """The PRINT_FREQ lines' `Time` (the running mean seconds per iteration) of one-epoch
    tools/train.py runs, one fresh process per entry of lambdas."""
    import tempfile
    from config import config
    config.defrost()
    config.merge_from_file(YAML)
    config.freeze()
    batch = config.TRAIN.BATCH_SIZE_PER_GPU
    runs = []
    for lam in lambdas:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [sys.executable, os.path.join(HERE, "train.py"), "--cfg", YAML,
                   "OUTPUT_DIR", os.path.join(tmp, "output"), "LOG_DIR", os.path.join(tmp, "log"),
                   "MI355X.SYNTHETIC_DATA", "True", "MI355X.ELBO_ONLY", "True",
                   "MI355X.DEFER_CHECKS", "True", "TRAIN.END_EPOCH", "1", "PRINT_FREQ", "10",
                   "MI355X.SYNTHETIC_CLIPS", str(batch * iters),
                   "MI355X.SSIM_LAMBDA", str(lam)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"train.py failed ({r.returncode}):\n{r.stderr[-2000:]}")
            pts = [(int(i), float(t)) for i, t in
                   re.findall(r"Iter:\[(\d+)/\d+\], Time: ([0-9.]+)", r.stdout + r.stderr)]
            if not pts or pts[-1][0] < iters - 10:
                raise RuntimeError(f"train.py logged {len(pts)} PRINT_FREQ lines")
            ssim = re.findall(r"loss_xt_ssim: ([0-9.eE+-]+)", r.stdout + r.stderr)
            runs.append({"ssim_lambda": lam, "iterations": iters, "batch": batch,
                         "time_s_running_mean": {str(i): t for i, t in pts},
                         "last_time_s": pts[-1][1],
                         "loss_xt_ssim_first_last": [float(ssim[0]), float(ssim[-1])]
                         if ssim else None})
            print(f"  train.py SSIM_LAMBDA {lam}: Time {pts[-1][1]:.2f} s/iter after "
                  f"{pts[-1][0] + 1} iterations")
    return runs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 128, 256, 9],
                    metavar=("N", "H", "W", "C"))
    ap.add_argument("--train-iters", type=int, default=0,
                    help="also time tools/train.py epochs of this many iterations (>= 50)")
    ap.add_argument("--json", default="")
    a = ap.parse_args(argv)
    if a.iters < 100:
        ap.error("--iters must be at least 100 (the median of fewer launches is not reported)")
    if a.train_iters and a.train_iters < 50:
        ap.error("--train-iters must be at least 50")
    n, h, w, c = a.shape
    dev = torch.device("cuda")
    numel = n * h * w * c
    print(f"prediction / target: NHWC ({n}, {h}, {w}, {c}), ps = {c}: {numel} fp32 elements "
          f"({4 * numel / 1e6:.1f} MB each)")
    g = torch.Generator().manual_seed(0)
    t = torch.randn((n, h, w, c), generator=g).to(dev)
    p = (t.cpu() + 0.3 * torch.randn((n, h, w, c), generator=g)).to(dev)
    dp = torch.empty_like(p)
    gout = torch.ones((), device=dev)
    out = torch.empty((), device=dev)
    act = Act(n, h, w, c, c)
    ref = ctypes.byref(act)
    lib = load()
    ws32 = torch.empty(lib.vae2_reduce_ws_size(numel), device=dev)
    ws64 = torch.empty(lib.vae2_ssim_loss_ws_size(ref), dtype=torch.float64, device=dev)
    ca, cb = ops.ssim_coeffs(dev, c)
    # the evaluation kernel's view of the same data: N * C planes
    pn = p.permute(0, 3, 1, 2).contiguous()
    tn = t.permute(0, 3, 1, 2).contiguous()
    win = metrics._win(dev, TAPS, 1.5)
    wsm = torch.empty(lib.vae2_metrics_ws_size(n * c, h, w), dtype=torch.float64, device=dev)
    outm = torch.empty((n * c, 2), dtype=torch.float64, device=dev)
    s = stream_ptr()
    scale = 1.0 / n

    def l1_fwd():
        call("vae2_l1_fwd", ptr(p), ref, ptr(t), ref, scale, ptr(ws32), ptr(out), s)

    def l1_bwd():
        call("vae2_l1_bwd", ptr(p), ref, ptr(t), ref, ptr(gout), scale, ptr(dp), ref, 0.0, s)

    def ssim_fwd():
        call("vae2_ssim_loss_fwd", ptr(p), ref, ptr(t), ref, ptr(ca), ptr(cb), 1e-4, 9e-4, scale,
             ptr(ws64), ptr(out), s)

    def ssim_bwd():
        call("vae2_ssim_loss_bwd", ptr(p), ref, ptr(t), ref, ptr(ca), ptr(cb), 1e-4, 9e-4,
             ptr(gout), scale, ptr(dp), ref, 0.0, s)

    def ssim_eval():
        call("vae2_ssim", ptr(pn), ptr(tn), n * c, h, w, ptr(win), TAPS, 1e-4, 9e-4, ptr(wsm),
             ptr(outm), s)

    rows = [("vae2_l1_fwd", l1_fwd, 8), ("vae2_l1_bwd", l1_bwd, 12),
            ("vae2_ssim_loss_fwd", ssim_fwd, 8), ("vae2_ssim_loss_bwd", ssim_bwd, 12),
            ("vae2_ssim", ssim_eval, 8)]
    times = time_launches([fn for _, fn, _ in rows], a.iters, a.warmup)
    fmas = fma_counts(n, h, w, c)
    res = {"shape": [n, h, w, c], "ps": c, "iters": a.iters,
           "note": "operands are Infinity-Cache resident between launches: the byte rates are "
                   "not HBM rates"}
    for (name, _, bpe), ts in zip(rows, times):
        med = statistics.median(ts)
        res[name] = {"median_us": med, "min_us": min(ts), "max_us": max(ts),
                     "bytes": bpe * numel, "GBps": bpe * numel / med / 1e3}
        line = (f"  {name:20s} median {med:8.1f} us  (min {min(ts):.1f}, max {max(ts):.1f})  "
                f"{bpe * numel / 1e6:5.1f} MB  {bpe * numel / med / 1e3:8.1f} GB/s")
        if name in fmas:
            res[name]["fma"] = fmas[name]
            res[name]["TFMAps"] = fmas[name] / med / 1e6
            line += f"  {fmas[name] / 1e9:.2f} GFMA  {fmas[name] / med / 1e6:.2f} TFMA/s"
        print(line)
    pair = res["vae2_ssim_loss_fwd"]["median_us"] + res["vae2_ssim_loss_bwd"]["median_us"]
    res["ssim_pair_us"] = pair
    res["l1_pair_us"] = res["vae2_l1_fwd"]["median_us"] + res["vae2_l1_bwd"]["median_us"]
    print(f"  one SSIM forward + backward: {pair:.1f} us; three of them (xt, x2t, x3t): "
          f"{3 * pair:.1f} us per step")
    if a.train_iters:
        res["train"] = train_times(a.train_iters)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
    sys.exit(0)
