"""Microbenchmark of the flat-buffer optimizer kernels on one buffer of the size of the
W18-small-v2 encoder-decoder's flat parameter buffer (or --numel N).

    python vae-2_amd/tools/optim_bench.py [--iters 100] [--warmup 10] [--numel N]
        [--clip] [--ema] [--json out.json]

Times vae2_sgd_step_dev (momentum 0.9, weight decay 1e-4: the TRAIN.OPTIMIZER sgd defaults)
and vae2_adam_step_dev, alternating, each launch between its own pair of HIP events (SGD's
first step, which does not read buf, runs before the timed window and the tool checks that
the device first-step flag is clear), and
prints the median time and the algorithmic byte rate (SGD reads p, g, buf and writes p, buf:
20 B per element; Adam reads p, g, m, v and writes p, m, v: 28 B per element).  A buffer of
this size stays resident in the 256 MiB Infinity Cache between launches, so the rates are
not HBM rates.

--clip adds, in the same run and alternating with the two unclipped steps (the yardstick):
the norm pass of gradient clipping (vae2_grad_sumsq + vae2_clip_coeffs between one pair of
events; it reads g: 4 B per element; vae2_grad_sumsq alone as well) and the two clipped steps (the bytes of the unclipped
ones).  Next to each measured ratio the output carries the prediction from the byte counts:
the norm pass 4/20 of SGD's time plus one small launch, the clipped steps level with the
unclipped ones.  The threshold is +inf (coefficient 1), so the timed values stay in range.

--ema adds, in the same run and alternating with the two steps: the weight-average update as
the optimizers launch it (vae2_ema_coeffs + vae2_ema_update_dev between one pair of events; it
reads p and ema and writes ema: 12 B per element), vae2_ema_update_dev alone (what of the
pair is not the small launch) and the first-update form (vae2_ema_update with first = 1, a
copy: 8 B per element).  Predictions from the byte counts: 12/28 of Adam's time and 12/20 of
SGD's, plus one small launch.  The tool checks that the timed device-form launches were not
first updates.
"""
import argparse
import json
import os
import statistics
import sys

import torch

import _init_paths  # noqa: F401

from vae2._lib import call, load  # noqa: E402
from vae2.ops import ptr, stream_ptr  # noqa: E402

YAML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "experiments",
                    "vae2_w18_small_v2_128x256.yaml")


def encdec_numel(cfg_path=YAML):
    """Elements of the flat parameter buffer of the encoder-decoder the YAML describes."""
    import models
    from config import config
    config.defrost()
    config.merge_from_file(cfg_path)
    config.freeze()
    net = models.enc_hrnet.get_encdec_model(config)
    return sum(p.numel() for p in {id(p): p for p in net.parameters()}.values())


def time_launches(fns, iters, warmup):
    """Per-launch HIP-event times (us) of each fn, the fns alternating."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            for _ in range(iters)] for _ in fns]
    for i in range(iters):
        for k, fn in enumerate(fns):
            a, b = evs[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) * 1e3 for a, b in ev] for ev in evs]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--numel", type=int, default=0, help="buffer elements (default: the model's)")
    ap.add_argument("--clip", action="store_true",
                    help="also time the gradient-norm pass and the clipped steps")
    ap.add_argument("--ema", action="store_true",
                    help="also time the weight-average (EMA) update and its first-update form")
    ap.add_argument("--json", default="")
    a = ap.parse_args(argv)
    if a.iters < 50:
        ap.error("--iters must be at least 50 (the median of fewer launches is not reported)")
    n = a.numel or encdec_numel()
    print(f"flat parameter buffer: {n} fp32 elements ({4 * n / 2 ** 20:.1f} MiB)")
    dev = torch.device("cuda")
    p, g, b, m = (torch.randn(n, device=dev) * 0.01 for _ in range(4))
    v = torch.rand(n, device=dev) * 1e-4
    state = torch.tensor([0.0, 1e-6], dtype=torch.float64, device=dev)  # {step, lr}
    astate = state.clone()
    coeffs = torch.zeros(4, device=dev)
    acoeffs = torch.zeros(2, device=dev)
    s = stream_ptr()

    def sgd():
        call("vae2_sgd_step_dev", ptr(p), ptr(g), ptr(b), n, ptr(coeffs), 0.9, 1e-4, 0, s)

    # SGD's first step (buf = g, buf not read: 16 B per element) runs here, outside the timed
    # window; the second vae2_sgd_coeffs call makes every later launch a steady-state step
    call("vae2_sgd_coeffs", ptr(state), 0.9, 0.0, 0, ptr(coeffs), s)
    sgd()
    call("vae2_sgd_coeffs", ptr(state), 0.9, 0.0, 0, ptr(coeffs), s)
    if float(state[0]) != 2.0 or float(coeffs[2]) != 0.0:
        raise RuntimeError("the timed SGD launches would take the first-step path "
                           f"(step {float(state[0])}, first flag {float(coeffs[2])})")
    call("vae2_adam_coeffs", ptr(astate), 0.9, 0.999, ptr(acoeffs), s)

    def adam():
        call("vae2_adam_step_dev", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(acoeffs), 0.9, 0.999,
             1e-8, 0.0, s)
    fns = [sgd, adam]
    rows = [("vae2_sgd_step_dev", 20), ("vae2_adam_step_dev", 28)]
    if a.clip:
        n_ws = int(load().vae2_grad_norm_ws_size(n))
        ws = torch.empty(n_ws, dtype=torch.float64, device=dev)
        clip = torch.zeros(4, device=dev)

        def norm():
            call("vae2_grad_sumsq", ptr(g), n, ptr(ws), s)
            call("vae2_clip_coeffs", ptr(ws), n_ws, float("inf"), ptr(clip), s)

        def sgd_clip():
            call("vae2_sgd_step_dev_clip", ptr(p), ptr(g), ptr(b), n, ptr(coeffs), ptr(clip),
                 0.9, 1e-4, 0, s)

        def adam_clip():
            call("vae2_adam_step_dev_clip", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(acoeffs),
                 ptr(clip), 0.9, 0.999, 1e-8, 0.0, s)

        def sumsq():  # the streaming pass alone: what of the norm pass is not launch cost
            call("vae2_grad_sumsq", ptr(g), n, ptr(ws), s)
        fns += [norm, sgd_clip, adam_clip, sumsq]
        rows += [("vae2_grad_sumsq+vae2_clip_coeffs", 4), ("vae2_sgd_step_dev_clip", 20),
                 ("vae2_adam_step_dev_clip", 28), ("vae2_grad_sumsq", 4)]
    if a.ema:
        ema = torch.empty(n, device=dev)
        estate = torch.zeros(2, dtype=torch.float64, device=dev)  # {updates, -}
        ecoeffs = torch.zeros(4, device=dev)
        decay = 0.999

        def ema_update():
            call("vae2_ema_update_dev", ptr(ema), ptr(p), n, ptr(ecoeffs), s)

        def ema_pair():
            call("vae2_ema_coeffs", ptr(estate), decay, ptr(ecoeffs), s)
            ema_update()

        def ema_first():
            call("vae2_ema_update", ptr(ema), ptr(p), n, decay, 1, s)

        # the first update (a copy) runs here, outside the timed window; the second
        # vae2_ema_coeffs call makes every later device-form launch a steady-state update
        ema_pair()
        call("vae2_ema_coeffs", ptr(estate), decay, ptr(ecoeffs), s)
        if float(estate[0]) != 2.0 or float(ecoeffs[1]) != 0.0:
            raise RuntimeError("the timed EMA launches would take the first-update path "
                               f"(count {float(estate[0])}, first flag {float(ecoeffs[1])})")
        ema_rows = [("vae2_ema_coeffs+vae2_ema_update_dev", 12), ("vae2_ema_update_dev", 12),
                    ("vae2_ema_update(first)", 8)]
        fns += [ema_pair, ema_update, ema_first]
        rows += ema_rows
    times = time_launches(fns, a.iters, a.warmup)
    out = {"numel": n, "iters": a.iters, "sgd_first_step_flag": float(coeffs[2]),
           "sgd_step_counter": float(state[0])}
    for (name, bpe), ts in zip(rows, times):
        med = statistics.median(ts)
        out[name] = {"median_us": med, "min_us": min(ts), "max_us": max(ts),
                     "bytes": bpe * n, "GBps": bpe * n / med / 1e3}
        print(f"  {name:36s} median {med:8.1f} us  (min {min(ts):.1f}, max {max(ts):.1f})  "
              f"{bpe} B/elem  {bpe * n / med / 1e3:8.1f} GB/s")
    ratio = out["vae2_sgd_step_dev"]["median_us"] / out["vae2_adam_step_dev"]["median_us"]
    print(f"  sgd / adam median time: {ratio:.3f}")
    med = {name: out[name]["median_us"] for name, _ in rows}
    ratios = {}
    if a.clip:
        if float(clip[1]) != 1.0:
            raise RuntimeError(f"the clip coefficient is {float(clip[1])}, not 1")
        out["grad_norm"] = float(clip[0])
        ratios.update({
            "norm_pass / sgd": {"measured": med[rows[2][0]] / med["vae2_sgd_step_dev"],
                                "predicted": 4 / 20,
                                "basis": "4 of SGD's 20 B per element at SGD's rate, plus one "
                                         "small launch"},
            "sgd_clip / sgd": {"measured": med["vae2_sgd_step_dev_clip"]
                               / med["vae2_sgd_step_dev"], "predicted": 1.0,
                               "basis": "the same bytes, one more multiply per element"},
            "adam_clip / adam": {"measured": med["vae2_adam_step_dev_clip"]
                                 / med["vae2_adam_step_dev"], "predicted": 1.0,
                                 "basis": "the same bytes, one more multiply per element"},
        })
    if a.ema:
        if float(ecoeffs[1]) != 0.0:
            raise RuntimeError("a timed EMA launch took the first-update path")
        out["ema_update_counter"] = float(estate[0])
        pair, first = med[ema_rows[0][0]], med[ema_rows[2][0]]
        ratios.update({
            "ema / adam": {"measured": pair / med["vae2_adam_step_dev"], "predicted": 12 / 28,
                           "basis": "12 of Adam's 28 B per element at Adam's rate, plus one "
                                    "small launch"},
            "ema / sgd": {"measured": pair / med["vae2_sgd_step_dev"], "predicted": 12 / 20,
                          "basis": "12 of SGD's 20 B per element at SGD's rate, plus one small "
                                   "launch"},
            "ema_first / adam": {"measured": first / med["vae2_adam_step_dev"],
                                 "predicted": 8 / 28,
                                 "basis": "a copy: 8 of Adam's 28 B per element at Adam's rate"},
        })
    if ratios:
        out["ratios"] = ratios
        for k, r in ratios.items():
            print(f"  {k:18s} measured {r['measured']:.3f}  predicted {r['predicted']:.3f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
    sys.exit(0)
