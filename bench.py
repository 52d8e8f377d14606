"""Benchmark: VAE² ELBO training step on MI355X (BASELINE.json metric).

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints one JSON line (metric, value,
unit, higher_is_better, dtype, ms_per_step, ...).  --dump-outputs DIR also writes what the
last timed step returned (the loss terms and the three predicted clips) as DIR/<name>.npy.
Everything else the benchmark measures (the roofline / per-family profile, the live
rocprofv3 passes over the dominant kernel, the CPU baseline) runs only with --full.

Workload (BASELINE.json configs[2], the metric's config): the shipped experiment
YAML (vae-2_amd/experiments/vae2_w18_small_v2_128x256.yaml) through the drop-in
surface — lib/config, models.enc_hrnet factories, utils.utils.FullModel_encdec,
core.criterion — HRNet-W18-small-v2 encoder + two decoders + posterior net,
128x256 clips of 3 x CLIP_LENGTH=3 = 9 frames, 8 clips per GPU (weak scaling; 64
clips at 8 GPUs), fp32, random-init weights (seed 0, the reference's init),
synthetic Gaussian clips resident in HBM.  One step = posterior net +
reparameterisation + encoder + 2 decoders forward, L1 x3 + KL, backward, RCCL
gradient all-reduce (N > 1, SyncBN statistics), Adam.  frames/s = clips * 9 /
step time, whole job.  The step is captured once as a HIP graph (vae2.graph.StepGraph:
same kernels, one launch, bit-identical to eager steps -- tests/test_graph_gpu.py; at
N > 1 with the RCCL collectives inside, tests/test_dist_rccl_gpu.py) and replayed; the
noise is drawn on the device inside the step so every replay samples fresh noise.

With --full the printed JSON also carries:
  roofline      the dominant kernel by time (one instantiation, as rocprofv3 names
                it), timed live with HIP events around its launches during
                --roofline-steps eager steps after the timed region (every C-ABI
                call isolated from the side streams, so the span is the kernel's
                own execution); achieved = algorithmic FLOPs (convs) or bytes per
                launch / average launch time; traffic = HBM bytes per launch from the
                committed PMC measurement (profiles/*_pmc_traffic.json) when present;
                step_frac = the step's algorithmic conv FLOPs / step time / fp32 peak
  families      the same profiled steps per kernel family (conv fwd / dgrad /
                wgrad, BatchNorm, heads, fuse/resample, ...): ms per step, launches,
                algorithmic GFLOP or GB and the rate against the roofline; the full
                per-kernel and per-layer-shape tables go to --profile-json
  cpu_baseline  the CPU oracle (oracle/ref_cpu.py, the reference's ops on CPU)
                timed on this host's cores, rank 0 at N=1 only, on a bounded sample.
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "vae-2_amd")
for _p in (ROOT, PKG, os.path.join(PKG, "lib")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

YAML = os.path.join(PKG, "experiments", "vae2_w18_small_v2_128x256.yaml")
METRIC = "training frames/sec on 128x256 8-frame Cityscapes clips, 1/2/4/8 MI355X"
# ELBO FLOPs per clip at 128x256 (FlopCounterMode over the reference)
REF_GFLOP_PER_CLIP = {(128, 256): 538.1, (64, 64): 67.27, (32, 32): 16.82, (256, 512): 2152.0}
DUMP_BYTES = 48 << 20  # --dump-outputs: bytes of array data written in all


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cfg", default=YAML)
    ap.add_argument("--batch", type=int, default=None, help="clips per GPU (YAML: 8)")
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--clip-length", type=int, default=None)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the profiled roofline / per-family "
                         "phase, the live rocprofv3 passes over the dominant kernel and the "
                         "CPU baseline (each can be switched off with its --no-* option); a "
                         "plain run prints the headline line only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned (loss terms, predicted "
                         "clips; rank 0's) as DIR/<name>.npy, float32, at most "
                         f"{DUMP_BYTES >> 20} MiB in all (a fixed seeded sample of each array "
                         "beyond that)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=2,
                    help="clips per CPU step (a bounded sample: 1 warm-up + --cpu-steps timed "
                         "steps at 8 clips would take ~2 min of the driver's run)")
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--roofline-steps", type=int, default=3)
    ap.add_argument("--profile-json", default=None,
                    help="write the live per-family / per-kernel / per-shape tables here")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32",
                    help="conv MFMA operand precision (bf16: operands rounded to bf16, fp32 "
                         "accumulation / storage / BN / optimizer; a separate, looser-"
                         "tolerance line, BASELINE configs 2 and 5)")
    ap.add_argument("--conv-grouping", choices=("on", "off"), default="off",
                    help="one launch for the direct-3x3 convs of a depth level (A/B)")
    ap.add_argument("--lazy-bn", choices=("on", "off"), default="on",
                    help="BasicBlock bn1 normalised inside conv2's staging, never stored "
                         "(vae2.ops.LazyBN; A/B)")
    ap.add_argument("--part-bn", choices=("on", "off"), default="on",
                    help="BatchNorm backward partials from the single consumer conv's data-"
                         "gradient epilogue where that conv is a 1x1 GEMM / gather-kernel conv "
                         "(vae2.ops.PartBN; A/B)")
    ap.add_argument("--conv-algo", type=int, default=None,
                    help="vae2_conv2d_set_algo bits (A/B of kernel choices; default: auto)")
    ap.add_argument("--heads-algo", type=int, default=None,
                    help="vae2_heads_set_algo value (A/B of the head kernel variants)")
    ap.add_argument("--conv-tune", default="",
                    help="vae2_conv2d_set_tune key=value[,key=value] (launch-shape A/B)")
    ap.add_argument("--side-streams", choices=("on", "off"), default="on",
                    help="posterior net / past decoder on side HIP streams (A/B)")
    ap.add_argument("--syncbn-exchange", choices=("ipc", "rccl"), default="ipc",
                    help="N > 1: the SyncBN statistics through the one-shot IPC peer all-reduce "
                         "kernel (vae2_syncbn_allreduce) or RCCL all_reduce")
    ap.add_argument("--full-step", action="store_true",
                    help="the reference's full training iteration (function.py:443-512): "
                         "GAN_LAMBDA 1 (both LSGAN generator terms through the two "
                         "discriminators) + the discriminator step with its own Adam")
    ap.add_argument("--level-lanes", type=int, default=None,
                    help="concurrent streams per HRNet depth level inside the captured graph "
                         "(vae2.ops.LEVEL_LANES; 0/1: one stream; negative: forward only)")
    ap.add_argument("--no-pmc", action="store_true",
                    help="skip the live rocprofv3 passes over the dominant kernel (PMC HBM "
                         "traffic, trace-averaged duration)")
    ap.add_argument("--graph", choices=("auto", "on", "off"), default="auto",
                    help="replay the step as one captured HIP graph (auto = on, at every world "
                         "size: the distributed step's RCCL collectives are captured in "
                         "thread-local capture mode, vae2/graph.py; bit-identical to eager "
                         "steps, tests/test_dist_rccl_gpu.py).  The eager step measured 0-3%% "
                         "faster on an idle host but 10-20%% slower when the host CPUs are "
                         "busy; the graph replay is stable")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.profile_json and not args.full:
        ap.error("--profile-json is written by the profiled phase: add --full")
    return args


def load_config(args):
    """The experiment YAML through the drop-in config surface, plus shape overrides."""
    from config import config
    config.defrost()
    config.merge_from_file(args.cfg)
    opts = []
    if args.batch is not None:
        opts += ["TRAIN.BATCH_SIZE_PER_GPU", str(args.batch)]
    if args.height is not None or args.width is not None:
        w, h = config.TRAIN.IMAGE_SIZE
        opts += ["TRAIN.IMAGE_SIZE", f"[{args.width or w}, {args.height or h}]"]
    if args.full_step:
        opts += ["TRAIN.GAN_LAMBDA", "1.0", "MI355X.ELBO_ONLY", "False"]
    if args.clip_length is not None:  # 3 segments of L frames
        opts += ["TRAIN.CLIP_LENGTH", str(args.clip_length),
                 "DATASET.NUM_CLASSES", str(args.clip_length)]
    config.merge_from_list(opts)
    config.freeze()
    return config


def build_models(config, with_d=False):
    """train.py's construction order (train.py:79-82) through the lib/ factories."""
    import models
    torch.manual_seed(0)
    ed = models.enc_hrnet.get_encdec_model(config)
    ez = models.enc_hrnet.get_encz_model(config)
    if not with_d:
        return ed, ez
    return (ed, ez, models.enc_hrnet.get_D_sequence_model(config),
            models.enc_hrnet.get_D_frame_model(config))


def _child_args(args):
    """bench.py arguments of a child run with this run's workload and kernel choices."""
    a = ["--cfg", args.cfg, "--dtype", args.dtype, "--lazy-bn", args.lazy_bn,
         "--part-bn", args.part_bn,
         "--side-streams", args.side_streams, "--conv-grouping", args.conv_grouping]
    for flag, v in (("--batch", args.batch), ("--height", args.height), ("--width", args.width),
                    ("--clip-length", args.clip_length), ("--conv-algo", args.conv_algo),
                    ("--heads-algo", args.heads_algo), ("--level-lanes", args.level_lanes)):
        if v is not None:
            a += [flag, str(v)]
    if args.conv_tune:
        a += ["--conv-tune", args.conv_tune]
    if args.full_step:
        a += ["--full-step"]
    return a


def _kname(name):
    return re.sub(r"\(.*\)$", "", name).replace("vae2::", "").replace("void ", "").strip()


def live_kernel_passes(args, kernel):
    """rocprofv3 over child runs of this benchmark, restricted to the dominant kernel
    (MI355X_MICROARCH.md HBM / rocprofv3 recipe): one --pmc FETCH_SIZE pass and one --pmc
    WRITE_SIZE pass over 2 eager steps (separate passes, the counters' own runs), and one
    --kernel-trace --stats pass over 3 graph-replayed steps (the timed region's form).
    Returns ({hbm bytes per launch, fetch/write split, launches}, {trace avg us, calls}) or
    Nones with the reason -- measured in this run, not looked up."""
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, None, "rocprofv3 not found"
    sys.path.insert(0, os.path.join(ROOT, "vae-2_amd", "tools"))
    import pmc_traffic as pt
    regex = re.sub(r"[<>()\[\]*+?.|^$]", ".", kernel)
    base = [sys.executable, os.path.abspath(__file__), "--warmup", "1", "--no-cpu-baseline",
            "--no-roofline", "--no-pmc"] + _child_args(args)
    env = dict(os.environ, TMPDIR="/tmp")
    tmp = tempfile.mkdtemp(prefix="vae2_rocprof_", dir="/tmp")
    try:
        def run(extra, sub, tail):
            cmd = [exe] + extra + ["--kernel-include-regex", regex, "-f", "csv", "-d",
                                   os.path.join(tmp, sub), "-o", "run", "--"] + base + tail
            r = subprocess.run(cmd, timeout=300, capture_output=True, env=env, cwd=ROOT)
            return r.returncode
        vals = {}
        for c in ("FETCH_SIZE", "WRITE_SIZE"):
            rc = run(["--pmc", c], c, ["--steps", "2", "--graph", "off"])
            if rc != 0:
                return None, None, f"rocprofv3 --pmc {c} pass exited {rc}"
            vals[c] = pt.per_launch(os.path.join(tmp, c), c, kernel)
            if not vals[c]:
                return None, None, f"no {c} samples for {kernel}"
        fetch = sum(vals["FETCH_SIZE"]) / len(vals["FETCH_SIZE"]) * 1024 * 2.0
        write = sum(vals["WRITE_SIZE"]) / len(vals["WRITE_SIZE"]) * 1024
        pmc = {"hbm_bytes_per_launch": fetch + write, "fetch_bytes_per_launch": fetch,
               "write_bytes_per_launch": write, "launches": len(vals["FETCH_SIZE"]),
               "note": "FETCH_SIZE x2 (gfx950 16-byte-read calibration) + WRITE_SIZE, KiB x1024, "
                       "mean over the dominant kernel's launches of 2 eager steps"}
        trace = None
        if run(["--kernel-trace", "--stats"], "trace", ["--steps", "3", "--graph", "on"]) == 0:
            import csv
            import glob
            for f in glob.glob(os.path.join(tmp, "trace", "**", "*kernel_stats.csv"),
                               recursive=True):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        if _kname(row["Name"]) == kernel:
                            trace = {"avg_us": float(row["AverageNs"]) / 1e3,
                                     "calls": int(row["Calls"])}
        return pmc, trace, None
    except subprocess.TimeoutExpired as e:
        return None, None, f"rocprofv3 pass timed out ({e.timeout} s)"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the newest committed PMC measurement
    (profiles/*_pmc_traffic.json, written by tools/pmc_traffic.py from separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this benchmark), else None."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json"))):
        try:
            with open(f) as fh:
                d = json.load(fh)
        except (OSError, ValueError):
            continue
        if d.get("kernel") == kernel.replace("void ", ""):
            best = d
    return best


def head_skip_gflop_per_clip(ed, H, W):
    """FLOPs the reference spends on its 270-channel heads that the commuted per-branch
    head path (vae2/heads.py) does not: per head and per direction (forward, data grad,
    weight grad) the full-resolution C x C 1x1 conv, 2*C*C*H*W, against the branch products
    at branch resolution, 2*C*sum_b(c_b*H_b*W_b); 3 heads in each of the encoder and the two
    decoders (enc_hrnet.py:833-847)."""
    split = [int(c) for c in ed.last_stage_channels]
    C = sum(split)
    sizes = [(H, W)]
    for _ in split[1:]:
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    branch = sum(c * h * w for c, (h, w) in zip(split, sizes))
    return 3 * 3 * 3 * 2.0 * C * (C * H * W - branch) / 1e9  # nets x heads x directions


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(args, config, gpu_batch):
    """Oracle ELBO step (fwd + bwd + torch Adam) on the host CPU, bounded sample."""
    from oracle import ref_cpu
    aff = len(os.sched_getaffinity(0))
    # the box's CPU share for one GPU is OMP_NUM_THREADS (16); never more than affinity
    cores = min(aff, int(os.environ.get("OMP_NUM_THREADS", aff)))
    torch.set_num_threads(cores)
    L = config.TRAIN.CLIP_LENGTH
    W, H = config.TRAIN.IMAGE_SIZE
    B = args.cpu_batch or gpu_batch
    ed, ez = build_models(config)
    params = list(ez.parameters()) + list(ed.parameters())
    opt = torch.optim.Adam(params, lr=config.TRAIN.LR)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(B, 3 * L, H, W, generator=g) for _ in range(3)]

    def step():
        opt.zero_grad()
        e = torch.randn(B, ez.z_dim, 1, 1)
        c = torch.randn(B, ez.z_dim, 1, 1)
        terms, _, _ = ref_cpu.elbo(ez, ed, *xs, e, c)
        terms["loss_all"].backward()
        opt.step()

    step()  # warm-up (allocator, oneDNN primitive caches)
    t0 = time.perf_counter()
    for _ in range(args.cpu_steps):
        step()
    dt = (time.perf_counter() - t0) / args.cpu_steps
    return {"value": round(B * 3 * L / dt, 3), "unit": "frames/s", "cores": cores,
            "kind": "port",
            "sample": f"oracle/ref_cpu.py ELBO step fwd+bwd+torch Adam (the reference's ATen "
                      f"ops), HRNet-W18-small-v2 {H}x{W}, {B} clips x {3 * L} frames per step "
                      f"(the GPU runs {gpu_batch} clips/step), fp32, "
                      f"1 warm-up + {args.cpu_steps} timed "
                      f"step(s) ({dt:.2f} s/step), torch threads={cores} = the box's CPU "
                      f"share for one GPU (OMP_NUM_THREADS; {aff} in the affinity mask), "
                      f"CPU: {cpu_model()}"}


def dump_outputs(dirname, tensors):
    """Write {name: device tensor} as dirname/<name>.npy (float32).  Within DUMP_BYTES in
    all the arrays are written whole; beyond it every array keeps the same fraction of its
    elements, a sample of its flattened form at sorted indices drawn with a fixed seed, so
    two runs with the same arguments write the same elements."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    total = 4 * sum(t.numel() for t in tensors.values())
    for name, t in tensors.items():
        a = t.detach().to("cpu", torch.float32).contiguous().numpy()
        if total > DUMP_BYTES:
            keep = max(1, a.size * DUMP_BYTES // total)
            if keep < a.size:
                idx = np.random.default_rng(0).choice(a.size, size=keep, replace=False)
                a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(dirname, name + ".npy"), a)


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        torch.cuda.set_device(local)
        os.environ.setdefault("TORCH_NCCL_CUDA_EVENT_CACHE", "0")  # = vae2.dist.prepare_nccl_env
        if "TORCH_NCCL_TRACE_BUFFER_SIZE" not in os.environ:  # flight recorder: the graph
            os.environ.setdefault("TORCH_FR_BUFFER_SIZE", "2000")  # capture's drain reads it
        dist.init_process_group("nccl", init_method="env://")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    from core.criterion import KLLoss, L1Loss, lsgan_adversarial_loss
    from utils.utils import FullModel_D, FullModel_encdec
    from vae2 import dist as vdist
    from vae2 import prof
    from vae2.optim import FusedAdam
    config = load_config(args)
    vdist.set_sync_bn(config.MI355X.SYNC_BN)
    if world > 1 and config.MI355X.SYNC_BN and args.syncbn_exchange == "ipc":
        vdist.init_syncbn_ipc()  # one-shot peer all-reduce (RCCL stays if it does not come up)
    if args.side_streams == "off":
        from vae2 import streams as vstreams
        vstreams.ENABLED = False
    if args.conv_grouping == "on":
        from vae2 import _lib
        _lib.load().vae2_conv2d_set_grouping(1)
    if args.heads_algo is not None:
        from vae2 import _lib
        _lib.load().vae2_heads_set_algo(args.heads_algo)
    if args.conv_algo is not None:
        from vae2 import _lib
        _lib.load().vae2_conv2d_set_algo(args.conv_algo)
    for kv in filter(None, args.conv_tune.split(",")):
        from vae2 import _lib
        k, v = kv.split("=")
        if _lib.load().vae2_conv2d_set_tune(int(k), int(v)) < 0:
            raise SystemExit(f"conv tune key {k}: unknown key or out-of-range value {v}")
    if args.level_lanes is not None:
        from vae2 import ops as vops
        vops.LEVEL_LANES = abs(args.level_lanes)
        vops.LEVEL_LANES_BWD = args.level_lanes > 0  # negative: forward only
    if args.lazy_bn == "off":
        from vae2 import ops as vops
        vops.LAZY_BN = False
    if args.part_bn == "off":
        from vae2 import ops as vops
        vops.PART_BN = False
    if args.dtype == "bf16":
        from vae2 import _lib
        _lib.load().vae2_conv2d_set_mfma_bf16(1)
        prof.set_mfma_dtype("bf16")

    L = config.TRAIN.CLIP_LENGTH
    W, H = config.TRAIN.IMAGE_SIZE
    B = config.TRAIN.BATCH_SIZE_PER_GPU
    full = args.full_step
    if full:
        ed, ez, dseq, dfrm = build_models(config, with_d=True)
    else:
        (ed, ez), dseq, dfrm = build_models(config), None, None
    fm = FullModel_encdec(ez, ed, dseq, dfrm, L1Loss(), KLLoss(),
                          lsgan_adversarial_loss() if full else None,
                          config.TRAIN.X1RECON_LAMBDA, config.TRAIN.X2RECON_LAMBDA,
                          config.TRAIN.X3RECON_LAMBDA, config.TRAIN.GAN_LAMBDA).to(dev)
    fm.train()
    fm.defer_checks = True
    opt = FusedAdam([fm.encz_model, fm.encdec_model], lr=config.TRAIN.LR)
    fmd = opt_d = None
    if full:  # function.py:503-512: D on real x2t vs the detached x2t_hat, its own Adam
        fmd = FullModel_D(dseq, dfrm, lsgan_adversarial_loss()).to(dev)
        fmd.train()
        opt_d = FusedAdam([dseq, dfrm], lr=config.TRAIN.LR)
    if world > 1:
        for o in (opt, opt_d):
            for f in (o.flats if o is not None else []):
                dist.broadcast(f.data, src=0)
    g = torch.Generator().manual_seed(1 + rank)
    xs = [torch.randn(B, 3 * L, H, W, generator=g).to(dev) for _ in range(3)]
    zc = ez.z_dim

    returned = {}  # --dump-outputs: what the step's callee handed back (static under the graph)

    def eager_step():
        opt.zero_grad()
        fm.set_noise(torch.randn(B, zc, 1, 1, device=dev), torch.randn(B, zc, 1, 1, device=dev))
        losses, x1p, x2p, x3p = fm(*xs, 1.0)
        if args.dump_outputs:
            names = ("loss_all", "xt_recon", "x2t_recon", "x3t_recon", "z_kl", "gan_seq",
                     "gan_frame", "xt_hat", "x2t_hat", "x3t_hat")
            returned.update((k, v.detach()) for k, v in zip(names, (*losses, x1p, x2p, x3p))
                            if torch.is_tensor(v))
        losses[0].backward()
        vdist.allreduce_grads(opt.flats)
        opt.step()
        if fmd is not None:
            opt_d.zero_grad()
            ld = fmd(xs[1], x2p.detach())[0]
            if args.dump_outputs:
                returned["d_loss"] = ld.detach()
            ld.backward()
            vdist.allreduce_grads(opt_d.flats)
            opt_d.step()
        return losses[0]

    use_graph = args.graph in ("on", "auto")
    step = eager_step
    if use_graph:
        from vae2.graph import StepGraph
        graph = StepGraph(eager_step, warmup=2)
        step = graph.replay
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    fm.check_anomalies()
    vdist.syncbn_check()  # (IPC SyncBN exchange: no timed-out exchange)

    # ---- timed region: the metric (full stream concurrency, no instrumentation) ----
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)
    fm.check_anomalies()
    vdist.syncbn_check()
    last_loss = float(loss.detach())

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, returned)

    # ---- profiled phase (--full): the same step eager, every C-ABI call timed with HIP
    # events on its stream, isolated from the side streams ----
    profiler = None
    if args.full and not args.no_roofline and args.roofline_steps > 0:
        torch.cuda.synchronize()
        with prof.StepProfiler() as profiler:
            for _ in range(args.roofline_steps):
                eager_step()
        torch.cuda.synchronize()
        fm.check_anomalies()

    if rank == 0:
        ms = 1e3 * elapsed / args.steps
        frames = world * B * 3 * L * args.steps
        out = {
            "metric": METRIC,
            "value": round(frames / elapsed, 2), "unit": "frames/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic (Gaussian Cityscapes-shaped clips resident in HBM; random-init "
                    "weights, reference init seed 0)",
            "config": {"workload": (f"VAE2 full training iteration (ELBO + GAN_LAMBDA 1 "
                                    f"LSGAN terms through both discriminators, Adam; then the "
                                    f"discriminator step, its Adam)" if full else
                                    f"VAE2 ELBO step (encz + encoder + 2 decoders fwd/bwd + "
                                    f"Adam)") + f", HRNet-W18-small-v2, {H}x{W}, {B} clips/GPU "
                                   f"x {3 * L} frames (CLIP_LENGTH={L})",
                       "yaml": os.path.relpath(args.cfg, ROOT),
                       "global_batch": world * B, "frames_per_clip": 3 * L,
                       "image": [H, W], "parallelism": f"dp{world}",
                       "sync_bn": world > 1 and config.MI355X.SYNC_BN,
                       "sync_bn_exchange": vdist.syncbn_exchange() if world > 1 else None,
                       "launch": "hip_graph" if use_graph else "eager",
                       "mfma_operands": ("bf16 (RNE; fp32 accumulation, fp32 activations in "
                                         "HBM, fp32 BN / loss / Adam)" if args.dtype == "bf16"
                                         else "fp32")},
            "last_loss": last_loss,
            # also clips/s and predicted frames/s (2L of the 3L frames a clip
            # carries are predicted: x2t_hat and x3t_hat; xt_hat reconstructs the context)
            "clips_per_s": round(world * B * args.steps / elapsed, 3),
            "predicted_frames_per_s": round(world * B * 2 * L * args.steps / elapsed, 2),
            "peak_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2),
        }
        if profiler is not None:
            n = args.roofline_steps
            summ = profiler.summary(n)
            dom = profiler.dominant(n)
            conv_gf = sum(r.get("gflop_per_step", 0.0) for r in summ["families"])
            ref_gf = REF_GFLOP_PER_CLIP.get((H, W))
            roof = dict(dom)
            live, trace, why = (None, None, "--no-pmc") if args.no_pmc or world > 1 else \
                live_kernel_passes(args, dom["kernel"])
            if live is not None:
                roof["traffic"] = round(live["hbm_bytes_per_launch"])
                roof["traffic_unit"] = "HBM bytes/launch (PMC, measured in this run)"
                roof["traffic_detail"] = {k: (round(v) if isinstance(v, float) else v)
                                          for k, v in live.items()}
                if roof.get("algorithmic_bytes_per_launch"):
                    roof["traffic_over_algorithmic"] = round(
                        live["hbm_bytes_per_launch"] / roof["algorithmic_bytes_per_launch"], 3)
            else:  # fall back to the newest committed measurement of the same kernel
                tr = pmc_traffic(dom["kernel"])
                roof["traffic"] = round(tr["hbm_bytes_per_launch"]) if tr else None
                roof["traffic_unit"] = (f"HBM bytes/launch (PMC, committed profiles/; live "
                                        f"pass unavailable: {why})")
            if trace is not None:
                # the same kernel in the timed region's form (graph replay, side streams
                # concurrent) from rocprofv3's kernel trace: achieved over the trace average
                t_us = trace["avg_us"]
                roof["trace"] = {"avg_us": round(t_us, 2), "calls": trace["calls"],
                                 "achieved": round(roof["achieved"] * roof["avg_launch_us"] / t_us, 2),
                                 "frac": round(roof["frac"] * roof["avg_launch_us"] / t_us, 4),
                                 "source": "rocprofv3 --kernel-trace --stats, 3 graph-replayed "
                                           "steps of this workload, this run"}
            roof["step_frac"] = round(conv_gf / ms / prof.MFMA_PEAK_TF, 4)
            roof["step_gflop"] = round(conv_gf, 1)
            if ref_gf is not None and L == 3 and not full:
                # the noted conv + head FLOPs must equal the reference's FlopCounter total
                # less what the commuted heads legitimately skip (tests assert "reconciled")
                skip = B * head_skip_gflop_per_clip(ed, H, W)
                want = B * ref_gf - skip
                roof["flop_reconciliation"] = {
                    "noted_gflop_per_step": round(conv_gf, 1),
                    "reference_gflop_per_step": round(B * ref_gf, 1),
                    "commuted_head_skip_gflop_per_step": round(skip, 1),
                    "expected_gflop_per_step": round(want, 1),
                    "ratio": round(conv_gf / want, 4),
                    "reconciled": abs(conv_gf / want - 1.0) < 0.01,
                    "note_conflicts": summ["note_conflicts"]}
            if ref_gf is not None and L == 3 and not full:
                roof["step_frac_ref_flops"] = round(
                    B * ref_gf / ms / prof.MFMA_PEAK_TF, 4)
            # the north star's target: the encoder / decoder conv stack as a whole -- every conv
            # family's algorithmic FLOPs over its summed kernel time, against the MFMA peak
            conv = [r for r in summ["families"]
                    if r["name"] in ("conv_fwd", "conv_dgrad", "conv_wgrad", "conv_1x1")]
            c_ms = sum(r["ms_per_step"] for r in conv)
            c_gf = sum(r.get("gflop_per_step", 0.0) for r in conv)
            if c_ms > 0:
                c_tf = c_gf / c_ms
                roof["conv_stack"] = {"families": [r["name"] for r in conv],
                                      "gflop_per_step": round(c_gf, 1),
                                      "kernel_ms_per_step": round(c_ms, 3),
                                      "achieved": round(c_tf, 2), "peak": prof.MFMA_PEAK_TF,
                                      "unit": "TFLOP/s", "bound": "mfma",
                                      "frac": round(c_tf / prof.MFMA_PEAK_TF, 4)}
            roof["measured"] = (f"{n} eager steps after the timed region, every C-ABI call "
                                "timed with HIP events on its stream, isolated from side "
                                "streams")
            out["roofline"] = roof
            out["families"] = {r["name"]: {k: r[k] for k in r if k != "name"}
                               for r in summ["families"]}
            if args.profile_json:
                with open(args.profile_json, "w") as f:
                    json.dump(summ, f, indent=1)
        if args.full and world == 1 and not args.no_cpu_baseline and not full:
            out["cpu_baseline"] = cpu_baseline(args, config, B)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
