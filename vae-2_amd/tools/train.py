"""VAE² training CLI on MI355X (drop-in for the reference's tools/train.py).

    python tools/train.py --cfg experiments/vae2_w18_small_v2_128x256.yaml [KEY VALUE ...]
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 tools/train.py --cfg ... GPUS "(0,1,2,3,4,5,6,7)"

Flow (reference train.py:55-353): parse args + YAML -> logger -> models (same
factories, same RNG order) -> process group (RCCL) -> dataset / sampler / loader
-> FullModel_encdec -> SyncBN statistics + flat-gradient all-reduce (instead of
DDP) -> SGD or Adam (TRAIN.OPTIMIZER) -> resume -> epoch loop -> rank-0 checkpoints with
the reference's file and key names.

Deliberate differences: `TRAIN.OPTIMIZER: sgd` trains (torch.optim.SGD with
TRAIN.LR / MOMENTUM / WD / NESTEROV over the same two parameter sets as Adam, as
vae2.optim.FusedSGD; the reference crashes there on `p.name`, train.py:234); single-GPU
checkpoints are written (the reference calls `.module` on a non-DDP model,
train.py:322); epochs past END_EPOCH use the main loader when no
DATASET.EXTRA_TRAIN_SET is given (the reference raises a NameError there);
`MI355X.CLIP_GRAD_NORM t` (t > 0) clips the global gradient 2-norm of each optimizer's
parameter set to t inside the fused step (0, the default, is off);
`MI355X.EMA_DECAY d` (0 < d < 1; 0, the default, is off) keeps an exponential moving
average of the generator weights (encz + ED; never the discriminators) on the device,
updated inside the fused step (vae2.optim, ema_decay): checkpoint_encdec.pth.tar then also
holds "ema_state_dict" (the averaged parameters with the live BatchNorm buffers) and
"ema_updates", and the last epoch writes model_encdec_final_state_ema.pth;
tools/inference.py evaluates the average with MI355X.EVAL_EMA True;
`MI355X.SSIM_LAMBDA s` (s > 0; 0, the default, is off) gives every L1 reconstruction term
an SSIM sibling, sum (1 - SSIM) / batch of the de-normalised frames with the weight
s * X?RECON_LAMBDA (vae2.ops.ssim_loss: the evaluation's SSIM without its clip to
[0, 255]), logged as loss_x?t_ssim next to the PRINT_FREQ line;
`MI355X.ELBO_ONLY True` drops the two discriminators (the ELBO step alone; the
reference always builds them and runs the D step); the Cityscapes sequence zips are
decoded once into a uint8 cache and normalised on the GPU (MI355X.CLIP_CACHE, default),
or replaced by MI355X.SYNTHETIC_DATA clips when that switch is set; the dataset is given
TRAIN.CLIP_LENGTH (the reference leaves CityscapesSequence at its default 3).
"""
import argparse
import os
import pprint
import shutil
import sys
import timeit

import torch

import _init_paths  # noqa: F401
import datasets  # noqa: F401  (lib/datasets: the drop-in CityscapesSequence)
import models  # noqa: F401
from config import config, update_config
from core.criterion import KLLoss, L1Loss, lsgan_adversarial_loss
from core.function import adversarial_train
from utils.utils import FullModel_D, FullModel_encdec, create_logger

from vae2 import clips
from vae2 import dist as vdist
from vae2.optim import FusedAdam, FusedSGD
from vae2.trainer import NullWriter, SyntheticClips


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Train VAE2 (MI355X)")
    parser.add_argument("--cfg", help="experiment configure file name", required=True, type=str)
    parser.add_argument("--local_rank", "--local-rank", type=int,
                        default=int(os.environ.get("LOCAL_RANK", "0")))
    parser.add_argument("opts", help="Modify config options using the command-line", default=None,
                        nargs=argparse.REMAINDER)
    args = parser.parse_args(argv)
    update_config(config, args)
    return args


def build_loader(cfg, list_path, shuffle, device, logger=None, random_pos=True):
    """(loader, number of clips) for one list file (train.py:113-140).

    MI355X.SYNTHETIC_DATA: Gaussian clips.  Otherwise the Cityscapes sequence zips
    (DATASET.ROOT + a list file, gen_cityscapes_data.py layout): with MI355X.CLIP_CACHE
    decoded once into a uint8 cache (rank 0 builds it, the others wait) and served by
    ClipLoader (pinned staging + HIP normalisation); without it the drop-in
    CityscapesSequence through a torch DataLoader (PIL decode per item, uint8 windows
    normalised on the GPU by adversarial_train)."""
    w, h = cfg.TRAIN.IMAGE_SIZE
    B = cfg.TRAIN.BATCH_SIZE_PER_GPU
    if cfg.MI355X.SYNTHETIC_DATA:
        dataset = SyntheticClips(cfg.MI355X.SYNTHETIC_CLIPS, cfg.TRAIN.CLIP_LENGTH, h, w)
    elif cfg.DATASET.DATASET != "cityscapessequence":
        raise ValueError("VAE2 trains on DATASET.DATASET cityscapessequence (got {})"
                         .format(cfg.DATASET.DATASET))
    elif cfg.MI355X.CLIP_CACHE:
        cdir = cfg.MI355X.CLIP_CACHE_DIR or clips.cache_dir_for(cfg.DATASET.ROOT, list_path,
                                                                (h, w))
        if vdist.rank() == 0:
            clips.build_cache(cfg.DATASET.ROOT, list_path, (h, w), cache_dir=cdir,
                              log=logger.info if logger else None)
        if vdist.is_dist():
            torch.distributed.barrier()
        cache = clips.ClipCache(cdir)
        sampler = (torch.utils.data.distributed.DistributedSampler(range(len(cache)))
                   if vdist.is_dist() else None)
        loader = clips.ClipLoader(cache, B, clip_length=cfg.TRAIN.CLIP_LENGTH, clip_num=3,
                                  sampler=sampler, shuffle=shuffle and sampler is None,
                                  random_pos=random_pos, device=device)
        return loader, sampler, len(cache)
    else:
        dataset = datasets.cityscapessequence(
            root=cfg.DATASET.ROOT, list_path=list_path, num_samples=None,
            num_classes=cfg.DATASET.NUM_CLASSES, multi_scale=cfg.TRAIN.MULTI_SCALE,
            flip=cfg.TRAIN.FLIP, ignore_label=cfg.TRAIN.IGNORE_LABEL,
            base_size=cfg.TRAIN.BASE_SIZE, crop_size=(h, w),
            downsample_rate=cfg.TRAIN.DOWNSAMPLERATE, scale_factor=cfg.TRAIN.SCALE_FACTOR,
            clip_length=cfg.TRAIN.CLIP_LENGTH, random_pos=random_pos,
            fixed_length=cfg.DATASET.FIXED_LENGTH)
    sampler = torch.utils.data.distributed.DistributedSampler(dataset) if vdist.is_dist() else None
    loader = torch.utils.data.DataLoader(
        dataset, batch_size=B, shuffle=shuffle and sampler is None, num_workers=cfg.WORKERS,
        pin_memory=True, drop_last=True, sampler=sampler)
    return loader, sampler, len(dataset)


def main(argv=None):
    args = parse_args(argv)
    logger, final_output_dir, tb_log_dir = create_logger(config, args.cfg, "train")
    logger.info(pprint.pformat(args))
    logger.info(config)
    writer_dict = {"writer": NullWriter(), "train_global_steps": 0, "valid_global_steps": 0}
    try:
        from tensorboardX import SummaryWriter
        writer_dict["writer"] = SummaryWriter(tb_log_dir)
    except ImportError:
        logger.info("tensorboardX not installed: scalars are logged to the text log only")

    gpus = list(config.GPUS)
    distributed = len(gpus) > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1
    if config.TRAIN.OPTIMIZER not in ("sgd", "adam"):
        raise ValueError("Only Support SGD and ADAM optimizer")
    if not config.MI355X.CLIP_GRAD_NORM >= 0:
        raise ValueError("MI355X.CLIP_GRAD_NORM must be >= 0 (0 = off), got {}".format(
            config.MI355X.CLIP_GRAD_NORM))
    if not 0 <= config.MI355X.EMA_DECAY < 1:
        raise ValueError("MI355X.EMA_DECAY must be in [0, 1) (0 = off), got {}".format(
            config.MI355X.EMA_DECAY))
    if not config.MI355X.SSIM_LAMBDA >= 0:
        raise ValueError("MI355X.SSIM_LAMBDA must be >= 0 (0 = off), got {}".format(
            config.MI355X.SSIM_LAMBDA))
    extra = config.MODEL.EXTRA

    # models, in the reference's construction order (train.py:79-82)
    encdec_model = models.enc_hrnet.get_encdec_model(config)
    encz_model = (models.enc_hrnet.get_encz_model(config)
                  if extra.BASELINE_MODE != "DETERMINISTIC" else None)
    use_d = not config.MI355X.ELBO_ONLY
    D_model_sequence = models.enc_hrnet.get_D_sequence_model(config) if use_d else None
    D_model_frame = models.enc_hrnet.get_D_frame_model(config) if use_d else None

    if args.local_rank == 0:
        this_dir = os.path.dirname(os.path.abspath(__file__))
        dst = os.path.join(final_output_dir, "models")
        if os.path.exists(dst):
            shutil.rmtree(dst)
        shutil.copytree(os.path.join(this_dir, "..", "lib", "models"), dst)

    if distributed:
        vdist.init("nccl")
        vdist.set_sync_bn(config.MI355X.SYNC_BN)
        if config.MI355X.SYNC_BN and config.MI355X.SYNC_BN_EXCHANGE == "ipc":
            vdist.init_syncbn_ipc()
    device = torch.device("cuda:{}".format(args.local_rank))
    torch.cuda.set_device(device)

    loader, sampler, n_clips = build_loader(config, config.DATASET.TRAIN_SET,
                                            config.TRAIN.SHUFFLE, device, logger)
    extra_loader, extra_sampler = loader, sampler
    if config.DATASET.EXTRA_TRAIN_SET:  # train.py:142-167
        extra_loader, extra_sampler, _ = build_loader(config, config.DATASET.EXTRA_TRAIN_SET,
                                                      config.TRAIN.SHUFFLE, device, logger)

    model_encdec = FullModel_encdec(
        encz_model=encz_model, encdec_model=encdec_model, D_model_sequence=D_model_sequence,
        D_model_frame=D_model_frame, criterion_recon=L1Loss(), criterion_KL=KLLoss(),
        criterion_gan=lsgan_adversarial_loss(), x1recon_lambda=config.TRAIN.X1RECON_LAMBDA,
        x2recon_lambda=config.TRAIN.X2RECON_LAMBDA, x3recon_lambda=config.TRAIN.X3RECON_LAMBDA,
        gan_lambda=config.TRAIN.GAN_LAMBDA, ssim_lambda=float(config.MI355X.SSIM_LAMBDA))
    model_encdec.defer_checks = config.MI355X.DEFER_CHECKS
    model_encdec = model_encdec.to(device)
    model_D = None
    if use_d:
        model_D = FullModel_D(D_model_sequence=D_model_sequence, D_model_frame=D_model_frame,
                              criterion_gan=lsgan_adversarial_loss()).to(device)
        assert model_encdec.D_model_sequence is model_D.D_model_sequence, "Unexpected behavior."
        assert model_encdec.D_model_frame is model_D.D_model_frame, "Unexpected behavior."
    # SGD or Adam over encz + ED ('D_model' excluded) and over the discriminators
    # (train.py:232-261)
    nets = [m for m in (encz_model, encdec_model) if m is not None]
    # each parameter set is clipped to the threshold on its own, as two clip_grad_norm_ calls
    clip = float(config.MI355X.CLIP_GRAD_NORM) or None
    # the weight average is the generator's alone
    ema_decay = float(config.MI355X.EMA_DECAY) or None
    if config.TRAIN.OPTIMIZER == "sgd":
        def make_opt(mods, ema_decay=None):
            return FusedSGD(mods, lr=config.TRAIN.LR, momentum=config.TRAIN.MOMENTUM,
                            weight_decay=config.TRAIN.WD, nesterov=config.TRAIN.NESTEROV,
                            max_grad_norm=clip, ema_decay=ema_decay)
    else:
        def make_opt(mods, ema_decay=None):
            return FusedAdam(mods, lr=config.TRAIN.LR, max_grad_norm=clip, ema_decay=ema_decay)
    optimizer = make_opt(nets, ema_decay)
    optimizer_D = make_opt([D_model_sequence, D_model_frame]) if use_d else None
    if vdist.is_dist():  # replicas start identical (DDP's initial broadcast)
        for opt in (optimizer, optimizer_D):
            for f in (opt.flats if opt is not None else []):
                torch.distributed.broadcast(f.data, src=0)

    epoch_iters = int(n_clips / config.TRAIN.BATCH_SIZE_PER_GPU / max(1, len(gpus)))
    last_epoch = 0
    state_file = os.path.join(final_output_dir, "checkpoint_encdec.pth.tar")
    state_file_D = os.path.join(final_output_dir, "checkpoint_D.pth.tar")
    if config.TRAIN.RESUME:  # train.py:270-290
        if os.path.isfile(state_file):
            ck = torch.load(state_file, map_location="cpu", weights_only=True)
            last_epoch = ck["epoch"]
            if ema_decay is not None and ck.get("ema_updates", 0) > 0 and "ema_state_dict" in ck:
                # seed the average from the live parameters so that swap_ema() is legal, then
                # load the saved average into the parameters' place inside it
                with torch.no_grad():
                    for f, e in zip(optimizer.flats, optimizer.ema):
                        e.copy_(f.data)
                    optimizer.ema_updates = int(ck["ema_updates"])
                with optimizer.swap_ema():
                    model_encdec.load_state_dict(ck["ema_state_dict"], strict=use_d)
            elif ema_decay is not None:
                logger.info("=> the checkpoint holds no EMA weights: the average starts from "
                            "the first update of this run")
            model_encdec.load_state_dict(ck["state_dict"], strict=use_d)
            optimizer.load_state_dict(ck["optimizer_encdec"])
            logger.info("=> loaded checkpoint (epoch {})".format(ck["epoch"]))
        if use_d and os.path.isfile(state_file_D):
            ck = torch.load(state_file_D, map_location="cpu", weights_only=True)
            last_epoch = ck["epoch"]
            model_D.load_state_dict(ck["state_dict"])
            optimizer_D.load_state_dict(ck["optimizer_D"])
            logger.info("=> loaded checkpoint (epoch {})".format(ck["epoch"]))

    start = timeit.default_timer()
    end_epoch = config.TRAIN.END_EPOCH + config.TRAIN.EXTRA_EPOCH
    num_iters = config.TRAIN.END_EPOCH * epoch_iters
    extra_iters = config.TRAIN.EXTRA_EPOCH * epoch_iters
    for epoch in range(last_epoch, end_epoch):
        if sampler is not None:
            sampler.set_epoch(epoch)
        if extra_sampler is not None and extra_sampler is not sampler:
            extra_sampler.set_epoch(epoch)
        if epoch >= config.TRAIN.END_EPOCH:  # train.py:300-306
            # EXTRA_LR reaches adversarial_train as base_lr, which only logs it: the
            # reference's adjust_learning_rate call is commented out (function.py:525-528),
            # so the optimizers keep training at TRAIN.LR in the extra epochs too
            ep_args = (epoch - config.TRAIN.END_EPOCH, config.TRAIN.EXTRA_EPOCH, epoch_iters,
                       config.TRAIN.EXTRA_LR, extra_iters, extra_loader)
        else:
            ep_args = (epoch, config.TRAIN.END_EPOCH, epoch_iters, config.TRAIN.LR, num_iters,
                       loader)
        adversarial_train(config, *ep_args, optimizer, optimizer_D, model_encdec, model_D,
                          writer_dict, device, final_output_dir,
                          use_multiplier=config.TRAIN.USE_X2RECON_MULTIPLIER,
                          is_baseline=extra.IS_BASELINE, baseline_mode=extra.BASELINE_MODE)
        if vdist.rank() == 0:  # train.py:317-348
            logger.info("=> saving checkpoint to {}".format(state_file))
            ck = {"epoch": epoch + 1, "state_dict": model_encdec.state_dict(),
                  "optimizer_encdec": optimizer.state_dict()}
            if ema_decay is not None:
                with optimizer.swap_ema():
                    ck["ema_state_dict"] = {k: v.clone()
                                            for k, v in model_encdec.state_dict().items()}
                ck["ema_updates"] = optimizer.ema_updates
            torch.save(ck, state_file)
            if use_d:
                logger.info("=> saving checkpoint to {}".format(state_file_D))
                torch.save({"epoch": epoch + 1, "state_dict": model_D.state_dict(),
                            "optimizer_D": optimizer_D.state_dict()}, state_file_D)
            if epoch == end_epoch - 1:
                torch.save(model_encdec.state_dict(),
                           os.path.join(final_output_dir, "model_encdec_final_state.pth"))
                if ema_decay is not None:
                    torch.save(ck["ema_state_dict"],
                               os.path.join(final_output_dir,
                                            "model_encdec_final_state_ema.pth"))
                if use_d:
                    torch.save(model_D.state_dict(),
                               os.path.join(final_output_dir, "model_D_final_state.pth"))
                writer_dict["writer"].close()
                logger.info("Hours: %d" % int((timeit.default_timer() - start) / 3600))
                logger.info("Done")
        if vdist.is_dist():
            # the other ranks wait here for rank 0's checkpoint writes: otherwise they would
            # start the next epoch and wait in its first SyncBN exchange, whose bounded wait
            # can expire during a slow save
            torch.distributed.barrier()


if __name__ == "__main__":
    sys.exit(main())
