"""CLI with the reference's flags and defaults (/root/reference/mmdyn/pytorch/main.py:13-54).

With ``--dataset-path`` pointing at a dataset (the PNG/json tree or its compiled pickle) it trains on it like the
reference, decoding the frames on the GPU (utils/datasets.py).  ``--synthetic-batches N`` (this build only)
replaces the dataset by N random batches per epoch -- the BASELINE workload:

    python -m mmdyn_hip.main --problem-type seq_modeling --input-type visuotactile --model-name cnn-mvae \
        --use-pose --batchsize 256 --num-epochs 2 --synthetic-batches 20
"""
import argparse
import os
import pickle

from . import config
from .problems.problems import Reconstruction, Regression, SeqModeling, DynModeling, SyntheticVisuoTactile


# The reference's flags (same names and defaults: main.py:13-54 there) as data.  (flag, default, type or None for a switch,
# what it selects here).  Defaults are API: a reference command line must mean the same thing with this build.
_REFERENCE_FLAGS = (
    ("problem-type", "seq_modeling", str, "which problem class runs: " + " | ".join(config.PROBLEM_TYPES)),
    ("model-name", "cnn-mvae", str, "registry name of the model: " + " | ".join(config.MODELS)),
    ("input-type", "visual", str, "modality fed to the model: visual | tactile | visuotactile"),
    ("use-pose", False, None, "cnn-mvae only: the 7-DoF pose as a third modality"),
    ("lr", 0.001, float, "learning rate of the fused Adam / SGD step"),
    ("dataset-path", "~/dataset", str, "PNG + json tree or its compiled pickle (frames are decoded on the GPU)"),
    ("batchsize", 128, int, "samples per step"),
    ("criterion", "crossentropy", str, "accepted for compatibility; the VAE problems use the ELBO"),
    ("optimizer", "Adam", str, " | ".join(config.OPTIMIZERS)),
    ("num-epochs", 100, int, "training epochs"),
    ("mask-loss", False, None, "restrict the reconstruction loss to the object segment"),
    ("vis-pose", False, None, "accepted for compatibility (no pose figures in this build; --log-images writes the image grids)"),
    ("pose-multiplier", 1000, float, "weight of the pose MSE inside the ELBO"),
    ("save-name", "run", str, "name of the log directory"),
    ("no-cuda", False, None, "rejected with an error: this build has no CPU path"),
    ("kl-weight", 1.0, float, "KL weight before the annealing schedule overwrites it"),
    ("latent-size", 256, int, "latent dimension"),
    ("annealing-epochs", 50, int, "epochs over which the KL weight is ramped"),
    ("conditional", False, None, "condition encoders / decoders on the shock force"),
)
# switches of this build only
_BUILD_FLAGS = (
    ("synthetic-batches", 0, int, "train on this many random batches per epoch instead of --dataset-path"),
    ("synthetic-seq-length", 1, int, "frames per synthetic sequence"),
    ("reference-schedule", False, None, "run the reference's 7-forward autograd schedule instead of the fused step"),
    ("image-size", 64, int, "side of the input images: 64 (the reference's only size) or the 128 / 256 pixel extended stacks "
                            "(models/shapes.py; BASELINE configs[3] / configs[4], no reference architecture)"),
    ("precision", "fp32x3", str, "matrix-core arithmetic of the fused step: fp32x3 (default: fp32 storage and results, exact three-term operand split on the bf16 matrix cores) | fp32 (the native fp32 matrix cores) | bf16 | bf16s | fp16 | fp16s"),
    ("exact-running-stats", False, None, "fused step: also run the image decoders on the subset passes whose reconstruction the "
                                         "reference computes and discards, so that the decoders' BatchNorm running statistics "
                                         "get the reference's 7 (3) updates per step instead of 4 (2); ~1.4x the step time"),
    ("use-availability", False, None, "seq / dyn modeling with cnn-mvae: train and validate on mixed-modality batches -- the dataset's "
                                      "per-frame availability table selects each row's experts in the posterior and drops the "
                                      "reconstruction terms of absent targets (default: every frame counts as complete)"),
    ("synthetic-absent", 0.0, float, "with --synthetic-batches: share of (frame, image modality) pairs marked missing"),
    ("grad-clip", 0.0, float, "clip every step's gradient by its global L2 norm (torch.nn.utils.clip_grad_norm_ arithmetic, on the "
                              "device, inside the replayed step) and log Grad_norm/train_epoch and Grad_clipped/train_epoch; "
                              "inf logs the norm without clipping; 0 = off"),
    ("ema-decay", 0.0, float, "keep an exponential moving average of the parameters with this decay in [0, 1) (on the device, inside "
                              "the replayed step) and write it into the best-validation checkpoint as 'model_ema' with "
                              "'ema_updates'; training and validation stay on the live weights; 0 = off"),
    ("ema-warmup", False, None, "with --ema-decay: update n uses the decay min(decay, (1 + n) / (10 + n))"),
    ("log-images", 0, int, "every K-th epoch (epoch %% K == 0) and on the last one, write the reference's image log as PNG files under "
                           "<log dir>/plot/: inputs, reconstructions and targets of the epoch's last training and validation "
                           "batch and 50 decoded draws from the prior, each as one grid built on the device (one launch per "
                           "grid).  The draws come from the model's noise source on every logged epoch (the reference draws "
                           "them from torch's generator on every epoch), so the noise of later epochs differs from a run with "
                           "the flag off, and -- the model being in train mode, as in the reference -- decoding them also "
                           "moves the decoders' BatchNorm running statistics once per logged epoch; 0 = off"),
)


def build_parser():
    parser = argparse.ArgumentParser(description="cnn-VAE / cnn-MVAE training on MI355X (mmdyn_hip)")
    for name, default, kind, text in _REFERENCE_FLAGS + _BUILD_FLAGS:
        if kind is None:
            parser.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            parser.add_argument("--" + name, type=kind, default=default, help=f"{text} (default: {default})")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    assert args.problem_type in config.PROBLEM_TYPES, "Invalid problem type."
    if not args.grad_clip >= 0:                      # (a negative value, or NaN)
        parser.error(f"--grad-clip must be a norm > 0, inf, or 0 for off (got {args.grad_clip})")
    if not 0 <= args.ema_decay < 1:                  # (also NaN)
        parser.error(f"--ema-decay must be a decay in (0, 1), or 0 for off (got {args.ema_decay})")
    if args.log_images < 0:
        parser.error(f"--log-images must be a number of epochs >= 1, or 0 for off (got {args.log_images})")
    L = args.synthetic_seq_length
    shock = 3 if args.conditional else 0
    if args.synthetic_batches > 0:
        loaders = dict(train_loader=SyntheticVisuoTactile(args.synthetic_batches, args.batchsize, L, seed=1234,
                                                          shock_dim=shock, size=args.image_size, absent=args.synthetic_absent),
                       test_loader=SyntheticVisuoTactile(max(1, args.synthetic_batches // 4), args.batchsize, L,
                                                         seed=4321, shock_dim=shock, size=args.image_size, absent=args.synthetic_absent),
                       seq_length=L, fused=not args.reference_schedule)
    else:
        loaders = dict(fused=not args.reference_schedule)      # Problem.set_dataset reads --dataset-path
    problem_args = argparse.Namespace(**{k: v for k, v in vars(args).items()
                                         if not k.startswith('synthetic') and k != 'reference_schedule'})
    if args.problem_type == 'regression':
        problem = Regression(problem_args, **loaders)
    elif args.problem_type == 'reconstruction':
        problem = Reconstruction(problem_args, **loaders)
    elif args.problem_type == 'dyn_modeling':
        problem = DynModeling(problem_args, **loaders)
    else:
        problem = SeqModeling(problem_args, **loaders)
    with open(os.path.join(problem.log_dir, 'problem.pkl'), 'wb') as f:
        pickle.dump(problem_args, f)
    problem.train()
    return problem


if __name__ == "__main__":
    main()
