"""Seeded inputs of the condition cases: shared by tests/golden/make_golden_conditions.py (which runs the reference on them and
stores the RESULTS in tests/golden/conditions.npz) and by the tests (which regenerate the same inputs from the same seeds)."""
import torch

from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise

KL_WEIGHT = 0.02
POSE_MULTIPLIER = 1000.0
LATENT = 64
LR = 1e-3
CAT_DIM, REAL_DIM = 5, 3
TRAIN_BATCH, EVAL_BATCH, SAMPLE_N, VAE_BATCH = 4, 3, 3, 4
# eval-mode subsets (visual, tactile, pose): joint, visual-only, pose-only
SUBSETS = {"joint": (1, 1, 1), "visual": (1, 0, 0), "pose": (0, 0, 1)}
# the six weight matrices whose last condition_dim columns multiply the condition
COND_WEIGHTS = ["visual_encoder.linear_means.weight", "visual_encoder.linear_log_var.weight",
                "tactile_encoder.linear_means.weight", "tactile_encoder.linear_log_var.weight",
                "visual_decoder.upsample.0.weight", "tactile_decoder.upsample.0.weight"]

MODEL_KW = dict(input_dim=4096, architecture="cnn", conditional=True, latent_size=LATENT)


def model_kw(categorical, use_pose=None):
    kw = dict(MODEL_KW, categorical_conditions=categorical, condition_dim=CAT_DIM if categorical else REAL_DIM)
    if use_pose is not None:
        kw["use_pose"] = use_pose
    return kw


def indices(n, seed, dim=CAT_DIM):
    """n class indices in [0, dim), every class of a small batch distinct where n <= dim."""
    return torch.randperm(dim, generator=torch.Generator().manual_seed(seed))[:n] if n <= dim else \
        torch.randint(0, dim, (n,), generator=torch.Generator().manual_seed(seed))


def train_case():
    """(a) / (e): categorical cnn-mvae + pose, one train step: (inputs, targets, eps [7], masks [8], class indices [B])."""
    inputs, targets = seeded_batch(TRAIN_BATCH, 2468, with_pose=True)
    eps, masks = seeded_noise(TRAIN_BATCH, LATENT, 7, 8, 1357)
    return inputs, targets, eps, masks, indices(TRAIN_BATCH, 21)


def eval_case(categorical):
    """(b) / (c): eval-mode forward of the three SUBSETS + inference: (inputs, eps per subset, condition, z, sample condition)."""
    inputs, _ = seeded_batch(EVAL_BATCH, 4242, with_pose=True)
    g = torch.Generator().manual_seed(11)
    eps = {k: torch.randn(EVAL_BATCH, LATENT, generator=g) for k in SUBSETS}
    z = torch.randn(SAMPLE_N, LATENT, generator=g)
    if categorical:
        cond, cs = indices(EVAL_BATCH, 22), indices(SAMPLE_N, 23).unsqueeze(1)
    else:
        cond, cs = torch.rand(EVAL_BATCH, REAL_DIM, generator=g), torch.rand(SAMPLE_N, REAL_DIM, generator=g)
    return inputs, eps, cond, z, cs


def vae_case():
    """(d): categorical cnn-vae, one train step + inference: (x, labels, eps [1], masks [1], z, sample condition)."""
    g = torch.Generator().manual_seed(555)
    x = torch.rand(VAE_BATCH, 3, 64, 64, generator=g)
    eps, masks = seeded_noise(VAE_BATCH, LATENT, 1, 1, 31)
    z = torch.randn(SAMPLE_N, LATENT, generator=g)
    return x, indices(VAE_BATCH, 24), eps, masks, z, indices(SAMPLE_N, 25).unsqueeze(1)
