"""Seeded inputs of the per-sample ELBO cases: shared by tests/golden/make_golden_rows.py (which runs the reference on them and
stores the RESULTS in tests/golden/elbo_rows.npz) and by the tests (which regenerate the same inputs from the same seeds)."""
import torch

from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise

KL_WEIGHT = 0.02
POSE_MULTIPLIER = 1000.0

# name -> (use_pose, batch, loss-mask channels or 0, conditional)
MVAE_CASES = {
    "pose": (True, 4, 0, False),
    "nopose": (False, 4, 0, False),
    "nopose_mask1": (False, 4, 1, False),
    "nopose_mask3": (False, 4, 3, False),
    "conditional": (True, 2, 0, True),
}
VAE_CASES = {"vae": 0, "vae_mask1": 1}       # name -> loss-mask channels or 0 (cnn-vae, visual, B = 16)
VAE_BATCH = 16
EVAL_BATCH = 3


def loss_mask(batch, channels, seed=2024, size=64):
    """A binary loss mask [B][channels][H][W] (about 70 % ones), a pure function of its arguments."""
    g = torch.Generator().manual_seed(seed + channels)
    return (torch.rand(batch, channels, size, size, generator=g) < 0.7).to(torch.float32)


def mvae_case(name):
    """(inputs, targets, eps, masks, loss_mask or None, condition or None) of one cnn-mvae case."""
    use_pose, B, mask_c, conditional = MVAE_CASES[name]
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    if conditional:       # the inputs of tests/golden/mvae_conditional_B2.npz
        inputs, targets = seeded_batch(B, 321, with_pose=True)
        eps, masks = seeded_noise(B, 256, n_pass, n_mask, 77)
        cond = torch.rand(B, 3, generator=torch.Generator().manual_seed(9))
    else:
        inputs, targets = seeded_batch(B, 1234, with_pose=use_pose)
        eps, masks = seeded_noise(B, 256, n_pass, n_mask, 4321)
        cond = None
    return inputs, targets, eps, masks, (loss_mask(B, mask_c) if mask_c else None), cond


def vae_case(name):
    """(x, y, eps, masks, loss_mask or None) of one cnn-vae case."""
    g = torch.Generator().manual_seed(555)
    x = torch.rand(VAE_BATCH, 3, 64, 64, generator=g)
    y = torch.rand(VAE_BATCH, 3, 64, 64, generator=g)
    eps, masks = seeded_noise(VAE_BATCH, 256, 1, 1, 31)
    mc = VAE_CASES[name]
    return x, y, eps, masks, (loss_mask(VAE_BATCH, mc) if mc else None)


def eval_case():
    """(inputs, targets, eps) of the eval-mode serving case: one joint (visual, tactile, pose) pass."""
    inputs, targets = seeded_batch(EVAL_BATCH, 4242, with_pose=True)
    eps = torch.randn(EVAL_BATCH, 256, generator=torch.Generator().manual_seed(11))
    return inputs, targets, eps
