"""The seeded case behind tests/golden/eval_grad.npz, shared by its generator (tests/golden/make_golden_eval_grad.py) and by the
tests that compare against it: a pure function of the constants below."""
import torch

from mmdyn_hip.utils.seeded_init import seeded_batch

B, LATENT = 3, 256
KL_WEIGHT, POSE_MULTIPLIER = 0.02, 1000.0
FULL = 4096            # a gradient tensor of at most this many elements is stored whole, a larger one as summarize(t, 256)


def case():
    """(inputs [visual, tactile, pose], targets, eps [B, L], z [B, L], r [B, 3, 64, 64])."""
    inputs, targets = seeded_batch(B, 2468, with_pose=True)
    g = torch.Generator().manual_seed(1357)
    eps = torch.randn(B, LATENT, generator=g)
    z = torch.randn(B, LATENT, generator=g)
    r = torch.rand(B, 3, 64, 64, generator=g) - 0.5
    return inputs, targets, eps, z, r
