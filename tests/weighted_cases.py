"""Seeded weights and gradient samples of the weighted-ELBO cases: shared by tests/golden/make_golden_weighted.py (which runs the
reference on the cases of tests/rows_cases.py and stores the RESULTS in tests/golden/weighted_elbo.npz) and by the tests."""
import zlib

import torch

MVAE_NAMES = ("pose", "nopose", "nopose_mask1")       # the seeded cnn-mvae cases of rows_cases.MVAE_CASES that are used here
VAE_NAME = "vae"
N_SAMPLES = 48              # gradient elements kept per parameter tensor (plus the tensor's L2 norm)


def weights(B, seed=99):
    """Per-sample weights of mixed magnitudes (1e-2 .. 1e1) with one exact zero and one negative entry (B >= 2); fp32 [B]."""
    g = torch.Generator().manual_seed(seed + B)
    w = torch.pow(10.0, torch.rand(B, generator=g) * 3 - 2).to(torch.float32)
    w[0] = 0.0
    if B > 1:
        w[1] = -w[1]
    return w


def sample_index(name, numel):
    """The seeded subset of a parameter gradient's elements that the fixture keeps: int64 [min(N_SAMPLES, numel)]."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return torch.randperm(numel, generator=g)[:N_SAMPLES].sort().values
