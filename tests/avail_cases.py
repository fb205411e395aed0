"""Seeded inputs of the mixed-modality cases: shared by tests/golden/make_golden_mixed.py (which runs the reference on them, the
WHOLE batch once per modality subset, and stores row b of the run of row b's subset in tests/golden/mixed_modal.npz) and by the
tests (which regenerate the same inputs from the same seeds)."""
import torch

from mmdyn_hip.utils.seeded_init import seeded_batch

import cond_cases as C

LATENT = C.LATENT
BATCH = 8
# the seven subsets of (visual, tactile, pose), in the order the rows take them; the joint one occurs twice
SUBSETS = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
ROW_SUBSET = [4, 1, 6, 0, 3, 5, 2, 7]          # row b holds SUBSETS[ROW_SUBSET[b]]
KL_WEIGHT, POSE_MULTIPLIER = C.KL_WEIGHT, C.POSE_MULTIPLIER

PLAIN_KW = dict(input_dim=4096, architecture="cnn", conditional=False, categorical_conditions=False, condition_dim=0,
                latent_size=LATENT, use_pose=True)


def model_kw(categorical):
    """The unconditional cnn-mvae + pose, or the categorical-condition model of tests/cond_cases.py."""
    return C.model_kw(True, True) if categorical else dict(PLAIN_KW)


def row_subsets():
    return [SUBSETS[i] for i in ROW_SUBSET]


def available(columns=3, dtype=torch.float64):
    """[BATCH, columns] availability of the case: what the dataset yields (float64 0. / 1.) for columns = 2."""
    return torch.tensor(row_subsets(), dtype=dtype)[:, :columns].contiguous()


def case(categorical):
    """(inputs [visual, tactile, pose], eps [BATCH, LATENT], condition | None)."""
    inputs, _ = seeded_batch(BATCH, 9091, with_pose=True)
    eps = torch.randn(BATCH, LATENT, generator=torch.Generator().manual_seed(17))
    return inputs, eps, (C.indices(BATCH, 26) if categorical else None)
