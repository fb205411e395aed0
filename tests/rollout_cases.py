"""Seeded requests of the rollout tests and a restatement of the chain's links on oracle/mvae_oracle.py in ``eval_mode``, shared by
tests/test_rollout_emu.py and tests/test_rollout_gpu.py.  The reference has no rollout, so nothing here comes from a golden file:
a step is the oracle's ``mvae_forward`` of each row on the modalities that row holds, the next state is the sigmoid of its image
logits and its pose output (or the observed frame), and the terms of a step are BCE-with-logits / squared error / the analytic KL
in fp64 against that step's target."""
import torch
import torch.nn.functional as F

from mmdyn_hip.utils.seeded_init import seeded_batch
from oracle import mvae_oracle as O

import cond_cases as CC

L = CC.LATENT
BATCH, STEPS = 3, 3
START = [(1, 1, 1), (1, 0, 0), (0, 1, 1)]          # what row b holds of (visual, tactile, pose) at step 0
KL_WEIGHT, POSE_MULTIPLIER = 0.3, 1000.0


def start(seed=801):
    """(inputs [visual, tactile, pose] of BATCH rows, available [BATCH, 3] float64)."""
    inputs, _ = seeded_batch(BATCH, seed, with_pose=True)
    return inputs, torch.tensor(START, dtype=torch.float64)


def frames(seed, T=STEPS, B=BATCH):
    """[visual [T, B, 3, 64, 64], tactile, pose [T, B, 7]]: recorded frames to observe or to score against."""
    a, _ = seeded_batch(T * B, seed, with_pose=True)
    return [t.reshape((T, B) + tuple(t.shape[1:])) for t in a]


def draws(seed=33, T=STEPS, B=BATCH):
    """T distinct standard-normal draws [B, L]."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, L, generator=g) for _ in range(T)]


def mixed_table(seed=5, T=STEPS, B=BATCH):
    """[T, B, 3] 0 / 1 with both values in every column."""
    tab = (torch.rand(T, B, 3, generator=torch.Generator().manual_seed(seed)) < 0.5).to(torch.float64)
    tab[0, 0], tab[0, 1] = 1.0, 0.0
    return tab


def oracle_state(model):
    return O.split_state({k: v.detach().cpu() for k, v in model.state_dict().items()}, requires_grad=False)


def oracle_step(prm, buf, state, on, eps, cond=None, use_pose=True):
    """One link: the oracle's eval-mode forward of every row on the modalities the row holds (``on``: bool [B][3]; None: all).
    state = [visual, tactile, pose] CPU tensors -> (visual logits, tactile logits, pose output | None, means, log_var)."""
    B = eps.shape[0]
    outs = []
    with O.eval_mode(), torch.no_grad():
        for b in range(B):
            row = [state[m][b:b + 1] if state[m] is not None and (on is None or bool(on[b, m])) else None for m in range(3)]
            if all(r is None for r in row):
                raise ValueError("the restatement needs a modality in every row")
            c = None if cond is None else cond[b:b + 1]
            outs.append(O.mvae_forward(prm, row[0], row[1], row[2], eps[b:b + 1], iter([None, None]), use_pose, buf, c))
    return tuple(None if outs[0][k] is None else torch.cat([o[k] for o in outs]) for k in range(5))


def step_terms(v, t, pr, mu, lv, targets, ton, pose_multiplier, kl_weight):
    """fp64 terms of one step from its logits / pose output / posterior against targets = [visual | None, tactile | None,
    pose | None] ([B, ...]); ton: bool [B][3] or None.  An absent (row, term) is 0 and left out of rows."""
    B = mu.shape[0]
    zero = torch.zeros(B, dtype=torch.float64)
    keep = lambda x, m: x if ton is None else torch.where(ton[:, m], x, zero)
    out = {"bce_visual": None, "bce_tactile": None, "mse_pose": None}
    rows = zero.clone()
    for m, (name, lg) in enumerate((("bce_visual", v), ("bce_tactile", t))):
        if targets[m] is not None:
            out[name] = keep(F.binary_cross_entropy_with_logits(lg.double(), targets[m].double(), reduction="none").sum((1, 2, 3)), m)
            rows = rows + out[name]
    if targets[2] is not None:
        out["mse_pose"] = keep(((pr.double() - targets[2].double()) ** 2).sum(1), 2)
        rows = rows + pose_multiplier * out["mse_pose"]
    out["kl"] = -0.5 * (1 + lv.double() - mu.double() ** 2 - lv.double().exp()).sum(1)
    out["rows"] = rows + kl_weight * out["kl"]
    return out


def next_state(v, t, pr, observed, oon):
    """s_{t+1} from the step's outputs: observed[m] ([B, ...] or None) where oon[b][m] (bool [B][3]; None: wherever given)."""
    pred = [torch.sigmoid(v), torch.sigmoid(t), pr]
    out = []
    for m in range(3):
        if pred[m] is None or observed is None or observed[m] is None:
            out.append(pred[m])
            continue
        row = torch.ones(pred[m].shape[0], dtype=torch.bool) if oon is None else oon[:, m]
        out.append(torch.where(row.reshape((-1,) + (1,) * (pred[m].dim() - 1)), observed[m], pred[m]))
    return out
