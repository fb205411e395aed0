"""Seeded cases and the yardstick of the fused training step on mixed-modality batches (``MVAEStep(available=, target_available=)``).

Cases: seeded inputs (``seeded_batch`` / ``seeded_noise``), 64 x 64 images (the smallest size the model has) and fixed tables:
  ``pose``    B = 5, with pose, [B, 3] tables;
  ``nopose``  B = 3, without pose, [B, 2] tables and a 1-channel ``loss_mask``.
Between them the input patterns hold the full set, each single modality, a pair and a row holding nothing; in each case the target
table differs from the input table, every modality is present in at least one row and absent in at least one, and at least one
(row, modality) is input-absent but target-present.

Yardstick: a torch-autograd restatement of the semantics, composed from ``oracle.mvae_oracle``'s layers -- every row through every
encoder and decoder (train-mode BatchNorm over the whole batch), ``product_of_experts`` on each ROW's own expert set, ``torch.where``
on the targets -- in the pattern of ``oracle_terms`` in tests/test_weighted_emu.py.  The reference cannot produce this number itself:
its MVAE.forward takes one modality subset per call, and running it per subset on sub-batches changes the batch statistics of every
BatchNorm layer, which couple the rows of a batch; the semantics here keep all B rows in the statistics."""
import torch
import torch.nn.functional as F

import rows_cases as C
from mmdyn_hip.models.shapes import state_dict_shapes
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise, seeded_state_dict
from oracle import mvae_oracle as O

KL_WEIGHT = 0.3
POSE_MULTIPLIER = C.POSE_MULTIPLIER

# name -> (use_pose, B, loss-mask channels, input table, target table)
CASES = {
    "pose": (True, 5, 0,
             [[1, 1, 1], [1, 0, 0], [0, 1, 1], [0, 0, 1], [0, 0, 0]],      # full, visual, tactile + pose, pose, nothing
             [[1, 0, 1], [1, 1, 0], [0, 1, 1], [1, 1, 1], [0, 1, 0]]),     # (row 1: tactile input-absent, target-present)
    "nopose": (False, 3, 1,
               [[1, 1], [0, 1], [0, 0]],                                   # both, tactile, nothing
               [[0, 1], [1, 1], [1, 0]]),                                  # (row 1: visual input-absent, target-present)
}


def weights(B, seed=11):
    """Positive per-sample weights in [0.25, 2.25), a pure function of its arguments."""
    return 0.25 + 2.0 * torch.rand(B, generator=torch.Generator().manual_seed(seed))


def case(name):
    """(use_pose, B, inputs, targets, eps, masks, loss_mask or None, available, target_available) of one case."""
    use_pose, B, mask_c, tin, ttg = CASES[name]
    inputs, targets = seeded_batch(B, 1234, with_pose=use_pose)
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass, n_mask, 4321)
    mask = C.loss_mask(B, mask_c) if mask_c else None
    return use_pose, B, inputs, targets, eps, masks, mask, torch.tensor(tin, dtype=torch.float32), torch.tensor(ttg, dtype=torch.float32)


def full_table(table, B):
    """bool [B][3]: a [B, 2] table counts the pose as present."""
    on = torch.ones(B, 3, dtype=torch.bool)
    on[:, :table.shape[1]] = table != 0
    return on


def row_poe(heads, on):
    """Row b's posterior: the prior times the experts the pass holds AND the row holds (vae.py:139-159 on the row's own subset).
    heads: [(mu, lv) or None] * 3, on: bool [B][3]."""
    ref = next(h for h in heads if h is not None)[0]
    B, L = ref.shape
    mus, lvs = [], []
    for b in range(B):
        m, l = [torch.zeros(1, L)], [torch.zeros(1, L)]                      # the prior expert
        for k, h in enumerate(heads):
            if h is not None and bool(on[b, k]):
                m.append(h[0][b:b + 1]), l.append(h[1][b:b + 1])
        mu, lv = O.product_of_experts(torch.stack(m), torch.stack(l))
        mus.append(mu), lvs.append(lv)
    return torch.cat(mus), torch.cat(lvs)


_YARD = {}


def yardstick_terms(name):
    """(prm, terms [3][P][B], kl [P][B]) with the autograd graph behind them: terms[m][p][b] = the reconstruction term of modality m
    (visual BCE, tactile BCE, pose_multiplier * MSE) of pass p and row b where the pass holds m and the row holds that TARGET, else 0
    (``torch.where``); kl = each pass's per-sample KL.  Computed once per case and shared by the tests that differ in the KL mode or
    the weights only; nothing modifies it."""
    if name in _YARD:
        return _YARD[name]
    use_pose, B, inputs, targets, eps, masks, mask, tin, ttg = case(name)
    on_in, on_tg = full_table(tin, B), full_table(ttg, B)
    prm, buf = O.split_state(seeded_state_dict(state_dict_shapes("cnn-mvae", use_pose=use_pose), 0))
    eps_it, mask_it = iter(eps), iter(masks)
    zero = torch.zeros(B)
    terms, kls = [[], [], []], []
    for a, b, c in (O.SUBSETS_POSE if use_pose else O.SUBSETS_NOPOSE):
        heads = [None, None, None]
        if a:
            heads[0] = O.image_encoder(inputs[0], prm, "visual_encoder", next(mask_it), buf)
        if b:
            heads[1] = O.image_encoder(inputs[1], prm, "tactile_encoder", next(mask_it), buf)
        if c:
            heads[2] = O.pose_encoder(inputs[2], prm)
        mu, lv = row_poe(heads, on_in)
        z = O.reparametrize(mu, lv, next(eps_it))
        for k, (on, dec) in enumerate(((a, "visual_decoder"), (b, "tactile_decoder"))):
            if on:
                r, x = O.image_decoder(z, prm, dec, buf), targets[k]
                if mask is not None:
                    r, x = r * mask, x * mask
                rows = F.binary_cross_entropy_with_logits(r, x, reduction="none").sum((1, 2, 3))
                terms[k].append(torch.where(on_tg[:, k], rows, zero))
            else:
                terms[k].append(zero)
        if c:
            rows = POSE_MULTIPLIER * F.mse_loss(O.pose_decoder(z, prm), targets[2], reduction="none").sum(1)
            terms[2].append(torch.where(on_tg[:, 2], rows, zero))
        else:
            terms[2].append(zero)
        kls.append(-0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(1))
    out = (prm, torch.stack([torch.stack(t) for t in terms]), torch.stack(kls))
    _YARD[name] = out
    return out


def yardstick(name, kl, w=None, kl_weight=KL_WEIGHT):
    """(prm, loss, partials [P], rows [B]): L = (1/B) sum_p sum_b w_b [sum_m terms[m][p][b] + kl_weight KL(p, b)] with KL(p, b) the
    sample's own (``kl="sample"``) or the batch total (``"batch"``); partials its per-pass parts; rows the unweighted per-sample
    sums over the passes."""
    prm, terms, kls = yardstick_terms(name)
    B = kls.shape[1]
    w = torch.ones(B) if w is None else w
    klb = kls if kl == "sample" else kls.sum(1, keepdim=True).expand_as(kls)
    per = terms.sum(0) + kl_weight * klb                                       # [P][B]
    partials = (per * w[None, :]).sum(1) / B
    return prm, partials.sum(), partials, per.sum(0)
