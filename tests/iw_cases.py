"""fp64 restatements of the importance-weighted K-sample bound, shared by tests/test_iw_bound_emu.py, tests/test_iw_bound_gpu.py and
tests/emu_backend_iw.py.  The reference has no such estimator, so nothing here comes from a golden file: the pieces are the definitions
(z_k = eps_k exp(lv / 2) + mu in fp32, ratio_k = sum 0.5 (z^2 - eps^2 - lv) in fp64 from that z, log_w_k = -rec_k - kl_weight ratio_k,
rows = -(logsumexp_k log_w_k - log K), ess = exp(2 lse(log_w) - lse(2 log_w))) and, for a whole request, the eval-mode forward
functions of oracle/mvae_oracle.py."""
import math

import torch
import torch.nn.functional as F

from oracle import mvae_oracle as O


def iw_ratio_ref(z, eps, lv):
    """(ratio [K][B], sum of the terms' magnitudes [K][B]) in fp64 from fp32 z / eps [K][B][L] and lv [B][L]."""
    z, eps, lv = z.double(), eps.double(), lv.double().unsqueeze(0)
    terms = 0.5 * (z * z - eps * eps - lv)
    return terms.sum(2), terms.abs().sum(2)


def iw_latent_ref(mu, lv, eps):
    """(z [K][B][L] fp32 by the kernel's expression, ratio [K][B] fp64 from that z) of mu / lv [B][L] and eps [K][B][L]."""
    mu, lv, eps = mu.float(), lv.float(), eps.float()
    z = eps * torch.exp(0.5 * lv).unsqueeze(0) + mu.unsqueeze(0)
    return z, iw_ratio_ref(z, eps, lv)[0]


def iw_assemble_ref(bce, mse, ratio, on, pose_multiplier, kl_weight):
    """bce: fp64 [n <= 2][K][B] or None; mse: fp64 [K][B] or None; ratio: fp64 [K][B]; on: bool [B][>= 3] target availability or None.
    -> (out fp64 [B] (before the fp32 cast), ess fp64 [B], log_w fp64 [K][B], bce and mse with the absent entries zeroed)."""
    K, B = ratio.shape
    rec = torch.zeros(K, B, dtype=torch.float64)
    if bce is not None:
        bce = bce.clone()
        for s in range(bce.shape[0]):
            if on is not None:
                bce[s] = torch.where(on[:, s].unsqueeze(0), bce[s], torch.zeros_like(bce[s]))
            rec = rec + bce[s]
    if mse is not None:
        mse = mse.clone()
        if on is not None:
            mse = torch.where(on[:, 2].unsqueeze(0), mse, torch.zeros_like(mse))
        rec = rec + pose_multiplier * mse
    log_w = -(rec + kl_weight * ratio)
    lse = torch.logsumexp(log_w, 0)
    out = -(lse - math.log(K))
    ess = torch.exp(2.0 * lse - torch.logsumexp(2.0 * log_w, 0))
    return out, ess, log_w, bce, mse


def oracle_state(model):
    """(parameters, buffers) of a model for the oracle's forward functions."""
    return O.split_state({k: v.detach().cpu() for k, v in model.state_dict().items()}, requires_grad=False)


def oracle_posterior(prm, buf, inputs, on, cond=None):
    """Eval-mode posterior of a request: inputs = [visual | None, tactile | None, pose | None], on: bool [B][3] (row b holds
    modality m; a modality passed as None is absent everywhere).  Row b is the oracle's product of experts over the prior and the
    experts row b holds.  -> (mu, lv) fp32 [B][L]."""
    B = on.shape[0]
    heads = [None, None, None]
    with O.eval_mode(), torch.no_grad():
        if inputs[0] is not None:
            heads[0] = O.image_encoder(inputs[0], prm, "visual_encoder", None, buf, cond)
        if inputs[1] is not None:
            heads[1] = O.image_encoder(inputs[1], prm, "tactile_encoder", None, buf, cond)
        if inputs[2] is not None:
            heads[2] = O.pose_encoder(inputs[2], prm)
    L = prm["visual_encoder.linear_means.bias"].shape[0]
    mu, lv = torch.zeros(B, L), torch.zeros(B, L)
    for b in range(B):
        mus, lvs = [torch.zeros(1, L)], [torch.zeros(1, L)]
        for m in range(3):
            if heads[m] is not None and bool(on[b, m]):
                mus.append(heads[m][0][b:b + 1])
                lvs.append(heads[m][1][b:b + 1])
        mu[b], lv[b] = (t[0] for t in O.product_of_experts(torch.stack(mus), torch.stack(lvs)))
    return mu, lv


def iw_request_ref(prm, buf, inputs, targets, eps, kl_weight, pose_multiplier, use_pose=True, available=None, target_available=None,
                   cond=None, loss_mask=None):
    """The bound of one request, restated on the oracle: inputs / targets = [visual | None, tactile | None, pose | None] (CPU
    tensors), eps [K][B][L], available / target_available: [B][3] (non-zero = present) or None, cond: what the oracle's heads /
    decoders concatenate (one-hot rows for a categorical model).  Everything fp64 except means / log_var / z (fp32)."""
    K, B, L = eps.shape
    inputs = list(inputs) + [None] * (3 - len(inputs))
    targets = list(targets) + [None] * (3 - len(targets))
    if not use_pose:
        inputs[2] = targets[2] = None
    on = torch.ones(B, 3, dtype=torch.bool) if available is None else (torch.as_tensor(available) != 0)
    if on.shape[1] == 2:
        on = torch.cat((on, torch.ones(B, 1, dtype=torch.bool)), 1)
    ton = None if target_available is None else (torch.as_tensor(target_available) != 0)
    if ton is not None and ton.shape[1] == 2:
        ton = torch.cat((ton, torch.ones(B, 1, dtype=torch.bool)), 1)
    mu, lv = oracle_posterior(prm, buf, inputs, on, cond)
    z, ratio = iw_latent_ref(mu, lv, eps)
    zz = z.reshape(K * B, L)
    cond_k = None if cond is None else cond.repeat((K,) + (1,) * (cond.dim() - 1))
    with O.eval_mode(), torch.no_grad():
        v = O.image_decoder(zz, prm, "visual_decoder", buf, cond_k)
        t = O.image_decoder(zz, prm, "tactile_decoder", buf, cond_k)
        pr = O.pose_decoder(zz, prm) if use_pose else None
    bce = torch.zeros(2, K, B, dtype=torch.float64)
    for s, (lg, tg) in enumerate(((v, targets[0]), (t, targets[1]))):
        if tg is not None:
            r, x = lg.double().reshape((K, B) + tuple(lg.shape[1:])), tg.double().unsqueeze(0)
            if loss_mask is not None:
                r, x = r * loss_mask.double().unsqueeze(0), x * loss_mask.double().unsqueeze(0)
            bce[s] = F.binary_cross_entropy_with_logits(r, x.expand_as(r), reduction="none").sum((2, 3, 4))
    mse = None
    if targets[2] is not None:
        mse = ((pr.double().reshape(K, B, -1) - targets[2].double().unsqueeze(0)) ** 2).sum(2)
    any_bce = targets[0] is not None or targets[1] is not None
    out, ess, log_w, bce_z, mse_z = iw_assemble_ref(bce if any_bce else None, mse, ratio, ton, pose_multiplier, kl_weight)
    kl = -0.5 * (1 + lv.double() - mu.double() ** 2 - lv.double().exp()).sum(1)
    return {"rows": out, "ess": ess, "log_w": log_w, "ratio": ratio, "kl": kl, "means": mu, "log_var": lv, "z": z,
            "bce_visual": bce_z[0] if targets[0] is not None else None, "bce_tactile": bce_z[1] if targets[1] is not None else None,
            "mse_pose": mse_z, "recon_x": [v, t] + ([pr] if use_pose else [])}
