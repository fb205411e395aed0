"""CPU emulation of the importance-weighted bound's ops (mmdyn_iw_latent, mmdyn_iw_assemble_rows): :class:`EmuBackendEvalGrad` plus the
two operations, written here from the header's contract with plain torch loops over k (tests/iw_cases.py restates them a second time,
vectorised, with torch.logsumexp).  :class:`Recorder` wraps any backend and lists the ops the product calls on it, in call order.
Tests install either with ``ops.set_backend``; never imported by the product."""
import math

import torch

from emu_backend_avail import _table
from emu_backend_evalgrad import EmuBackendEvalGrad


class EmuBackendIW(EmuBackendEvalGrad):

    def iw_latent(self, mu, lv, eps_noise, z, ratio, K, B, L):
        if ratio.dtype != torch.float64 or tuple(ratio.shape) != (K, B):
            raise ValueError(f"mmdyn_hip: iw_latent: ratio must be fp64 [K={K}][B={B}]")
        if tuple(eps_noise.shape) != (K, B, L) or tuple(z.shape) != (K, B, L) or tuple(mu.shape) != (B, L) or tuple(lv.shape) != (B, L):
            raise ValueError(f"mmdyn_hip: iw_latent: tensors do not match [K={K}][B={B}][L={L}]")
        for k in range(K):
            z[k] = eps_noise[k] * torch.exp(0.5 * lv) + mu
            zk, ek = z[k].double(), eps_noise[k].double()
            ratio[k] = (0.5 * (zk * zk - ek * ek - lv.double())).sum(1)

    def iw_assemble_rows(self, bce_rows, mse_rows, ratio, tavail, out, ess, log_w, K, B, pose_multiplier, kl_weight=1.0,
                         kl_weight_dev=None):
        if kl_weight_dev is not None:
            kl_weight = float(torch.tensor(kl_weight, dtype=torch.float32) * kl_weight_dev[0])
        on = _table(tavail, B, "iw_assemble_rows")
        lw = torch.empty(K, B, dtype=torch.float64)
        for k in range(K):
            rec = torch.zeros(B, dtype=torch.float64)
            for s in range(0 if bce_rows is None else bce_rows.shape[0]):
                if on is not None:
                    bce_rows[s, k] = torch.where(on[:, s], bce_rows[s, k], torch.zeros_like(bce_rows[s, k]))
                rec = rec + bce_rows[s, k]
            if mse_rows is not None:
                if on is not None:
                    mse_rows[k] = torch.where(on[:, 2], mse_rows[k], torch.zeros_like(mse_rows[k]))
                rec = rec + pose_multiplier * mse_rows[k]
            lw[k] = -(rec + kl_weight * ratio[k])
        if log_w is not None:
            log_w.copy_(lw)
        for b in range(B):
            col = lw[:, b]
            mx = float(col[~torch.isnan(col)].max()) if bool((~torch.isnan(col)).any()) else float("nan")
            if bool(torch.isnan(col).any()):
                res = n_eff = float("nan")
            elif math.isinf(mx):
                res, n_eff = -mx, float("nan")
            else:
                e = torch.exp(col - mx)
                s1, s2 = float(e.sum()), float((e * e).sum())
                res, n_eff = -((mx + math.log(s1)) - math.log(K)), s1 * s1 / s2
            out[b] = res
            if ess is not None:
                ess[b] = n_eff


class Recorder:
    """Forwards every attribute to ``inner``; calls of public methods are listed by name in ``ops``."""

    def __init__(self, inner):
        object.__setattr__(self, "inner", inner)
        object.__setattr__(self, "ops", [])

    def __getattr__(self, name):
        attr = getattr(self.inner, name)
        if name.startswith("_") or not callable(attr):
            return attr

        def call(*a, **k):
            self.ops.append(name)
            return attr(*a, **k)
        return call

    def __setattr__(self, name, value):
        setattr(self.inner, name, value)
