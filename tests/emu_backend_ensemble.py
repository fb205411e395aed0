"""CPU emulation of the ensemble rollout's feed op (mmdyn_ensemble_feed): :class:`EmuBackendPlan` plus the one operation, written here
from the header's contract with ``torch.sigmoid``, ``torch.where`` (never a multiplication by the table, so an observation row that
is not taken cannot reach the output even when it holds NaN) and a TWO-pass fp64 mean / variance -- not the kernel's single pass.
Tests install it with ``ops.set_backend``; never imported by the product."""
import torch

from emu_backend_avail import _table
from emu_backend_plan import EmuBackendPlan


class EmuBackendEnsemble(EmuBackendPlan):

    def ensemble_feed(self, groups, obs_avail, N, B):
        if not 1 <= len(groups) <= 4:
            raise ValueError("mmdyn_hip: ensemble_feed: between 1 and 4 groups")
        if N < 1 or B < 1:
            raise ValueError("mmdyn_hip: ensemble_feed: N and B must be positive")
        on = _table(obs_avail, B, "ensemble_feed")
        for g in groups:
            recon, obs, out, mean, var, spread = g["recon"], g.get("obs"), g["out"], g["mean"], g.get("var"), g.get("spread")
            row = tuple(recon.shape[1:])
            if recon.shape[0] != N * B or out.shape != recon.shape or tuple(mean.shape) != (B,) + row or \
                    any(t is not None and tuple(t.shape) != (B,) + row for t in (obs, var)):
                raise ValueError("mmdyn_hip: ensemble_feed: recon / out [N * B, ...] and obs / mean / var [B, ...] differ in row shape")
            if spread is not None and (var is None or spread.dtype != torch.float64 or tuple(spread.shape) != (B,)):
                raise ValueError("mmdyn_hip: ensemble_feed: spread must be fp64 [B] and needs var")
            if not 0 <= g["column"] < 4:
                raise ValueError("mmdyn_hip: ensemble_feed: column outside the table")
            p = (torch.sigmoid(recon) if g["logits"] else recon).reshape((N, B) + row)
            if obs is None:
                out.copy_(p.reshape(out.shape))
            else:
                taken = torch.ones(B, dtype=torch.bool) if on is None else on[:, g["column"]]
                taken = taken.reshape((1, B) + (1,) * len(row))
                out.copy_(torch.where(taken, obs.unsqueeze(0), p).reshape(out.shape))
            p64 = p.double()
            m = p64.sum(0) / N
            v = ((p64 - m.unsqueeze(0)) ** 2).sum(0) / N
            mean.copy_(m.to(torch.float32))
            if var is not None:
                var.copy_(v.to(torch.float32))
            if spread is not None:
                spread += var.double().reshape(B, -1).sum(1)
