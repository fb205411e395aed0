"""CPU emulation of the rollout's feed op (mmdyn_rollout_feed): :class:`EmuBackendIW` plus the one operation, written here from the
header's contract with ``torch.sigmoid`` and ``torch.where`` (never a multiplication by the table, so the side that is not taken
cannot reach the output even when it holds NaN).  Tests install it with ``ops.set_backend``; never imported by the product."""
import torch

from emu_backend_avail import _table
from emu_backend_iw import EmuBackendIW


class EmuBackendRollout(EmuBackendIW):

    def rollout_feed(self, groups, obs_avail, B):
        if not 1 <= len(groups) <= 4:
            raise ValueError("mmdyn_hip: rollout_feed: between 1 and 4 groups")
        on = _table(obs_avail, B, "rollout_feed")
        for g in groups:
            recon, obs, out = g["recon"], g.get("obs"), g["out"]
            if out.shape != recon.shape or recon.shape[0] != B or (obs is not None and obs.shape != recon.shape):
                raise ValueError("mmdyn_hip: rollout_feed: recon / obs / out differ in shape")
            if not 0 <= g["column"] < 4:
                raise ValueError("mmdyn_hip: rollout_feed: column outside the table")
            fill = torch.sigmoid(recon) if g["logits"] else recon
            if obs is None:
                out.copy_(fill)
                continue
            row = torch.ones(B, dtype=torch.bool) if on is None else on[:, g["column"]]
            out.copy_(torch.where(row.reshape((B,) + (1,) * (recon.dim() - 1)), obs, fill))
