"""CPU emulation of the candidate-condition ops (mmdyn_concat_condition_tiled, mmdyn_plan_select, mmdyn_gather_best):
:class:`EmuBackendRollout` plus the three operations, written here from the header's contract with plain torch on the CPU.  Wherever
a side is not taken -- an absent (row, term), a candidate that did not win -- it is kept out with ``torch.where`` or an index, never
with a multiplication, so a NaN there cannot reach the output.  Tests install it with ``ops.set_backend``; never imported by the
product."""
import torch

from emu_backend_avail import _table
from emu_backend_rollout import EmuBackendRollout


class EmuBackendPlan(EmuBackendRollout):

    def concat_condition_tiled(self, x, cond, out, K, cd, x_rows, bad_index=None):
        rows = out.shape[0]
        if x_rows < 1 or rows % x_rows or x.shape[0] != x_rows:
            raise ValueError(f"mmdyn_hip: concat_condition_tiled: rows={rows} is not a multiple of x_rows={x_rows} = the rows of x")
        self.concat_condition(x.repeat(rows // x_rows, 1), cond, out, K, cd, bad_index)

    def plan_select(self, bce_rows, mse_rows, kl_rows, tavail, candidates, cost, best, best_cost, best_condition, N, B,
                    pose_multiplier, kl_weight=1.0, kl_weight_dev=None):
        f64 = torch.float64
        for t, shape, what in ((bce_rows, (2, N, B), "bce_rows"), (mse_rows, (N, B), "mse_rows"), (kl_rows, (N, B), "kl_rows")):
            if t is not None and (t.dtype != f64 or tuple(t.shape) != shape):
                raise ValueError(f"mmdyn_hip: plan_select: {what} must be fp64 {shape}")
        index = candidates.dtype == torch.int64
        if candidates.shape[0] != N * B or best_condition.shape[0] != B or best_condition.dtype != candidates.dtype or \
                tuple(cost.shape) != (N, B) or best.dtype != torch.int32 or tuple(best.shape) != (B,) or tuple(best_cost.shape) != (B,):
            raise ValueError(f"mmdyn_hip: plan_select: tensors do not match [N={N}][B={B}]")
        if kl_weight_dev is not None:
            kl_weight = float(torch.tensor(kl_weight, dtype=torch.float32) * kl_weight_dev[0])
        on = _table(tavail, B, "plan_select")
        zero = torch.zeros(N, B, dtype=f64)

        def term(table, m):
            if table is None:
                return zero
            if on is not None:
                table.copy_(torch.where(on[:, m].unsqueeze(0), table, zero))       # the absent entries become 0 in the table
            return table
        c = term(None if bce_rows is None else bce_rows[0], 0) + term(None if bce_rows is None else bce_rows[1], 1)
        c = c + torch.tensor(pose_multiplier, dtype=f64) * term(mse_rows, 2)
        c = c + torch.tensor(kl_weight, dtype=f64) * kl_rows
        cost.copy_(c.to(torch.float32))
        for b in range(B):
            win, low = -1, float("nan")
            for n in range(N):
                v = float(c[n, b])
                if v == v and (win < 0 or v < low):
                    win, low = n, v
            best[b], best_cost[b] = win, low
            if win < 0:
                best_condition[b] = -1 if index else float("nan")
            else:
                best_condition[b] = candidates[win * B + b]

    def gather_best(self, groups, best, N, B):
        if not 1 <= len(groups) <= 4:
            raise ValueError("mmdyn_hip: gather_best: between 1 and 4 groups")
        if best.dtype != torch.int32 or tuple(best.shape) != (B,):
            raise ValueError(f"mmdyn_hip: gather_best: best must be int32 [B={B}]")
        taken = (best >= 0) & (best < N)
        rows = torch.where(taken, best.to(torch.int64), torch.zeros(B, dtype=torch.int64)) * B + torch.arange(B)
        for g in groups:
            src, out = g["src"], g["out"]
            if src.shape[0] != N * B or out.shape[0] != B or src.shape[1:] != out.shape[1:]:
                raise ValueError("mmdyn_hip: gather_best: src / out differ in row shape")
            picked = src[rows]                                                   # an index: the other rows are never read
            fill = torch.sigmoid(picked) if g["logits"] else picked
            out.copy_(torch.where(taken.reshape((B,) + (1,) * (src.dim() - 1)), fill, torch.full_like(fill, float("nan"))))
