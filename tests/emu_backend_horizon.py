"""CPU emulation of the horizon planner's ops (mmdyn_plan_select_steps, mmdyn_gather_best_steps): :class:`EmuBackendPlan` plus the two
operations, written here from the header's contract with plain torch on the CPU.  Wherever a side is not taken -- an absent (step,
row, term), a candidate that did not win -- it is kept out with ``torch.where`` or an index, never with a multiplication, so a NaN
there cannot reach the output.  Tests install it with ``ops.set_backend``; never imported by the product."""
import torch

from emu_backend_avail import _table
from emu_backend_plan import EmuBackendPlan

TOP_MAX = 8


class EmuBackendHorizon(EmuBackendPlan):

    def plan_select_steps(self, bce_rows, mse_rows, kl_rows, tavail, step_weight, candidates, cost, step_cost, best, best_cost,
                          best_condition, top, top_cost, N, B, T, Tg, pose_multiplier, kl_weight=1.0, kl_weight_dev=None):
        f64 = torch.float64
        if N < 1 or B < 1 or T < 1 or Tg not in (1, T):
            raise ValueError(f"mmdyn_hip: plan_select_steps: N={N}, B={B}, T={T} must be positive and Tg={Tg} be 1 or T")
        for t, shape, what in ((bce_rows, (2, Tg, N, B), "bce_rows"), (mse_rows, (Tg, N, B), "mse_rows"), (kl_rows, (Tg, N, B), "kl_rows")):
            if t is not None and (t.dtype != f64 or tuple(t.shape) != shape):
                raise ValueError(f"mmdyn_hip: plan_select_steps: {what} must be fp64 {shape}")
        index = candidates.dtype == torch.int64
        if tuple(candidates.shape[:2]) != (T, N * B) or tuple(best_condition.shape[:2]) != (B, T) or \
                best_condition.dtype != candidates.dtype or tuple(cost.shape) != (N, B) or tuple(step_cost.shape) != (Tg, N, B) or \
                best.dtype != torch.int32 or tuple(best.shape) != (B,) or tuple(best_cost.shape) != (B,):
            raise ValueError(f"mmdyn_hip: plan_select_steps: tensors do not match [T={T}][N={N}][B={B}]")
        if step_weight is not None and (step_weight.dtype != torch.float32 or tuple(step_weight.shape) != (Tg,)):
            raise ValueError(f"mmdyn_hip: plan_select_steps: step_weight must be fp32 [Tg={Tg}]")
        if (top is None) != (top_cost is None):
            raise ValueError("mmdyn_hip: plan_select_steps: top and top_cost come together")
        K = 0 if top is None else top.shape[0]
        if top is not None and (not 1 <= K <= TOP_MAX or tuple(top.shape) != (K, B) or tuple(top_cost.shape) != (K, B) or
                                top.dtype != torch.int32):
            raise ValueError(f"mmdyn_hip: plan_select_steps: top / top_cost must be [K <= {TOP_MAX}][B={B}]")
        if tavail is not None and tuple(tavail.shape[:2]) != (Tg, B):
            raise ValueError(f"mmdyn_hip: plan_select_steps: the availability tables must be [Tg={Tg}][B={B}][4]")
        if kl_weight_dev is not None:
            kl_weight = float(torch.tensor(kl_weight, dtype=torch.float32) * kl_weight_dev[0])
        zero = torch.zeros(N, B, dtype=f64)
        total = None
        for t in range(Tg):
            on = None if tavail is None else _table(tavail[t], B, "plan_select_steps")

            def term(table, m):
                if table is None:
                    return zero
                if on is not None:
                    table.copy_(torch.where(on[:, m].unsqueeze(0), table, zero))       # the absent entries become 0 in the table
                return table
            c = term(None if bce_rows is None else bce_rows[0, t], 0) + term(None if bce_rows is None else bce_rows[1, t], 1)
            c = c + torch.tensor(pose_multiplier, dtype=f64) * term(None if mse_rows is None else mse_rows[t], 2)
            c = c + torch.tensor(kl_weight, dtype=f64) * kl_rows[t]
            step_cost[t].copy_(c.to(torch.float32))
            if step_weight is not None:
                c = step_weight[t].to(f64) * c                                         # its own rounding, then the sum's
            total = c if total is None else total + c
        cost.copy_(total.to(torch.float32))
        nan = float("nan")
        for b in range(B):
            order = []                                                                 # (total, n) ascending; equal totals in n order
            for n in range(N):
                v = float(total[n, b])
                if v == v:
                    k = len(order)
                    while k > 0 and v < order[k - 1][0]:
                        k -= 1
                    order.insert(k, (v, n))
            win, low = (order[0][1], order[0][0]) if order else (-1, nan)
            best[b], best_cost[b] = win, low
            for t in range(T):
                if win < 0:
                    best_condition[b, t] = -1 if index else nan
                else:
                    best_condition[b, t] = candidates[t, win * B + b]
            for k in range(K):
                top[k, b], top_cost[k, b] = (order[k][1], order[k][0]) if k < len(order) else (-1, nan)

    def gather_best_steps(self, groups, best, N, B, T):
        if not 1 <= len(groups) <= 4:
            raise ValueError("mmdyn_hip: gather_best_steps: between 1 and 4 groups")
        if best.dtype != torch.int32 or tuple(best.shape) != (B,):
            raise ValueError(f"mmdyn_hip: gather_best_steps: best must be int32 [B={B}]")
        taken = (best >= 0) & (best < N)
        rows = torch.where(taken, best.to(torch.int64), torch.zeros(B, dtype=torch.int64)) * B + torch.arange(B)
        for g in groups:
            src, out = g["src"], g["out"]
            if tuple(src.shape[:2]) != (T, N * B) or tuple(out.shape[:2]) != (T, B) or src.shape[2:] != out.shape[2:]:
                raise ValueError("mmdyn_hip: gather_best_steps: src / out differ in row shape")
            picked = src[:, rows]                                                # an index: the other rows are never read
            fill = torch.sigmoid(picked) if g["logits"] else picked
            out.copy_(torch.where(taken.reshape((1, B) + (1,) * (src.dim() - 2)), fill, torch.full_like(fill, float("nan"))))
