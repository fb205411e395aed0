"""CPU emulation of the refinement ops (mmdyn_plan_sample, mmdyn_plan_refit): :class:`EmuBackendHorizon` plus the two operations,
written here from the header's contract with plain torch on the CPU.  A candidate that is no elite is kept out of the refit by an
index, the incumbent slot and the clamp by ``torch.where`` -- never by a multiplication, so a NaN on the side that is not taken cannot
reach the output.  The elites are found as the kernel finds them, by counting the candidates in front of each one (the restatement in
tests/refine_cases.py sorts instead).  Tests install it with ``ops.set_backend``; never imported by the product."""
import numpy as np
import torch

from emu_backend_horizon import EmuBackendHorizon

REFIT_N_MAX = 4096


def _touch(a, b):
    if a is None or b is None:
        return False
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


class EmuBackendRefine(EmuBackendHorizon):

    def plan_sample(self, mean, std, eps, keep, lo, hi, cand, N, B, T):
        f32 = torch.float32
        if N < 1 or B < 1 or T < 1:
            raise ValueError(f"mmdyn_hip: plan_sample: N={N}, B={B}, T={T} must be positive")
        if any(t is None for t in (mean, std, eps, cand)) or (lo is None) != (hi is None):
            raise ValueError("mmdyn_hip: plan_sample: mean, std, eps and cand are required; lo and hi come together")
        cd = mean.shape[-1]
        for t, shape, what in ((mean, (B, T, cd), "mean"), (std, (B, T, cd), "std"), (eps, (N, B, T, cd), "eps"), (keep, (B, T, cd), "keep"),
                               (lo, (cd,), "lo"), (hi, (cd,), "hi"), (cand, (T, N * B, cd), "cand")):
            if t is not None and (t.dtype != f32 or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"mmdyn_hip: plan_sample: {what} must be contiguous fp32 {shape}")
            if t is not None and t is not cand and _touch(cand, t):
                raise ValueError(f"mmdyn_hip: plan_sample: cand overlaps {what}")
        out = cand.view(T, N, B, cd)
        first = mean if keep is None else torch.where(keep == keep, keep, mean)
        out[:, 0] = first.transpose(0, 1)
        if N > 1:
            p = std.unsqueeze(0) * eps[1:]
            out[:, 1:] = (mean.unsqueeze(0) + p).permute(2, 0, 1, 3)
        if lo is not None:
            c = out.clone()
            out.copy_(torch.where(c < lo, lo.expand_as(c), torch.where(c > hi, hi.expand_as(c), c)))

    def plan_refit(self, cost, cand, mean_in, std_in, mean_out, std_out, elite, count, K, N, B, T, alpha=0.0, std_min=0.0):
        f32, f64 = torch.float32, torch.float64
        alpha, std_min = float(np.float32(alpha)), float(np.float32(std_min))
        if B < 1 or T < 1 or not 1 <= N <= REFIT_N_MAX or not 1 <= K <= N:
            raise ValueError(f"mmdyn_hip: plan_refit: B={B}, T={T} must be positive, N={N} in [1, {REFIT_N_MAX}], K={K} in [1, N]")
        if not 0.0 <= alpha < 1.0 or not std_min >= 0.0:
            raise ValueError(f"mmdyn_hip: plan_refit: alpha={alpha} must lie in [0, 1) and std_min={std_min} be >= 0")
        if any(t is None for t in (cost, cand, mean_in, std_in, mean_out, std_out)):
            raise ValueError("mmdyn_hip: plan_refit: cost, cand, mean_in, std_in, mean_out and std_out are required")
        cd = cand.shape[-1]
        ins = [(cost, (N, B), f32, "cost"), (cand, (T, N * B, cd), f32, "cand"), (mean_in, (B, T, cd), f32, "mean_in"),
               (std_in, (B, T, cd), f32, "std_in")]
        outs = [(mean_out, (B, T, cd), f32, "mean_out"), (std_out, (B, T, cd), f32, "std_out"), (elite, (N, B), torch.uint8, "elite"),
                (count, (B,), torch.int32, "count")]
        for t, shape, dtype, what in ins + outs:
            if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"mmdyn_hip: plan_refit: {what} must be contiguous {dtype} {shape}")
        for i, (o, _, _, what) in enumerate(outs):
            for j, (t, _, _, other) in enumerate(ins):
                own = i < 2 and j == i + 2 and o.data_ptr() == t.data_ptr()
                if not own and _touch(o, t):
                    raise ValueError(f"mmdyn_hip: plan_refit: {what} overlaps {other}")
            for p, _, _, other in outs[i + 1:]:
                if _touch(o, p):
                    raise ValueError(f"mmdyn_hip: plan_refit: {what} overlaps {other}")
        c4 = cand.view(T, N, B, cd)
        a = torch.tensor(alpha, dtype=f64)
        rest = torch.tensor(1.0, dtype=f64) - a
        floor = torch.tensor(std_min, dtype=f32)
        index = torch.arange(N)
        for b in range(B):
            col = cost[:, b]
            # ahead[n] = the candidates m in front of n: a smaller cost, or an equal one with a lower index (NaN: in front of nothing)
            ahead = ((col.unsqueeze(0) < col.unsqueeze(1)) | ((col.unsqueeze(0) == col.unsqueeze(1)) & (index.unsqueeze(0) < index.unsqueeze(1)))).sum(1)
            flag = (col == col) & (ahead < K)
            if elite is not None:
                elite[:, b] = flag.to(torch.uint8)
            idx = flag.nonzero().reshape(-1).tolist()                 # ascending n
            if count is not None:
                count[b] = len(idx)
            m_in, s_in = mean_in[b].clone(), std_in[b].clone()
            if not idx:
                mean_out[b], std_out[b] = m_in, s_in
                continue
            kp = torch.tensor(float(len(idx)), dtype=f64)
            total = torch.zeros(T, cd, dtype=f64)
            for n in idx:
                total = total + c4[:, n, b].to(f64)
            m = total / kp
            acc = torch.zeros(T, cd, dtype=f64)
            for n in idx:
                d = c4[:, n, b].to(f64) - m
                acc = acc + d * d
            s = torch.sqrt(acc / kp)
            mean_out[b] = (a * m_in.to(f64) + rest * m).to(f32)
            std_out[b] = torch.fmax((a * s_in.to(f64) + rest * s).to(f32), floor)
