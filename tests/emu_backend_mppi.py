"""CPU emulation of the MPPI ops (mmdyn_plan_refit_weighted, mmdyn_plan_shift): :class:`EmuBackendRefine` plus the two operations,
written here from the header's contract with plain torch on the CPU, row by row as the kernel works (the restatement in
tests/mppi_cases.py works on all rows at once and masks with ``torch.where``; here a candidate of weight zero is never indexed).
Tests install it with ``ops.set_backend``; never imported by the product."""
import math

import numpy as np
import torch

from emu_backend_refine import REFIT_N_MAX, EmuBackendRefine, _touch


class EmuBackendMppi(EmuBackendRefine):

    def plan_refit_weighted(self, cost, cand, mean_in, std_in, mean_out, std_out, elite, count, weight, ess, K, N, B, T,
                            temperature=1.0, alpha=0.0, std_min=0.0):
        f32, f64 = torch.float32, torch.float64
        temperature, alpha, std_min = float(np.float32(temperature)), float(np.float32(alpha)), float(np.float32(std_min))
        if B < 1 or T < 1 or not 1 <= N <= REFIT_N_MAX or not 1 <= K <= N:
            raise ValueError(f"mmdyn_hip: plan_refit_weighted: B={B}, T={T} must be positive, N={N} in [1, {REFIT_N_MAX}], K={K} in [1, N]")
        if not 0.0 <= alpha < 1.0 or not std_min >= 0.0:
            raise ValueError(f"mmdyn_hip: plan_refit_weighted: alpha={alpha} must lie in [0, 1) and std_min={std_min} be >= 0")
        if not 0.0 < temperature < math.inf:
            raise ValueError(f"mmdyn_hip: plan_refit_weighted: temperature={temperature} must be finite and > 0")
        if any(t is None for t in (cost, cand, mean_in, std_in, mean_out, std_out)):
            raise ValueError("mmdyn_hip: plan_refit_weighted: cost, cand, mean_in, std_in, mean_out and std_out are required")
        cd = cand.shape[-1]
        ins = [(cost, (N, B), f32, "cost"), (cand, (T, N * B, cd), f32, "cand"), (mean_in, (B, T, cd), f32, "mean_in"),
               (std_in, (B, T, cd), f32, "std_in")]
        outs = [(mean_out, (B, T, cd), f32, "mean_out"), (std_out, (B, T, cd), f32, "std_out"), (elite, (N, B), torch.uint8, "elite"),
                (count, (B,), torch.int32, "count"), (weight, (N, B), f64, "weight"), (ess, (B,), f32, "ess")]
        for t, shape, dtype, what in ins + outs:
            if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"mmdyn_hip: plan_refit_weighted: {what} must be contiguous {dtype} {shape}")
        for i, (o, _, _, what) in enumerate(outs):
            for j, (t, _, _, other) in enumerate(ins):
                own = i < 2 and j == i + 2 and o.data_ptr() == t.data_ptr()
                if not own and _touch(o, t):
                    raise ValueError(f"mmdyn_hip: plan_refit_weighted: {what} overlaps {other}")
            for p, _, _, other in outs[i + 1:]:
                if _touch(o, p):
                    raise ValueError(f"mmdyn_hip: plan_refit_weighted: {what} overlaps {other}")
        c4 = cand.view(T, N, B, cd)
        a = torch.tensor(alpha, dtype=f64)
        rest = torch.tensor(1.0, dtype=f64) - a
        floor = torch.tensor(std_min, dtype=f32)
        temp = torch.tensor(temperature, dtype=f64)
        index = torch.arange(N)
        for b in range(B):
            col = cost[:, b]
            if K == N:                                                   # nothing is cut: nothing is ranked
                flag = col == col
            else:
                ahead = ((col.unsqueeze(0) < col.unsqueeze(1)) | ((col.unsqueeze(0) == col.unsqueeze(1)) & (index.unsqueeze(0) < index.unsqueeze(1)))).sum(1)
                flag = (col == col) & (ahead < K)
            if elite is not None:
                elite[:, b] = flag.to(torch.uint8)
            idx = flag.nonzero().reshape(-1)                             # ascending n
            if count is not None:
                count[b] = idx.numel()
            m_in, s_in = mean_in[b].clone(), std_in[b].clone()
            w_col = torch.zeros(N, dtype=f64)
            if idx.numel():
                c = col[idx]
                c_min = c.min()
                d = c.to(f64) - c_min.to(f64)
                q = d / temp
                w = torch.exp(-q)
                w[c == c_min] = 1.0
                w_col[idx] = w
            if weight is not None:
                weight[:, b] = w_col
            if not idx.numel():
                mean_out[b], std_out[b] = m_in, s_in
                if ess is not None:
                    ess[b] = 0.0
                continue
            W = torch.zeros((), dtype=f64)
            Q = torch.zeros((), dtype=f64)
            for n in idx.tolist():                                       # (a zero in between adds nothing)
                W = W + w_col[n]
                Q = Q + w_col[n] * w_col[n]
            if ess is not None:
                ess[b] = ((W * W) / Q).to(f32)
            live = [n for n in idx.tolist() if float(w_col[n]) != 0.0]
            total = torch.zeros(T, cd, dtype=f64)
            for n in live:
                total = total + w_col[n] * c4[:, n, b].to(f64)
            m = total / W
            acc = torch.zeros(T, cd, dtype=f64)
            for n in live:
                d = c4[:, n, b].to(f64) - m
                acc = acc + w_col[n] * (d * d)
            s = torch.sqrt(acc / W)
            mean_out[b] = (a * m_in.to(f64) + rest * m).to(f32)
            std_out[b] = torch.fmax((a * s_in.to(f64) + rest * s).to(f32), floor)

    def plan_shift(self, prev_mean, prev_std, prev_keep, init_mean, init_std, mean_out, std_out, keep_out, B, T, shift=1, widen=0.0):
        f32 = torch.float32
        widen = float(np.float32(widen))
        if B < 1 or T < 1 or not 0 <= shift <= T:
            raise ValueError(f"mmdyn_hip: plan_shift: B={B}, T={T} must be positive and shift={shift} lie in [0, T]")
        if not 0.0 <= widen < math.inf:
            raise ValueError(f"mmdyn_hip: plan_shift: widen={widen} must be finite and >= 0")
        if any(t is None for t in (prev_mean, prev_std, init_mean, init_std, mean_out, std_out)) or (prev_keep is None) != (keep_out is None):
            raise ValueError("mmdyn_hip: plan_shift: the means and stds are required; prev_keep and keep_out come together")
        cd = prev_mean.shape[-1]
        ins = [(prev_mean, "prev_mean"), (prev_std, "prev_std"), (prev_keep, "prev_keep"), (init_mean, "init_mean"), (init_std, "init_std")]
        outs = [(mean_out, "mean_out"), (std_out, "std_out"), (keep_out, "keep_out")]
        for t, what in ins + outs:
            if t is not None and (t.dtype != f32 or tuple(t.shape) != (B, T, cd) or not t.is_contiguous()):
                raise ValueError(f"mmdyn_hip: plan_shift: {what} must be contiguous fp32 {(B, T, cd)}")
        for i, (o, what) in enumerate(outs):
            for t, other in ins + outs[i + 1:]:
                if _touch(o, t):
                    raise ValueError(f"mmdyn_hip: plan_shift: {what} overlaps {other}")
        w = torch.tensor(widen, dtype=f32)
        for t in range(T):
            if t + shift < T:
                mean_out[:, t] = prev_mean[:, t + shift]
                std_out[:, t] = torch.fmax(prev_std[:, t + shift], w * init_std[:, t])
                if keep_out is not None:
                    keep_out[:, t] = prev_keep[:, t + shift]
            else:
                mean_out[:, t] = init_mean[:, t]
                std_out[:, t] = init_std[:, t]
                if keep_out is not None:
                    keep_out[:, t] = init_mean[:, t]
