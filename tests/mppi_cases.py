"""Restatements of the MPPI tests (``MVAEInference.plan_refine(temperature=..., warm_start=...)``), shared by tests/test_mppi_emu.py
and tests/test_mppi_gpu.py.  The reference has no such operation, so nothing here comes from a golden file.

``weights_ref`` / ``refit_weighted_ref`` / ``shift_ref`` restate the contracts of mmdyn_plan_refit_weighted / mmdyn_plan_shift
(include/mmdyn_hip.h) with ONE torch operation per rounding on the CPU, in the manner of tests/refine_cases.py.  The one operation
whose rounding a math library decides is the fp64 ``exp`` of the weights; ``refit_weighted_ref`` therefore takes the weights as an
optional argument, so the sums can be restated from the weights a backend wrote: ``mean_out`` must then have these bits."""
import torch

import refine_cases as RF

f32 = RF.f32
EXP_ULPS = 4          # allowed fp64 distance of a device weight to torch's: both libraries document <= 1 ulp for exp; twice their sum
Q_ULP_MAX = 700.0     # the arguments of the ulp comparison: exp(-q) is a normal number for q <= 700 ...
Q_ZERO_MIN = 800.0    # ... and exactly 0 from q = 800 on (the smallest subnormal is exp(-744.4))


def weights_ref(cost, K, temperature):
    """(weight fp64 [N][B], q fp64 [N][B], elite uint8 [N][B], count int32 [B]): the header's weights of cost [N][B] with torch's
    fp64 exp.  q is the exponent's argument (NaN where the weight does not come from exp: non-elites and elites at c_min)."""
    N, B = cost.shape
    temp = torch.tensor(f32(temperature), dtype=torch.float64)
    weight, q_all = torch.zeros(N, B, dtype=torch.float64), torch.full((N, B), float("nan"), dtype=torch.float64)
    elite, count = torch.zeros(N, B, dtype=torch.uint8), torch.zeros(B, dtype=torch.int32)
    for b, idx in enumerate(RF.elites_ref(cost, K)):
        count[b] = len(idx)
        if not idx:
            continue
        elite[idx, b] = 1
        c = cost[idx, b]
        c_min = c.min()
        d = c.double() - c_min.double()
        q = d / temp
        w = torch.exp(-q)
        at_min = c == c_min
        weight[idx, b] = torch.where(at_min, torch.ones_like(w), w)
        q_all[idx, b] = torch.where(at_min, torch.full_like(q, float("nan")), q)
    return weight, q_all, elite, count


def refit_weighted_ref(cost, cand, mean_in, std_in, K, temperature, alpha=0.0, std_min=0.0, weights=None):
    """(mean_out, std_out fp32 [B][T][cd], elite uint8 [N][B], count int32 [B], weight fp64 [N][B], ess fp32 [B]) of the header's
    contract: fp64, one operation per rounding, every sum in ascending n.  ``weights``: fp64 [N][B] to take in place of
    ``weights_ref``'s (the elites and their count always come from the costs).  A candidate of weight zero is kept out by
    ``torch.where``, never by its product."""
    N, B = cost.shape
    T, _, cd = cand.shape
    c4 = cand.view(T, N, B, cd).double()
    own, _, elite, count = weights_ref(cost, K, temperature)
    weight = own if weights is None else weights.clone()
    a = torch.tensor(f32(alpha), dtype=torch.float64)
    rest = torch.tensor(1.0, dtype=torch.float64) - a
    floor = torch.tensor(f32(std_min), dtype=torch.float32)
    W, Q = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    for n in range(N):
        w = weight[n]
        W = W + w
        ww = w * w
        Q = Q + ww
    some = count > 0
    sq_w = W * W
    ess = torch.where(some, (sq_w / Q).float(), torch.zeros(B))
    total = torch.zeros(T, B, cd, dtype=torch.float64)                   # (the kernel's sums start from 0.0)
    for n in range(N):
        w = weight[n].view(1, B, 1)
        p = w * c4[:, n]
        total = torch.where(w != 0, total + p, total)
    m = total / W.view(1, B, 1)
    acc = torch.zeros(T, B, cd, dtype=torch.float64)
    for n in range(N):
        w = weight[n].view(1, B, 1)
        d = c4[:, n] - m
        sq = d * d
        p = w * sq
        acc = torch.where(w != 0, acc + p, acc)
    s = torch.sqrt(acc / W.view(1, B, 1))
    mean_fit = (a * mean_in.double() + rest * m.transpose(0, 1)).float()
    std_fit = torch.fmax((a * std_in.double() + rest * s.transpose(0, 1)).float(), floor)
    keep = some.view(B, 1, 1)
    return torch.where(keep, mean_fit, mean_in), torch.where(keep, std_fit, std_in), elite, count, weight, ess


def shift_ref(prev_mean, prev_std, prev_keep, init_mean, init_std, shift, widen):
    """(mean_out, std_out, keep_out | None) of mmdyn_plan_shift: fp32 [B][T][cd] each."""
    T = prev_mean.shape[1]
    w = torch.tensor(f32(widen), dtype=torch.float32)
    mean, std, keep = init_mean.clone(), init_std.clone(), init_mean.clone()
    if shift < T:
        mean[:, :T - shift] = prev_mean[:, shift:]
        floor = w * init_std[:, :T - shift]                              # one fp32 product
        std[:, :T - shift] = torch.fmax(prev_std[:, shift:], floor)
        if prev_keep is not None:
            keep[:, :T - shift] = prev_keep[:, shift:]
    return mean, std, (keep if prev_keep is not None else None)


def ulps64(a, b):
    """Largest distance of two fp64 tensors of one sign in units in the last place."""
    return int((a.contiguous().view(torch.int64) - b.contiguous().view(torch.int64)).abs().max()) if a.numel() else 0


def stepped(w, k):
    """The weights moved k fp64 ulps (towards larger values for k > 0) wherever they come from exp: strictly inside (0, 1)."""
    moved = (w.contiguous().view(torch.int64) + k).view(torch.float64)
    return torch.where((w > 0) & (w < 1), moved, w)
