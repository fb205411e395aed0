"""Restatements and seeded requests of the refinement tests (``MVAEInference.plan_refine``: the cross-entropy method on the horizon
planner), shared by tests/test_refine_emu.py and tests/test_refine_gpu.py.  The reference has no such operation, so nothing here comes
from a golden file.

``sample_ref`` / ``refit_ref`` restate the contracts of mmdyn_plan_sample / mmdyn_plan_refit (include/mmdyn_hip.h) with ONE torch
operation per rounding on the CPU, so each product, sum and quotient is rounded on its own as the header fixes it: the kernels'
``cand`` and ``mean_out`` must have these bits.  ``loop_ref`` chains them into the refinement loop on a cost that needs no model (the
squared distance to a fixed target sequence); its own convergence is asserted here, on the CPU, once.  ``chain`` is the loop a caller
of the parent commit would write around ``plan_rollout``, with the restatements in the host's part."""
import functools

import numpy as np
import torch

from mmdyn_hip.utils.seeded_init import seeded_batch

import cond_cases as CC
import rollout_cases as RC

CD = CC.REAL_DIM
# name -> (B, N, K, T, I, every step scored, bounds, seed): every step scored; a final goal with bounds and N past the row kernels'
# eight passes per launch; the smallest request over three iterations
CASES = {"steps": (2, 4, 2, 2, 2, True, False, 0),
         "nine": (2, 9, 3, 2, 2, False, True, 1),
         "one": (1, 3, 1, 1, 3, True, False, 2)}
LOOP = dict(B=3, N=32, K=4, T=2, cd=2, iterations=10, seed=4)


def f32(x):
    """The fp32 value a float argument has inside the kernel, as a Python float."""
    return float(np.float32(x))


# ---- mmdyn_plan_sample ---------------------------------------------------------------------------------------------------------
def sample_ref(mean, std, eps, keep=None, lo=None, hi=None):
    """cand [T][N * B][cd] from mean / std / keep [B][T][cd], eps [N][B][T][cd], lo / hi [cd] (fp32, CPU)."""
    N, B, T, cd = eps.shape
    p = std.unsqueeze(0) * eps                       # rounded to fp32
    c = mean.unsqueeze(0) + p                        # rounded to fp32
    first = mean if keep is None else torch.where(torch.isnan(keep), mean, keep)
    c = torch.cat((first.unsqueeze(0), c[1:]))       # the incumbent slot: its eps is not used
    if lo is not None:
        c = torch.where(c < lo, lo.expand_as(c), torch.where(c > hi, hi.expand_as(c), c))
    return c.permute(2, 0, 1, 3).reshape(T, N * B, cd).contiguous()


# ---- mmdyn_plan_refit ----------------------------------------------------------------------------------------------------------
def elites_ref(cost, K):
    """Per row b the elites of cost [N][B] in ascending n: the K smallest, ties to the lower n, NaN never."""
    N, B = cost.shape
    out = []
    for b in range(B):
        col = cost[:, b].tolist()
        order = sorted((n for n in range(N) if col[n] == col[n]), key=lambda n: (col[n], n))
        out.append(sorted(order[:K]))
    return out


def refit_ref(cost, cand, mean_in, std_in, K, alpha=0.0, std_min=0.0):
    """(mean_out, std_out fp32 [B][T][cd], elite uint8 [N][B], count int32 [B]) of the header's contract; fp64, one operation per
    rounding, the elites summed in ascending n."""
    N, B = cost.shape
    T, _, cd = cand.shape
    c4 = cand.view(T, N, B, cd)
    a = torch.tensor(f32(alpha), dtype=torch.float64)
    rest = torch.tensor(1.0, dtype=torch.float64) - a
    floor = torch.tensor(f32(std_min), dtype=torch.float32)
    mean_out, std_out = mean_in.clone(), std_in.clone()
    elite, count = torch.zeros(N, B, dtype=torch.uint8), torch.zeros(B, dtype=torch.int32)
    for b, idx in enumerate(elites_ref(cost, K)):
        count[b] = len(idx)
        if not idx:
            continue
        elite[idx, b] = 1
        kp = torch.tensor(float(len(idx)), dtype=torch.float64)
        rows = [c4[:, n, b].double() for n in idx]                   # [T][cd] each
        total = torch.zeros(T, cd, dtype=torch.float64)              # (the kernel's sums start from 0.0: -0.0 + 0.0 = +0.0)
        for r in rows:
            total = total + r
        m = total / kp
        acc = torch.zeros(T, cd, dtype=torch.float64)
        for r in rows:
            d = r - m
            sq = d * d
            acc = acc + sq
        s = torch.sqrt(acc / kp)
        mean_out[b] = (a * mean_in[b].double() + rest * m).float()
        std_out[b] = torch.fmax((a * std_in[b].double() + rest * s).float(), floor)
    return mean_out, std_out, elite, count


# ---- the loop without the model -------------------------------------------------------------------------------------------------
def distance_cost(cand, target, N, B):
    """cost [N][B] fp32 = the squared distance of candidate (n, b) to target [B][T][cd], in fp64 with the T * cd squares added one
    by one in (t, d) order -- the same bits on every device -- and rounded to fp32 at the end."""
    T, _, cd = cand.shape
    d = cand.view(T, N, B, cd).double() - target.double().permute(1, 0, 2).unsqueeze(1)
    sq = d * d
    total = None
    for t in range(T):
        for j in range(cd):
            total = sq[t, :, :, j] if total is None else total + sq[t, :, :, j]
    return total.float().contiguous()


def loop_inputs():
    """(init_mean, init_std, target [B][T][cd], the I draws [N][B][T][cd]) of the model-free loop."""
    B, N, T, cd, I = (LOOP[k] for k in ("B", "N", "T", "cd", "iterations"))
    g = torch.Generator().manual_seed(LOOP["seed"])
    target = 2.0 * torch.rand(B, T, cd, generator=g) - 1.0
    return torch.zeros(B, T, cd), torch.ones(B, T, cd), target, [torch.randn(N, B, T, cd, generator=g) for _ in range(I)]


@functools.lru_cache(maxsize=None)
def loop_ref():
    """Every iteration's (mean, std) of the restated loop: sample_ref -> distance_cost -> refit_ref, slot 0 = the previous winner.
    Its own worth is asserted here: every row's mean ends strictly closer to the target than the initial mean."""
    B, N, K = LOOP["B"], LOOP["N"], LOOP["K"]
    mean, std, target, draws = loop_inputs()
    first, keep, out = mean, None, []
    for eps in draws:
        cand = sample_ref(mean, std, eps, keep)
        cost = distance_cost(cand, target, N, B)
        win = [min((n for n in range(N)), key=lambda n: (float(cost[n, b]), n)) for b in range(B)]
        keep = torch.stack([cand.view(-1, N, B, cand.shape[2])[:, win[b], b] for b in range(B)])
        mean, std, _, _ = refit_ref(cost, cand, mean, std, K)
        out.append((mean, std))
    far = lambda m: ((m.double() - target.double()) ** 2).sum((1, 2))
    assert bool((far(mean) < far(first)).all()), (far(mean), far(first))
    return out


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def request(name):
    """(inputs [visual, tactile, pose], goal, init_mean [T, cd], init_std [T, cd], bounds | None, the I candidate draws
    [N][B][T][cd]) of one case, CPU tensors.  Conditions live in [0, 1] like those of tests/horizon_cases.py."""
    B, N, K, T, I, every, bounds, seed = CASES[name]
    inputs, _ = seeded_batch(B, 1700 + seed, with_pose=True)
    goal = RC.frames(1710 + seed, T if every else 1, B)
    if not every:
        goal = [t[0] for t in goal]
    g = torch.Generator().manual_seed(1720 + seed)
    mean = 0.25 + 0.5 * torch.rand(T, CD, generator=g)
    std = 0.1 + 0.2 * torch.rand(T, CD, generator=g)
    draws = [torch.randn(N, B, T, CD, generator=g) for _ in range(I)]
    return inputs, goal, mean, std, (torch.full((CD,), 0.2), torch.full((CD,), 0.8)) if bounds else None, draws


def chain(plan_rollout, name, iterations=None, alpha=0.0, std_min=0.0):
    """The loop on the host around ``plan_rollout(candidates [B, N, T, cd]) -> its result dict on the CPU``: per iteration the
    restated candidates, one request, the restated refit from the request's ``cost``.  Returns the last request's result plus
    ``mean`` / ``std`` / ``candidates`` [T][N * B][cd] / ``history`` [I][B] / ``elite_count`` [I][B]."""
    B, N, K, T, I = CASES[name][:5]
    I = I if iterations is None else iterations
    _, _, mean, std, bounds, draws = request(name)
    mean, std = mean.expand(B, T, CD).contiguous(), std.expand(B, T, CD).contiguous()
    lo, hi = bounds if bounds is not None else (None, None)
    keep, history, counts, r = None, [], [], None
    for i in range(I):
        cand = sample_ref(mean, std, draws[i], keep, lo, hi)
        r = plan_rollout(cand.view(T, N, B, CD).permute(2, 1, 0, 3).contiguous())
        keep = r["best_condition"]
        mean, std, _, count = refit_ref(r["cost"], cand, mean, std, K, alpha, std_min)
        history.append(r["best_cost"])
        counts.append(count)
    return dict(r, mean=mean, std=std, candidates=cand, history=torch.stack(history), elite_count=torch.stack(counts))
