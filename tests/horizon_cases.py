"""Seeded requests of the horizon-planner tests (``MVAEInference.plan_rollout``) and their restatements on oracle/mvae_oracle.py,
shared by tests/test_horizon_emu.py and tests/test_horizon_gpu.py.  The reference has no such operation, so nothing here comes from a
golden file: step t of candidate n is the oracle's eval-mode forward of a state with condition (n, t) (tests/rollout_cases.py:
``oracle_step``), its terms the fp64 terms of that pass against the step's goal (``step_terms``), the next state ``next_state`` with
nothing observed; the total is the weighted sum over the scored steps and the choice its argmin.  The models are those of
tests/plan_cases.py (``build``: COND_SCALE 40).

``select_steps_ref`` restates the contract of mmdyn_plan_select_steps on fp64 tables: every product and every sum is one torch
operation, so each is rounded on its own, as the header fixes it."""
import functools

import torch
import torch.nn.functional as F

from mmdyn_hip.utils.seeded_init import seeded_batch

import cond_cases as CC
import plan_cases as PC
import rollout_cases as RC

L = PC.L
KL_WEIGHT, POSE_MULTIPLIER = PC.KL_WEIGHT, PC.POSE_MULTIPLIER
# name -> (B, N, T, categorical, per-row candidates, every step scored, step weights, seed): every step scored; a final goal alone;
# class-index sequences under weights; per-row candidates past the row kernels' eight passes per launch
CASES = {"steps": (2, 3, 2, False, False, True, None, 0),
         "final": (2, 3, 3, False, False, False, None, 1),
         "classes": (2, 4, 2, True, False, True, (0.5, 1.0), 2),
         "nine": (2, 9, 2, False, True, True, (1.0, 0.9), 3)}


def request(name):
    """(inputs [visual, tactile, pose], goal [visual, tactile, pose] -- [T, B, ...] each, or [B, ...] for a final goal --,
    candidates as the caller passes them, step weights [Tg] | None) of one case, CPU tensors."""
    B, N, T, categorical, per_row, every, weights, seed = CASES[name]
    inputs, _ = seeded_batch(B, 1100 + seed, with_pose=True)
    goal = RC.frames(1200 + seed, T if every else 1, B)
    if not every:
        goal = [t[0] for t in goal]
    g = torch.Generator().manual_seed(1300 + seed)
    if categorical:
        # distinct index sequences: sequence n is the base-CAT_DIM digits of a number drawn without replacement
        code = torch.randperm(CC.CAT_DIM ** T, generator=g)[:N]
        cand = torch.stack([(code // CC.CAT_DIM ** t) % CC.CAT_DIM for t in range(T)], 1)
        assert len({tuple(r) for r in cand.tolist()}) == N
    else:
        cand = torch.rand((B, N, T, CC.REAL_DIM) if per_row else (N, T, CC.REAL_DIM), generator=g)
    return inputs, goal, cand, None if weights is None else torch.tensor(weights, dtype=torch.float32)


def candidate_rows(cand, B, categorical):
    """[T][N][B][cd] fp32: the condition the oracle takes for (step t, candidate n, row b) -- one-hot rows for a categorical model."""
    if categorical:
        idx = cand.permute(2, 1, 0) if cand.dim() == 3 else cand.t().unsqueeze(2).expand(cand.shape[1], cand.shape[0], B)
        return F.one_hot(idx.to(torch.int64), CC.CAT_DIM).float()
    if cand.dim() == 4:
        return cand.permute(2, 1, 0, 3).contiguous()
    return cand.transpose(0, 1).unsqueeze(2).expand(cand.shape[1], cand.shape[0], B, cand.shape[2]).contiguous()


def select_steps_ref(bce, mse, kl, on, weights, pose_multiplier, kl_weight):
    """The contract of mmdyn_plan_select_steps on fp64 tables [Tg][N][B] (bce: [2][Tg][N][B]; ``on``: bool [Tg][B][3] or None;
    ``weights``: fp32 [Tg] or None): (c [Tg][N][B] fp64, total [N][B] fp64, best int32 [B], order: per row the list of n by
    ascending total, equal totals in n order, NaN left out)."""
    Tg, N, B = kl.shape
    zero = torch.zeros(N, B, dtype=torch.float64)
    cs, total = [], None
    for t in range(Tg):
        pick = lambda tab, m: zero if tab is None else (tab[t] if on is None else torch.where(on[t][:, m].unsqueeze(0), tab[t], zero))
        c = pick(None if bce is None else bce[0], 0) + pick(None if bce is None else bce[1], 1)
        c = c + torch.tensor(float(pose_multiplier), dtype=torch.float64) * pick(mse, 2)
        c = c + torch.tensor(float(kl_weight), dtype=torch.float64) * kl[t]
        cs.append(c)
        term = c if weights is None else weights[t].to(torch.float64) * c
        total = term if total is None else total + term
    order = []
    for b in range(B):
        col = total[:, b].tolist()
        order.append(sorted((n for n in range(N) if col[n] == col[n]), key=lambda n: (col[n], n)))
    best = torch.tensor([o[0] if o else -1 for o in order], dtype=torch.int32)
    return torch.stack(cs), total, best, order


def chained(model, inputs, goal, rows, weights, every, eps=None, available=None, goal_available=None, kl_weight=KL_WEIGHT,
            pose_multiplier=POSE_MULTIPLIER):
    """The fully chained restatement: oracle states fed to the oracle.  ``rows``: [T][N][B][cd]; ``eps``: T draws [B, L] (None: the
    posterior means).  A dict of ``step_cost`` [Tg][N][B] and ``cost`` [N][B] (fp64) and ``best`` [B]."""
    prm, buf = RC.oracle_state(model)
    T, N, B = rows.shape[:3]
    Tg = T if every else 1
    on = None if available is None else torch.as_tensor(available) != 0
    gon = None if goal_available is None else torch.as_tensor(goal_available) != 0
    step_cost = torch.zeros(Tg, N, B, dtype=torch.float64)
    for n in range(N):
        state = inputs
        for t in range(T):
            e = torch.zeros(B, L) if eps is None else eps[t]
            v, tc, pr, mu, lv = RC.oracle_step(prm, buf, state, on if t == 0 else None, e, rows[t, n])
            if every or t == T - 1:
                s = t if every else 0
                g = [x[s] for x in goal] if every else goal
                ga = None if gon is None else (gon[s] if every else gon)
                step_cost[s, n] = RC.step_terms(v, tc, pr, mu, lv, g, ga, pose_multiplier, kl_weight)["rows"]
            state = RC.next_state(v, tc, pr, None, None)
    w = torch.ones(Tg, dtype=torch.float64) if weights is None else weights.to(torch.float64)
    cost = (w.reshape(Tg, 1, 1) * step_cost).sum(0)
    return {"step_cost": step_cost, "cost": cost, "best": torch.argmin(cost, 0)}


@functools.lru_cache(maxsize=None)
def restated(name):
    """The chained restatement of a case at the posterior means, computed once per session and shared (read-only)."""
    B, N, T, categorical, per_row, every, weights, seed = CASES[name]
    inputs, goal, cand, w = request(name)
    return chained(PC.build(categorical), inputs, goal, candidate_rows(cand, B, categorical), w, every)


def random_tables(B, N, T, seed):
    """Random fp64 tables of the sizes the engine produces: (bce [2][T][N][B], mse [T][N][B], kl [T][N][B])."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    return 8000.0 + 1000.0 * r(2, T, N, B), 0.5 * r(T, N, B), 20.0 + 30.0 * r(T, N, B)
