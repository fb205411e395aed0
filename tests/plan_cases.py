"""Seeded requests of the candidate-condition tests (``MVAEInference.plan``) and their restatement on oracle/mvae_oracle.py, shared by
tests/test_plan_emu.py and tests/test_plan_gpu.py.  The reference has no such operation, so nothing here comes from a golden file:
candidate n of a row is the oracle's eval-mode forward of that row with condition n (tests/rollout_cases.py: ``oracle_step``), its
cost the fp64 terms of that pass against the goal (``step_terms``), the choice the argmin over n.

The models are those of ``cond_cases.model_kw`` with seeded weights.  The seeded initialisation leaves the six condition blocks
(``cond_cases.COND_WEIGHTS``) too weak to separate candidates by ten times the tolerance of the cost comparison, which the tests of
the CHOICE require of the restatement alone; the set-up here multiplies those columns by COND_SCALE (a constant of the test model,
chosen on the oracle, never on the code under test)."""
import functools

import torch
import torch.nn.functional as F

from mmdyn_hip.models import setup_model
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_running_stats, seeded_state_dict

import cond_cases as CC
import rollout_cases as RC

L = CC.LATENT
KL_WEIGHT, POSE_MULTIPLIER = 0.3, 1000.0
COND_SCALE = 40.0
# name -> (B, N, categorical, per-row candidates): all classes of a categorical model; shared real candidates; per-row candidates
# past the row kernels' eight passes per launch; the smallest request
CASES = {"classes": (3, 5, True, False), "shared": (3, 3, False, False), "per_row": (2, 9, False, True), "one": (1, 1, False, False)}
# the mixed request: the rows of rollout_cases.START hold (visual, tactile, pose) as listed there
GOAL_ON = [(1, 1, 1), (0, 1, 1), (1, 1, 0)]           # which goal terms row b has


def build(categorical, device="cpu", scale=COND_SCALE):
    m = setup_model("cnn-mvae", cross_modal=True, **CC.model_kw(categorical, True))
    sd = seeded_running_stats(seeded_state_dict(m.state_dict(), 0))
    cd = CC.CAT_DIM if categorical else CC.REAL_DIM
    for k in CC.COND_WEIGHTS:
        sd[k] = sd[k].clone()
        sd[k][:, -cd:] *= scale
    m.load_state_dict(sd)
    return m.to(device).eval()


def request(name):
    """(inputs [visual, tactile, pose], goal [visual, tactile, pose], candidates as the caller passes them (None: all classes),
    eps [B, L]) of one case, CPU tensors."""
    B, N, categorical, per_row = CASES[name]
    inputs, goal = seeded_batch(B, 900 + len(name), with_pose=True)
    g = torch.Generator().manual_seed(90 + B + N)
    eps = torch.randn(B, L, generator=g)
    if categorical:
        cand = None
    else:
        cand = torch.rand((B, N, CC.REAL_DIM) if per_row else (N, CC.REAL_DIM), generator=g)
    return inputs, goal, cand, eps


def candidate_rows(name, cand):
    """[N][B][cd] fp32: the condition the oracle takes for (candidate n, row b) -- one-hot rows for a categorical model."""
    B, N, categorical, per_row = CASES[name]
    if categorical:
        idx = torch.arange(CC.CAT_DIM) if cand is None else cand
        idx = idx.t() if idx.dim() == 2 else idx.unsqueeze(1).expand(idx.shape[0], B)
        return F.one_hot(idx.to(torch.int64), CC.CAT_DIM).float()
    return cand.transpose(0, 1).contiguous() if per_row else cand.unsqueeze(1).expand(N, B, CC.REAL_DIM).contiguous()


def restate(model, inputs, goal, cand_rows, eps, available=None, goal_available=None, kl_weight=KL_WEIGHT,
            pose_multiplier=POSE_MULTIPLIER):
    """The fp64 tables of the request from the oracle, one forward per (candidate, row): a dict of [N][B] tensors ``cost``,
    ``bce_visual``, ``bce_tactile``, ``mse_pose``, ``kl``, plus ``means`` / ``log_var`` [N][B][L], the logits / pose outputs
    ``visual`` / ``tactile`` / ``pose`` [N][B][...] and ``best`` [B]."""
    prm, buf = RC.oracle_state(model)
    on = None if available is None else torch.as_tensor(available) != 0
    gon = None if goal_available is None else torch.as_tensor(goal_available) != 0
    cols = {k: [] for k in ("cost", "bce_visual", "bce_tactile", "mse_pose", "kl", "means", "log_var", "visual", "tactile", "pose")}
    for c in cand_rows:
        v, t, pr, mu, lv = RC.oracle_step(prm, buf, inputs, on, eps, c)
        terms = RC.step_terms(v, t, pr, mu, lv, goal, gon, pose_multiplier, kl_weight)
        for k, x in (("cost", terms["rows"]), ("bce_visual", terms["bce_visual"]), ("bce_tactile", terms["bce_tactile"]),
                     ("mse_pose", terms["mse_pose"]), ("kl", terms["kl"]), ("means", mu), ("log_var", lv), ("visual", v),
                     ("tactile", t), ("pose", pr)):
            cols[k].append(x)
    out = {k: (None if v[0] is None else torch.stack(v)) for k, v in cols.items()}
    out["best"] = torch.argmin(out["cost"], 0)
    return out


@functools.lru_cache(maxsize=None)
def restated(name, sample, mixed=False):
    """The restatement of a case, computed once per session and shared (read-only).  ``sample`` False: eps = 0 (the posterior
    mean); ``mixed``: the request's rows hold rollout_cases.START and the goal GOAL_ON."""
    B, N, categorical, _ = CASES[name]
    inputs, goal, cand, eps = request(name)
    model = build(categorical)
    av = torch.tensor(RC.START, dtype=torch.float64) if mixed else None
    gav = torch.tensor(GOAL_ON, dtype=torch.float64) if mixed else None
    return restate(model, inputs, goal, candidate_rows(name, cand), eps if sample else torch.zeros_like(eps), av, gav)


def gap(cost):
    """Per row: (runner-up - best) of an [N][B] fp64 cost table; +inf for N = 1."""
    if cost.shape[0] < 2:
        return torch.full((cost.shape[1],), float("inf"), dtype=torch.float64)
    s = torch.sort(cost, 0).values
    return s[1] - s[0]


# ---- mmdyn_plan_select: tables and the restatement of its contract ------------------------------------------------------------
def select_ref(bce, mse, kl, on, pose_multiplier, kl_weight):
    """fp64 cost [N][B] in the written order ((bce_v + bce_t) + pm * mse) + klw * kl -- absent (row, term) and missing tables enter
    as 0 --, its fp32 rounding, and the argmin with the lowest index among equals (NaN never wins; all NaN: -1)."""
    N, B = kl.shape
    zero = torch.zeros(N, B, dtype=torch.float64)
    pick = lambda tab, m: zero if tab is None else (tab if on is None else torch.where(on[:, m].unsqueeze(0), tab, zero))
    c = pick(None if bce is None else bce[0], 0) + pick(None if bce is None else bce[1], 1)
    c = c + torch.tensor(float(pose_multiplier), dtype=torch.float64) * pick(mse, 2)
    c = c + torch.tensor(float(kl_weight), dtype=torch.float64) * kl
    best = torch.empty(B, dtype=torch.int32)
    for b in range(B):
        col = c[:, b]
        ok = (~torch.isnan(col)).nonzero().reshape(-1)
        if ok.numel() == 0:
            best[b] = -1
        else:
            m = col[ok].min()
            best[b] = int(ok[(col[ok] == m).nonzero()[0, 0]])
    return c, c.to(torch.float32), best


def random_tables(B, N, seed):
    """Random fp64 tables of the sizes the engine produces: (bce [2][N][B], mse [N][B], kl [N][B])."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    return 8000.0 + 1000.0 * r(2, N, B), 0.5 * r(N, B), 20.0 + 30.0 * r(N, B)
