"""The horizon planner on the CPU: ``MVAEInference.plan_rollout`` through the emulation backend (tests/emu_backend_horizon.py) -- every
link against the oracle's forward of the engine's own states, the choice against the fully chained oracle (tests/horizon_cases.py),
T = 1 against ``plan``, N = 1 against ``rollout`` --, the rules of ``plan_select_steps`` on integer-valued tables and its fp64
restatement, ``gather_best_steps`` against T ``gather_best`` calls, the launch accounting, the error paths and
``DynModeling.plan_rollout``.  The ``check_*`` functions take the backend and / or the device: tests/test_horizon_gpu.py runs them
on the HIP library."""
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

import cond_cases as CC
import dirty
import horizon_cases as HC
import plan_cases as PC
import rollout_cases as RC
import synthetic_tree as ST
import test_mixed_modal_emu as TMM
import test_plan_emu as TP
from emu_backend_horizon import EmuBackendHorizon
from emu_backend_plan import EmuBackendPlan
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise, setup_model
from mmdyn_hip.models.functional import availability_table
from mmdyn_hip.problems.problems import DynModeling
from test_elbo_rows_emu import REL          # engine rows against the oracle: the bound that file and its GPU twin apply
from test_ensemble_emu import ShapeRecorder

OUT_TOL = TMM.OUT_TOL
L = HC.L
KW = dict(kl_weight=HC.KL_WEIGHT, pose_multiplier=HC.POSE_MULTIPLIER)
KLW = float(np.float32(HC.KL_WEIGHT))       # the weight as the kernel sees it: an fp32 word in device memory
TERMS = ("bce_visual", "bce_tactile", "mse_pose", "kl")
STATES = ("visual", "tactile", "pose")
KEYS = {"cost", "step_cost", "best", "best_cost", "best_condition", "trajectory", "means", "log_var"} | set(TERMS) | set(STATES)
GAP = 10 * REL                              # the chained restatement's best-to-runner-up gap, relative to the best cost, that pins ``best``


@pytest.fixture(autouse=True)
def emu_horizon():
    old = ops.set_backend(EmuBackendHorizon())
    yield
    ops.set_backend(old)


dev_list, keep = TP.dev_list, TP.keep


def same_bits(a, b):
    return dirty.first_diff(a, b) is None


# ---- plan_select_steps: tables built on the host, no model -----------------------------------------------------------------------
def run_steps(backend, device, bce, mse, kl, table, weights, cand, pm, klw=1.0, klw_dev=None, top=None, T=None):
    """One launch on copies of the tables ([Tg][N][B]; bce [2][Tg][N][B]); ``table``: [Tg][B][3] or None; ``cand``: [T][N * B](cd);
    every destination pre-filled with sevens."""
    Tg, N, B = kl.shape
    T = cand.shape[0] if T is None else T
    mv = lambda t: None if t is None else t.clone().to(device)
    bce, mse, kl, cand, weights = mv(bce), mv(mse), mv(kl), mv(cand), mv(weights)
    tab = None if table is None else availability_table(table.reshape(Tg * B, -1), Tg * B, device).view(Tg, B, -1)
    full = lambda *s, dtype=torch.float32: torch.full(s, 7, dtype=dtype, device=device)
    cost, step_cost, best, best_cost = full(N, B), full(Tg, N, B), full(B, dtype=torch.int32), full(B)
    best_cond = full(*((B, T) + tuple(cand.shape[2:])), dtype=cand.dtype)
    tk, tc = (None, None) if top is None else (full(top, B, dtype=torch.int32), full(top, B))
    backend.plan_select_steps(bce, mse, kl, tab, weights, cand, cost, step_cost, best, best_cost, best_cond, tk, tc, N, B, T, Tg, pm,
                              klw, None if klw_dev is None else torch.tensor([klw_dev], device=device))
    out = dict(cost=cost, step_cost=step_cost, best=best, best_cost=best_cost, best_cond=best_cond, top=tk, top_cost=tc, bce=bce, mse=mse)
    return {k: None if v is None else v.cpu() for k, v in out.items()}


def nn(t, fill=-7.0):
    return torch.nan_to_num(t, nan=fill)


def check_select_rules(backend, device):
    """1. The rules on integer-valued tables (exact in any order of summation)."""
    nan, inf = float("nan"), float("inf")
    f64 = torch.float64
    Tg, N, B, cd = 2, 4, 6, 2
    # rows: an exact tie of totals reached through different splits (candidates 1 and 3); a NaN in ONE step of the candidate that
    # would win; all NaN; +inf against finite; -inf wins; a plain row
    s0 = torch.tensor([[5, 1, 9, 0], [3, nan, 1, 4], [nan, nan, nan, nan], [inf, inf, 8, 1], [1, -inf, 0, 2], [4, 3, 2, 1]], dtype=f64).t()
    s1 = torch.tensor([[0, 1, 0, 2], [0, -5, 0, 0], [0, 0, 0, 0], [0, 0, 0, inf], [0, 5, 0, 0], [0, 0, 0, 0]], dtype=f64).t()
    bce = torch.zeros(2, Tg, N, B, dtype=f64)
    bce[0, 0], bce[0, 1] = s0, s1
    kl = torch.zeros(Tg, N, B, dtype=f64)
    cand = torch.arange(Tg * N * B * cd, dtype=torch.float32).reshape(Tg, N * B, cd) + 1.0
    r = run_steps(backend, device, bce, None, kl, None, None, cand, 1000.0, top=3)
    assert r["best"].tolist() == [1, 2, -1, 2, 1, 3]
    assert torch.equal(nn(r["best_cost"]), nn(torch.tensor([2.0, 1.0, nan, 8.0, -inf, 1.0])))
    assert torch.equal(nn(r["cost"]), nn((s0 + s1).float())) and torch.equal(nn(r["step_cost"]), nn(torch.stack((s0, s1)).float()))
    for b, w in enumerate(r["best"].tolist()):          # the winner's T conditions
        for t in range(Tg):
            assert bool(torch.isnan(r["best_cond"][b, t]).all()) if w < 0 else torch.equal(r["best_cond"][b, t], cand[t, w * B + b])
    assert r["top"].t().tolist() == [[1, 3, 0], [2, 0, 3], [-1, -1, -1], [2, 0, 1], [1, 2, 0], [3, 2, 1]]
    assert torch.equal(nn(r["top_cost"].t()), nn(torch.tensor([[2, 2, 5], [1, 3, 4], [nan, nan, nan], [8, inf, inf], [-inf, 0, 1],
                                                                 [1, 2, 3]], dtype=torch.float32)))
    # class-index candidates: the winner's T indices, -1 where every total is NaN
    idx = (torch.arange(Tg * N * B) % 5).to(torch.int64).reshape(Tg, N * B)
    r = run_steps(backend, device, bce, None, kl, None, None, idx, 1000.0)
    assert r["best_cond"].dtype == torch.int64
    assert r["best_cond"].tolist() == [[int(idx[t, w * B + b]) if w >= 0 else -1 for t in range(Tg)] for b, w in enumerate(r["best"].tolist())]
    # every term with integer values; pose_multiplier 4; the KL weight 3 from the device word (times the argument 1); the step
    # weights (2, 3) from device memory; absent (step, row, term) entries holding NaN / Inf are left out and read 0 afterwards
    g = torch.Generator().manual_seed(3)
    ri = lambda *s: torch.randint(0, 50, s, generator=g).to(f64)
    bce, mse, kl = ri(2, Tg, N, B), ri(Tg, N, B), ri(Tg, N, B)
    on = torch.tensor([[[1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0], [0, 0, 0], [1, 1, 1]],
                       [[1, 1, 1], [1, 1, 1], [1, 0, 0], [0, 1, 1], [1, 1, 1], [0, 0, 0]]], dtype=torch.bool)
    bce[0, 0][:, 1], mse[0][:, 3], bce[1, 1][:, 2], bce[0, 1][:, 5] = nan, inf, -inf, nan
    w = torch.tensor([2.0, 3.0])
    r = run_steps(backend, device, bce, mse, kl, on.to(f64), w, cand, 4.0, 1.0, klw_dev=3.0)
    c, total, best, _ = HC.select_steps_ref(bce, mse, kl, on, w, 4.0, 3.0)
    assert bool(torch.isfinite(total).all())
    assert torch.equal(r["step_cost"], c.float()) and torch.equal(r["cost"], total.float()) and torch.equal(r["best"], best)
    z = torch.zeros(N, B, dtype=f64)
    for t in range(Tg):
        pick = lambda tab, m: torch.where(on[t][:, m].unsqueeze(0), tab, z)
        assert torch.equal(r["bce"][0, t], pick(bce[0, t], 0)) and torch.equal(r["bce"][1, t], pick(bce[1, t], 1))
        assert torch.equal(r["mse"][t], pick(mse[t], 2))
    # without the pointer the argument alone is the KL weight
    r2 = run_steps(backend, device, bce, mse, kl, on.to(f64), w, cand, 4.0, 3.0)
    assert torch.equal(r2["cost"], r["cost"]) and torch.equal(r2["best"], r["best"])
    # a final goal: the tables hold the one scored step, the winner's condition is copied for all T steps
    cand3 = torch.arange(3 * N * B * cd, dtype=torch.float32).reshape(3, N * B, cd)
    r3 = run_steps(backend, device, r["bce"][:, 1:], r["mse"][1:], kl[1:], None, None, cand3, 4.0, 3.0)
    assert tuple(r3["best_cond"].shape) == (B, 3, cd) and tuple(r3["step_cost"].shape) == (1, N, B)
    assert all(torch.equal(r3["best_cond"][b, t], cand3[t, int(r3["best"][b]) * B + b]) for b in range(B) for t in range(3))


def check_one_step_is_plan_select(backend, device, B, N):
    """2. Tg = T = 1 without weights: the bits of plan_select on the same tables."""
    bce, mse, kl = PC.random_tables(B, N, 40 + B + N)
    on = torch.rand(B, 3, generator=torch.Generator().manual_seed(B)) < 0.8
    cand = torch.rand(N * B, 3, generator=torch.Generator().manual_seed(N))
    for table in (None, on.to(torch.float64)):
        a = TP.run_select(backend, device, bce, mse, kl, table, cand, PC.POSE_MULTIPLIER, 1.0, klw_dev=PC.KL_WEIGHT)
        b = run_steps(backend, device, bce.unsqueeze(1), mse.unsqueeze(0), kl.unsqueeze(0), None if table is None else table.unsqueeze(0),
                      None, cand.unsqueeze(0), PC.POSE_MULTIPLIER, 1.0, klw_dev=PC.KL_WEIGHT)
        assert same_bits(a["cost"], b["cost"]) and same_bits(a["cost"], b["step_cost"][0]) and same_bits(a["best"], b["best"])
        assert same_bits(a["best_cost"], b["best_cost"]) and same_bits(a["best_cond"], b["best_cond"][:, 0])
        assert same_bits(a["bce"], b["bce"][:, 0]) and same_bits(a["mse"], b["mse"][0])


def check_total_is_not_contracted(backend, device):
    """4. total = total + w * c in the WRITTEN order -- the product rounded before it is added -- not a fused multiply-add.  Two
    candidates whose written-order fp64 totals tie exactly at 1.0, so candidate 0 must win; with w_1 * c_1 fused into the sum,
    candidate 1 would come out at 1 - 2^-52 and win.  Then the mirror image, where the fused form would lift candidate 0 above the
    tie.  The premises are asserted in exact rational arithmetic."""
    f64 = torch.float64
    w = 3.0
    m1 = 1.0 + 2.0 ** -52                                       # 3 * m1 = 3 + 3 * 2^-52 is no double: it rounds to 3 + 2^-50
    p1 = w * m1
    assert Fraction(p1) - Fraction(w) * Fraction(m1) == Fraction(1, 2 ** 52)
    v0, v1 = 1.0 - w * 1.0, 1.0 - p1                            # both exact
    assert v0 + w * 1.0 == 1.0 == v1 + p1                       # the written order: a tie
    fused = float(Fraction(v1) + Fraction(w) * Fraction(m1))    # one rounding of the exact sum
    assert fused == 1.0 - 2.0 ** -52 and fused < 1.0
    Tg, N, B = 2, 2, 2
    weights = torch.tensor([1.0, w])
    cand = torch.arange(Tg * N * B * 2, dtype=torch.float32).reshape(Tg, N * B, 2)
    kl = torch.zeros(Tg, N, B, dtype=f64)

    def run(c0, c1):
        """c0 / c1: [N] the step costs of the two candidates, carried by the visual table alone (c = ((v + 0) + pm * 0) + klw * 0)."""
        bce = torch.zeros(2, Tg, N, B, dtype=f64)
        bce[0, 0] = torch.tensor(c0, dtype=f64).unsqueeze(1).expand(N, B)
        bce[0, 1] = torch.tensor(c1, dtype=f64).unsqueeze(1).expand(N, B)
        return run_steps(backend, device, bce, None, kl, None, weights, cand, 1000.0, 1.0, top=2)
    r = run([v0, v1], [1.0, m1])
    assert r["best"].tolist() == [0, 0] and r["top"].tolist() == [[0, 0], [1, 1]], (r["best"], r["top"])
    assert r["cost"].tolist() == [[1.0, 1.0], [1.0, 1.0]] and r["best_cost"].tolist() == [1.0, 1.0]
    m2 = 1.0 + 3.0 * 2.0 ** -52                                 # 3 * m2 = 3 + 9 * 2^-52 rounds DOWN to 3 + 2^-49
    p2 = w * m2
    assert Fraction(w) * Fraction(m2) - Fraction(p2) == Fraction(1, 2 ** 52)
    u0, u1 = 1.0 - p2, 1.0 - w * 1.0
    assert u0 + p2 == 1.0 == u1 + w * 1.0 and float(Fraction(u0) + Fraction(w) * Fraction(m2)) > 1.0
    r = run([u0, u1], [m2, 1.0])                                # fused: candidate 0 costs more than 1.0 and candidate 1 would win
    assert r["best"].tolist() == [0, 0] and r["top"].tolist() == [[0, 0], [1, 1]], (r["best"], r["top"])


def check_select_restatement(backend, device, B, N, T):
    """3. + 5. Random tables against the restatement, exactly (the contract fixes every rounding): with and without the
    availability tables, with fp32 weights, without, and with weights of 1.0 as a tensor (the bits of None); ``top`` with K in
    {1, 3, 8}, K > N included; two runs give the same bits."""
    bce, mse, kl = HC.random_tables(B, N, T, 60 + B + N + T)
    g = torch.Generator().manual_seed(B + T)
    on = torch.rand(T, B, 3, generator=g) < 0.8
    weights = torch.rand(T, generator=g) + 0.25
    cand = torch.rand(T, N * B, 3, generator=torch.Generator().manual_seed(N))
    rows = torch.arange(B)
    for table in (None, on):
        for w in (None, weights):
            c, total, best, order = HC.select_steps_ref(bce, mse, kl, table, w, HC.POSE_MULTIPLIER, KLW)
            for K in (1, 3, 8):
                runs = [run_steps(backend, device, bce, mse, kl, None if table is None else table.to(torch.float64), w, cand,
                                  HC.POSE_MULTIPLIER, 1.0, klw_dev=HC.KL_WEIGHT, top=K) for _ in range(2)]
                r = runs[0]
                assert torch.equal(r["step_cost"], c.float()) and torch.equal(r["cost"], total.float()) and torch.equal(r["best"], best)
                assert torch.equal(r["best_cost"], total[best.long(), rows].float())
                assert all(torch.equal(r["best_cond"][:, t], cand[t, best.long() * B + rows]) for t in range(T))
                want = torch.tensor([[o[k] if k < len(o) else -1 for o in order] for k in range(K)], dtype=torch.int32)
                assert torch.equal(r["top"], want) and torch.equal(r["top"][0], r["best"])
                listed = want >= 0
                assert torch.equal(r["top_cost"][listed], total[want.long().clamp_min(0), rows.expand(K, B)][listed].float())
                assert bool(torch.isnan(r["top_cost"][~listed]).all()) and (K <= N or not bool(listed[N:].any()))
                assert all(same_bits(runs[0][k], runs[1][k]) for k in ("cost", "step_cost", "best", "best_cost", "best_cond", "top", "top_cost"))
            if w is None:
                ones = run_steps(backend, device, bce, mse, kl, None if table is None else table.to(torch.float64), torch.ones(T),
                                 cand, HC.POSE_MULTIPLIER, 1.0, klw_dev=HC.KL_WEIGHT, top=8)
                assert all(same_bits(ones[k], r[k]) for k in ("cost", "step_cost", "best", "best_cost", "best_cond", "top", "top_cost"))


# ---- gather_best_steps --------------------------------------------------------------------------------------------------------
def shifted(device, shape, shift):
    """A contiguous destination that starts ``shift`` floats past a 16-byte boundary."""
    n = int(np.prod(shape))
    out = torch.zeros(n + 4, device=device)[shift:shift + n].view(shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4 * shift
    return out


def check_gather_steps(backend, device, row_lens, B, N, T, shift):
    """7. One launch against T gather_best calls on the step slices, bit for bit -- with a row without a winner and an index >= N
    (NaN rows in every step) --, and with NaN over every source row that is not taken: the output is unchanged."""
    gen = lambda seed, *s: torch.randn(*s, generator=torch.Generator().manual_seed(seed))
    best = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(7 + B)).to(torch.int32)
    if B >= 2:
        best[1] = -1
    if B >= 3:
        best[B - 1] = N
    best = best.to(device)
    taken = ((best >= 0) & (best < N)).cpu()

    def operands():
        return [dict(src=(3.0 * gen(970 + g, T, N * B, n)).to(device), out=shifted(device, (T, B, n), shift), logits=g == 1)
                for g, n in enumerate(row_lens)]
    got, want = operands(), operands()
    backend.gather_best_steps(got, best, N, B, T)
    for t in range(T):
        backend.gather_best([dict(src=g["src"][t], out=g["out"][t], logits=g["logits"]) for g in want], best, N, B)
    for g, w in zip(got, want):
        assert same_bits(g["out"], w["out"]), dirty.first_diff(g["out"], w["out"])
        assert bool(torch.isfinite(g["out"][:, taken]).all()) and bool(torch.isnan(g["out"][:, ~taken]).all())
        if not g["logits"]:
            assert torch.equal(g["out"][0, 0], g["src"][0, int(best[0]) * B])
    clean = [g["out"].clone() for g in got]
    keep_rows = torch.zeros(N * B, dtype=torch.bool)
    keep_rows[(best.cpu().long() * B + torch.arange(B))[taken]] = True
    for g in got:
        g["src"][:, ~keep_rows.to(device)] = float("nan")
        g["out"].fill_(0.0)
    backend.gather_best_steps(got, best, N, B, T)
    for g, c in zip(got, clean):
        assert same_bits(g["out"], c)


# ---- the engine -----------------------------------------------------------------------------------------------------------------
def ask(eng, name, device, eps=None, **over):
    """One plan_rollout() call of a case; ``eps``: the T draws [B, L] to inject (sample=True), None: the posterior means."""
    B, N, T = HC.CASES[name][:3]
    inputs, goal, cand, w = HC.request(name)
    kw = dict(x=dev_list(inputs[:2], device), pose=inputs[2].to(device), steps=T, goal=dev_list(goal, device), candidates=cand.to(device),
              step_weight=w, sample=eps is not None, **KW)
    kw.update(over)
    if eps is not None:
        eng.noise = InjectedNoise([e.clone() for e in eps], [])
    return keep(eng.plan_rollout(**kw))


def cpu(r):
    c = lambda v: None if v is None else ([c(t) for t in v] if isinstance(v, (list, tuple)) else v.cpu())
    return {k: c(v) for k, v in r.items()}


def assert_gap(want, what):
    """The choice is only pinned where the chained restatement itself separates the best candidate from the runner-up by ten times
    the tolerance of the cost comparison: asserted for every row, no row is skipped."""
    g, low = PC.gap(want["cost"]), want["cost"].min(0).values.abs()
    print(what, "gap / |best cost| per row", (g / low).tolist(), "needed", GAP)
    assert bool((g >= GAP * low).all()), (what, g, low)


def tables_of(r):
    bce = None if r["bce_visual"] is None and r["bce_tactile"] is None else \
        torch.stack([torch.zeros_like(r["kl"]) if r[k] is None else r[k] for k in TERMS[:2]])
    return bce, r["mse_pose"], r["kl"]


def check_own_tables(r, weights, top=None, klw=KLW):
    """``cost`` / ``step_cost`` / ``best`` (/ ``top``) are the kernel's restatement applied to the engine's own fp64 tables, exactly."""
    bce, mse, kl = tables_of(r)
    c, total, best, order = HC.select_steps_ref(bce, mse, kl, None, weights, HC.POSE_MULTIPLIER, klw)
    assert torch.equal(r["step_cost"], c.float()) and torch.equal(r["cost"], total.float()) and torch.equal(r["best"], best)
    assert torch.equal(r["best_cost"], total[best.long(), torch.arange(best.numel())].float())
    if top is not None:
        assert r["top"].tolist() == [[o[k] if k < len(o) else -1 for o in order] for k in range(top)]


def check_one_step_consistency(device, name, sample, sigmoid_atol=0.0):
    """8. Every (step, candidate) against the oracle's eval-mode forward of the engine's OWN state slot t - 1 (the request at t = 0)
    with candidate (n, t) and the step's draw: nothing compounds, so the tolerances are those of one forward."""
    B, N, T, categorical, per_row, every, weights, _ = HC.CASES[name]
    model = PC.build(categorical, device)
    eng = MVAEInference(model, use_graph=False)
    inputs, goal, cand, w = HC.request(name)
    eps = RC.draws(35, T, B) if sample else None
    r = cpu(ask(eng, name, device, eps, top=min(N, 3)))
    Tg = T if every else 1
    assert set(r) == KEYS | {"top", "top_cost"}
    assert tuple(r["cost"].shape) == (N, B) and tuple(r["step_cost"].shape) == (Tg, N, B) and r["cost"].dtype == torch.float32
    assert tuple(r["best"].shape) == (B,) and r["best"].dtype == torch.int32 and tuple(r["best_cost"].shape) == (B,)
    assert tuple(r["visual"].shape) == (T, N, B, 3, 64, 64) == tuple(r["tactile"].shape) and tuple(r["pose"].shape) == (T, N, B, 7)
    assert tuple(r["means"].shape) == (T, N, B, L) == tuple(r["log_var"].shape)
    assert [tuple(t.shape) for t in r["trajectory"]] == [(T, B, 3, 64, 64), (T, B, 3, 64, 64), (T, B, 7)]
    assert tuple(r["best_condition"].shape) == ((B, T) if categorical else (B, T, CC.REAL_DIM))
    assert all(tuple(r[k].shape) == (Tg, N, B) and r[k].dtype == torch.float64 for k in TERMS)
    prm, buf = RC.oracle_state(model)
    rows_of = HC.candidate_rows(cand, B, categorical)
    for t in range(T):
        for n in range(N):
            state = inputs if t == 0 else [r[k][t - 1, n] for k in STATES]
            e = eps[t] if sample else torch.zeros(B, L)
            v, tc, pr, mu, lv = RC.oracle_step(prm, buf, state, None, e, rows_of[t, n])
            np.testing.assert_allclose(r["means"][t, n].numpy(), mu.numpy(), **OUT_TOL, err_msg=f"means {t} {n}")
            np.testing.assert_allclose(r["log_var"][t, n].numpy(), lv.numpy(), **OUT_TOL, err_msg=f"log_var {t} {n}")
            np.testing.assert_allclose(r["pose"][t, n].numpy(), pr.numpy(), **OUT_TOL, err_msg=f"pose {t} {n}")
            for k, lg in (("visual", v), ("tactile", tc)):
                np.testing.assert_allclose(r[k][t, n].numpy(), torch.sigmoid(lg).numpy(), rtol=OUT_TOL["rtol"],
                                           atol=OUT_TOL["atol"] / 4 + sigmoid_atol, err_msg=f"{k} {t} {n}")
            if every or t == T - 1:
                s = t if every else 0
                want = RC.step_terms(v, tc, pr, mu, lv, [x[s] for x in goal] if every else goal, None, HC.POSE_MULTIPLIER, HC.KL_WEIGHT)
                for k in TERMS:
                    np.testing.assert_allclose(r[k][s, n].numpy(), want[k].numpy(), rtol=REL, err_msg=f"{k} {t} {n}")
                np.testing.assert_allclose(r["step_cost"][s, n].double().numpy(), want["rows"].numpy(), rtol=REL)
    check_own_tables(r, w, top=min(N, 3))
    if T > 1:
        moves = [float((r["means"][t + 1] - r["means"][t]).abs().median()) for t in range(T - 1)]
        print(name, "median |means[t+1] - means[t]|", moves)
        assert min(moves) > 100 * OUT_TOL["atol"]
    eng.close()
    return r


def check_choice(device, name):
    """9. ``best`` against the fully chained oracle (oracle states fed to the oracle), for every row, under the gap condition; the
    winner's cost, T conditions and trajectory are the winner's entries."""
    B, N, T, categorical, per_row, every, weights, _ = HC.CASES[name]
    want = HC.restated(name)
    assert_gap(want, name)
    eng = MVAEInference(PC.build(categorical, device), use_graph=False)
    cand, w = HC.request(name)[2:]
    r = cpu(ask(eng, name, device))
    print(name, "cost against the chained oracle, largest relative deviation", float(((r["cost"].double() - want["cost"]).abs() / want["cost"].abs()).max()))
    assert torch.equal(r["best"].long(), want["best"]), (r["best"], want["best"], r["cost"], want["cost"])
    rows, win = torch.arange(B), r["best"].long()
    assert torch.equal(r["best_cost"], r["cost"][win, rows])
    per = cand if per_row else cand.unsqueeze(0).expand((B,) + tuple(cand.shape))        # [B][N][T](cd)
    assert torch.equal(r["best_condition"], per[rows, win].to(r["best_condition"].dtype))
    for m, k in enumerate(STATES):
        assert same_bits(r["trajectory"][m], r[k][:, win, rows])
    check_own_tables(r, w)
    eng.close()


def check_one_step_is_plan(device, sample):
    """10. T = 1 with a [B] goal: every output shared with plan() has the bits of plan() on the same request."""
    name = "shared"
    B, N, categorical, _ = PC.CASES[name]
    eng = MVAEInference(PC.build(categorical, device), use_graph=False)
    inputs, goal, cand, eps = PC.request(name)
    a = TP.ask(eng, name, device, eps if sample else None)
    if sample:
        eng.noise = InjectedNoise([eps.clone()], [])
    b = keep(eng.plan_rollout(dev_list(inputs[:2], device), pose=inputs[2].to(device), steps=1, goal=dev_list(goal, device),
                              candidates=cand.unsqueeze(1).to(device), sample=sample, **dict(KW, kl_weight=PC.KL_WEIGHT)))
    pairs = [("cost", a["cost"], b["cost"]), ("step_cost", a["cost"], b["step_cost"][0]), ("best", a["best"], b["best"]),
             ("best_cost", a["best_cost"], b["best_cost"]), ("best_condition", a["best_condition"], b["best_condition"][:, 0]),
             ("means", a["means"], b["means"][0]), ("log_var", a["log_var"], b["log_var"][0])]
    pairs += [(k, a[k], b[k][0]) for k in TERMS] + [(f"prediction {m}", a["prediction"][m], b["trajectory"][m][0]) for m in range(3)]
    print("T = 1 against plan(): bit-equal", {k: same_bits(x, y) for k, x, y in pairs})
    for k, x, y in pairs:
        assert same_bits(x, y), (k, dirty.first_diff(x, y))
    eng.close()


def check_one_candidate_is_rollout(device):
    """11. N = 1: the trajectory slots, means and log_var have the bits of rollout(steps=T, condition=that sequence); the terms are
    within REL of its targets= tables; best == 0."""
    B, T = 3, 3
    model = PC.build(False, device)
    eng = MVAEInference(model, use_graph=False)
    inputs = dev_list(RC.start()[0], device)
    goal = dev_list(RC.frames(1401, T, B), device)
    cond = torch.rand(T, B, CC.REAL_DIM, generator=torch.Generator().manual_seed(14)).to(device)
    eps = RC.draws(36, T, B)
    eng.noise = InjectedNoise([e.clone() for e in eps], [])
    a = TP.keep(eng.rollout(inputs[:2], pose=inputs[2], steps=T, condition=cond, sample=True, targets=goal, **KW))
    eng.noise = InjectedNoise([e.clone() for e in eps], [])
    b = keep(eng.plan_rollout(inputs[:2], pose=inputs[2], steps=T, goal=goal, candidates=cond.transpose(0, 1).unsqueeze(1), sample=True, **KW))
    assert b["best"].tolist() == [0] * B
    for k in STATES + ("means", "log_var"):
        assert same_bits(a[k], b[k][:, 0]), (k, dirty.first_diff(a[k], b[k][:, 0]))
    for m, k in enumerate(STATES):
        assert same_bits(a[k], b["trajectory"][m]), k
    for k in TERMS:
        np.testing.assert_allclose(b[k][:, 0].cpu().numpy(), a[k].cpu().numpy(), rtol=REL, err_msg=k)
    np.testing.assert_allclose(b["step_cost"][:, 0].cpu().numpy(), a["rows"].cpu().numpy(), rtol=REL)
    eng.close()


def check_permutation(device):
    """12. Permuted candidates: ``best`` maps through the permutation (the gap of the case is asserted) and step 0's step_cost is
    permuted within REL (later steps start from states that differ by rounding)."""
    name = "steps"
    assert_gap(HC.restated(name), "permutation")
    eng = MVAEInference(PC.build(False, device), use_graph=False)
    cand = HC.request(name)[2]
    perm = torch.tensor([2, 0, 1])
    a, b = ask(eng, name, device), ask(eng, name, device, candidates=cand[perm].to(device))
    np.testing.assert_allclose(b["step_cost"][0].cpu().numpy(), a["step_cost"][0][perm].cpu().numpy(), rtol=REL)
    assert torch.equal(perm[b["best"].cpu().long()], a["best"].cpu().long())
    assert torch.equal(b["best_condition"], a["best_condition"])
    eng.close()


def check_mixed_request(device):
    """13. The mixed start (rollout_cases.START) with a per-step goal_available holding both values in every column: absent entries
    are 0 in the tables and left out of the cost; NaN planted in the absent goal rows reaches nothing."""
    B, N, T = RC.BATCH, 3, 2
    eng = MVAEInference(PC.build(False, device), use_graph=False)
    inputs, av = RC.start()
    goal = RC.frames(1402, T, B)
    gav = RC.mixed_table(8, T, B)
    assert all(0 < float(gav[:, :, m].sum()) < T * B for m in range(3))
    cand = torch.rand(N, T, CC.REAL_DIM, generator=torch.Generator().manual_seed(15))
    call = lambda g: cpu(keep(eng.plan_rollout(dev_list(inputs[:2], device), pose=inputs[2].to(device), steps=T, goal=dev_list(g, device),
                                               candidates=cand.to(device), available=av, goal_available=gav, **KW)))
    r = call(goal)
    on = gav != 0
    for m, k in enumerate(TERMS[:3]):
        assert float(r[k].transpose(1, 2)[~on[:, :, m]].abs().sum()) == 0.0 and float(r[k].transpose(1, 2)[on[:, :, m]].min()) > 0.0, k
    check_own_tables(r, None)
    dirty_goal = [g.clone() for g in goal]
    for m in range(3):
        dirty_goal[m][~on[:, :, m]] = float("nan")
    r2 = call(dirty_goal)
    for k in ("cost", "step_cost", "best", "best_cost") + TERMS:
        assert same_bits(r[k], r2[k]) and bool(torch.isfinite(r2[k].double()).all()), k
    # the start's availability reaches step 0: the oracle's forward of the rows' own modalities
    prm, buf = RC.oracle_state(eng.model)
    v, tc, pr, mu, lv = RC.oracle_step(prm, buf, inputs, torch.tensor(RC.START, dtype=torch.bool), torch.zeros(B, L),
                                       HC.candidate_rows(cand, B, False)[0, 1])
    np.testing.assert_allclose(r["means"][0, 1].numpy(), mu.numpy(), **OUT_TOL)
    eng.close()


def tree_batch(root, device):
    """The first loader batch of tests/synthetic_tree.py: n = 2 sequences of l = 3 frames with a 3-dim shock."""
    from mmdyn_hip.utils import datasets as D
    ST.build_tree(str(root))
    random.seed(7)
    out = D.dataset_setup(str(root), "seq_modeling", input_size=(64, 64), batchsize=2, shuffle=False, device=device)
    data, target = next(iter(out["train_loader"]))
    return [t.cpu() for t in data], [t.cpu() for t in target], out["seq_length"]


def check_problem_layer(device, root):
    """16. DynModeling.plan_rollout on a batch of the synthetic tree: default candidates = the batch's own recorded shock sequences
    (the row's own sequence is candidate b), ``recorded``, the engine beside it, the model's mode, the refusals."""
    data, target, l = tree_batch(root, device)
    n = data[0].shape[0] // l
    assert (n, l) == (2, 3) and tuple(data[4].shape) == (n * l, CC.REAL_DIM)
    model = PC.build(False, device)
    prob = TMM.problem_of(model, "cnn-mvae", True, device, DynModeling)
    prob._seq_length, prob._kl_weight, prob._pose_multiplier = l, HC.KL_WEIGHT, HC.POSE_MULTIPLIER
    model.train()
    res = prob.plan_rollout(data, target, top=2)
    assert model.training
    model.eval()
    assert set(res) == KEYS | {"top", "top_cost", "recorded"}
    rec = data[4].reshape(n, l, -1)
    assert tuple(res["recorded"].shape) == (n, l, CC.REAL_DIM) and torch.equal(res["recorded"].cpu(), rec)
    assert tuple(res["cost"].shape) == (n, n) and tuple(res["step_cost"].shape) == (l, n, n) and tuple(res["top"].shape) == (2, n)
    assert tuple(res["best_condition"].shape) == (n, l, CC.REAL_DIM)
    win = res["best"].cpu().long()
    assert int(win.min()) >= 0 and int(win.max()) < n and torch.equal(res["best_condition"].cpu(), rec[win])
    assert [tuple(t.shape) for t in res["trajectory"]] == [(l, n, 3, 64, 64), (l, n, 3, 64, 64), (l, n, 7)]
    # the engine beside it: the start is frame 0 of each sequence, the goal frames 1 .. l with the dataset's final target
    fr = lambda t: t.reshape((n, l) + tuple(t.shape[1:]))
    goal = [torch.cat((fr(data[m])[:, 1:].transpose(0, 1), target[m][l - 1::l].unsqueeze(0).to(data[m].dtype))).to(device) for m in range(3)]
    gav = torch.cat((torch.cat((fr(data[3])[:, 1:].transpose(0, 1).float(), torch.ones(1, n, 2))), torch.ones(l, n, 1)), 2)
    eng = MVAEInference(model, use_graph=False)
    want = eng.plan_rollout([data[0][::l].to(device), data[1][::l].to(device)], pose=data[2][::l].to(device), steps=l, goal=goal,
                            candidates=rec.to(device), available=data[3][::l].to(device), goal_available=gav, **KW)
    np.testing.assert_allclose(res["step_cost"].cpu().numpy(), want["step_cost"].cpu().numpy(), rtol=REL)
    on = gav != 0
    for m, k in enumerate(TERMS[:3]):
        assert float(res[k].cpu().transpose(1, 2)[~on[:, :, m]].abs().sum()) == 0.0, k
    eng.close()
    # fewer steps, the caller's own candidates and weights
    short = prob.plan_rollout(data, target, candidates=torch.rand(4, 2, CC.REAL_DIM), steps=2, step_weight=torch.tensor([0.5, 1.0]))
    assert tuple(short["cost"].shape) == (4, n) and tuple(short["recorded"].shape) == (n, 2, CC.REAL_DIM) and "top" not in short
    prob._horizon_planner.close()
    for bad in (0, l + 1, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            prob.plan_rollout(data, target, steps=bad)
    with pytest.raises(ValueError, match="shock"):
        prob.plan_rollout(data[:4], target)
    with pytest.raises(ValueError, match="whole sequences"):
        prob.plan_rollout([t[:-1] for t in data], target)
    with pytest.raises(ValueError):
        prob.plan_rollout(data[0], target[0])
    import avail_cases as A
    plain = TMM.problem_of(setup_model("cnn-mvae", cross_modal=True, **A.PLAIN_KW).to(device).eval(), "cnn-mvae", False, device, DynModeling)
    plain._seq_length = l
    with pytest.raises(ValueError, match="unconditional"):
        plain.plan_rollout(data, target)
    vae = TMM.problem_of(model, "cnn-vae", True, device, DynModeling)
    vae._seq_length = l
    with pytest.raises(ValueError, match="cnn-vae"):
        vae.plan_rollout(data, target)


# ---- the CPU suite ----------------------------------------------------------------------------------------------------------
def test_select_rules():
    check_select_rules(EmuBackendHorizon(), "cpu")


@pytest.mark.parametrize("B,N", [(1, 1), (5, 9), (300, 2)])
def test_one_scored_step_is_plan_select(B, N):
    check_one_step_is_plan_select(EmuBackendHorizon(), "cpu", B, N)


def test_total_is_not_contracted():
    check_total_is_not_contracted(EmuBackendHorizon(), "cpu")


@pytest.mark.parametrize("B,N,T", [(1, 1, 1), (5, 9, 3), (300, 2, 2)])
def test_select_against_the_restatement(B, N, T):
    check_select_restatement(EmuBackendHorizon(), "cpu", B, N, T)


@pytest.mark.parametrize("row_lens,B,N,T,shift", [((48, 48, 7), 5, 3, 3, 0), ((12288, 12288, 7), 2, 2, 2, 0), ((12, 12), 3, 3, 2, 1)])
def test_gather_steps_is_gather_best_per_step(row_lens, B, N, T, shift):
    check_gather_steps(EmuBackendHorizon(), "cpu", row_lens, B, N, T, shift)


@pytest.mark.parametrize("name,sample", [("steps", True), ("final", False), ("classes", False), ("nine", False)])
def test_one_step_consistency(name, sample):
    check_one_step_consistency("cpu", name, sample)


@pytest.mark.parametrize("name", list(HC.CASES))
def test_choice_against_the_chained_oracle(name):
    check_choice("cpu", name)


@pytest.mark.parametrize("sample", [False, True])
def test_one_step_is_plan(sample):
    check_one_step_is_plan("cpu", sample)


def test_one_candidate_is_rollout():
    check_one_candidate_is_rollout("cpu")


def test_permuted_candidates():
    check_permutation("cpu")


def test_mixed_request_and_absent_goal_terms():
    check_mixed_request("cpu")


def test_problem_layer(tmp_path):
    check_problem_layer("cpu", tmp_path)


# ---- emulation only ---------------------------------------------------------------------------------------------------------
def test_hip_backend_validates_on_the_host():
    """HipBackend.plan_select_steps / gather_best_steps check shapes and dtypes before they touch the library, and refuse CPU
    tensors."""
    hip = ops.HipBackend()
    N, B, T, cd = 2, 3, 2, 3
    f = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    d = lambda *s: f(*s, dtype=torch.float64)
    i32 = torch.int32
    sel = lambda **k: dict(dict(bce_rows=d(2, T, N, B), mse_rows=d(T, N, B), kl_rows=d(T, N, B), tavail=None, step_weight=f(T),
                                candidates=f(T, N * B, cd), cost=f(N, B), step_cost=f(T, N, B), best=f(B, dtype=i32), best_cost=f(B),
                                best_condition=f(B, T, cd), top=None, top_cost=None, N=N, B=B, T=T, Tg=T, pose_multiplier=1.0), **k)
    for k in (sel(bce_rows=d(2, N, B)), sel(mse_rows=f(T, N, B)), sel(kl_rows=d(T, B, N)), sel(kl_rows=None), sel(candidates=f(N * B, cd)),
              sel(candidates=f(T, N * B + 1, cd)), sel(candidates=f(T, N * B, dtype=torch.int64)), sel(best=f(B, dtype=torch.int64)),
              sel(cost=f(B, N)), sel(step_cost=f(N, B)), sel(best_condition=f(B, cd)), sel(N=0), sel(T=0), sel(Tg=3), sel(step_weight=f(T + 1)),
              sel(step_weight=d(T)), sel(tavail=torch.ones(T, B, 3, dtype=torch.uint8)), sel(tavail=torch.ones(B, 4, dtype=torch.uint8)),
              sel(top=f(2, B, dtype=i32)), sel(top=f(9, B, dtype=i32), top_cost=f(9, B)), sel(top=f(2, B, dtype=i32), top_cost=f(3, B)),
              sel(top=f(2, B), top_cost=f(2, B))):
        with pytest.raises(ValueError):
            hip.plan_select_steps(**k)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.plan_select_steps(**sel())
    grp = lambda **k: dict(dict(src=f(T, N * B, 7), out=f(T, B, 7), logits=False), **k)
    best = f(B, dtype=i32)
    for groups, bst, n, t in (([], best, N, T), ([grp()] * 5, best, N, T), ([grp(out=f(T, B, 8))], best, N, T),
                              ([grp(src=f(T, N * B + 1, 7))], best, N, T), ([grp(src=d(T, N * B, 7))], best, N, T),
                              ([grp(out=f(T, B, 14)[:, :, ::2])], best, N, T), ([grp()], best.long(), N, T),
                              ([grp()], f(B + 1, dtype=i32), N, T), ([grp()], best, 0, T), ([grp()], best, N, 0), ([grp()], best, N, T + 1),
                              ([grp(src=f(N * B, 7), out=f(B, 7))], best, N, T), ([grp(src=f(T, N * B, 0), out=f(T, B, 0))], best, N, T)):
        with pytest.raises(ValueError):
            hip.gather_best_steps(groups, bst, n, B, t)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.gather_best_steps([grp()], best, N, B, T)


def request_kw(N, T, every, seed=5):
    inputs, _ = RC.start()
    goal = RC.frames(1500 + seed, T if every else 1, RC.BATCH)
    cand = torch.rand(N, T, CC.REAL_DIM, generator=torch.Generator().manual_seed(N + T))
    return dict(x=inputs[:2], pose=inputs[2], steps=T, goal=goal if every else [g[0] for g in goal], candidates=cand, **KW)


def recorded(fn):
    rec = ShapeRecorder(EmuBackendHorizon())
    old = ops.set_backend(rec)
    eng = MVAEInference(PC.build(False), use_graph=False)
    del rec.ops[:], rec.sigs[:]                                         # (the weights are packed when the engine is built)
    try:
        fn(eng)
    finally:
        ops.set_backend(old)
        eng.close()
    quiet = ("random_normal", "counter_add")
    return [o for o in rec.ops if o not in quiet], [s for s in rec.sigs if s[0] not in quiet]


def test_launch_accounting():
    """17. The recorded calls, by name and by the shapes they are handed, against the schedule: step 0 = the calls of plan() up to
    its decoders (nothing in front of the heads scales with N), every later step = the calls of forward() on N * B rows, each step
    closed by one rollout_feed; a scored step adds the row kernels (one launch per goal term and 8 candidates) and kl_rows, an
    unscored step nothing; the request ends in one plan_select_steps and one gather_best_steps, and no plan_select, gather_best,
    assembly or complete_select launch is issued."""
    B = RC.BATCH
    terms = ["bce_logits_rows_groups", "bce_logits_rows_groups", "mse_rows_groups"]
    close = ["plan_select_steps", "gather_best_steps"]
    for N in (1, 8, 9):
        kw1 = request_kw(N, 1, False)
        plan_ops, plan_sigs = recorded(lambda e: e.plan(kw1["x"], pose=kw1["pose"], goal=kw1["goal"], candidates=kw1["candidates"][:, 0], **KW))
        cut = plan_ops.index("bce_logits_rows_groups")
        front, front_sigs = plan_ops[:cut], plan_sigs[:cut]                   # plan() up to and including its decoders
        assert plan_ops[cut:] == terms * (1 + (N > 8)) + ["kl_rows", "plan_select", "gather_best"]
        cond = kw1["candidates"][:, 0].repeat_interleave(B, 0)                # N * B condition rows
        big = lambda t: t.repeat((N,) + (1,) * (t.dim() - 1))
        fwd_ops, fwd_sigs = recorded(lambda e: e.forward([big(kw1["x"][0]), big(kw1["x"][1])], pose=big(kw1["pose"]), condition=cond))
        scored = terms * (1 + (N > 8)) + ["kl_rows"]
        for T in (1, 3):
            for every in (False, True):
                kw = request_kw(N, T, every)
                got, sigs = recorded(lambda e: e.plan_rollout(**kw))
                want, want_sigs = [], []
                for t in range(T):
                    want += front if t == 0 else fwd_ops
                    want_sigs += front_sigs if t == 0 else fwd_sigs
                    if every or t == T - 1:
                        want += scored
                        want_sigs += [None] * len(scored)
                    want += ["rollout_feed"]
                    want_sigs += [None]
                assert got == want + close, (N, T, every, got)
                for g, w in zip(sigs, want_sigs):
                    assert w is None or g == w, (N, T, every, g, w)
                feeds = [s for s in sigs if s[0] == "rollout_feed"]
                assert all(s[1][0] == (N * B, 3, 64, 64) for s in feeds) and len(feeds) == T
                assert not {"plan_select", "gather_best", "complete_select"} & set(got) and not any(o.startswith("elbo_assemble") for o in got)
    # nothing in front of step 0's heads scales with N: the recorded shapes up to the first tiled join are those of N = 1
    heads = lambda N: recorded(lambda e: e.plan_rollout(**request_kw(N, 2, True)))[1]
    one, nine = heads(1), heads(9)
    first = [s[0] for s in one].index("concat_condition_tiled")
    assert one[:first] == nine[:first] and first > 5
    # plan and rollout record what they record without the new ops in the backend
    kw = request_kw(3, 2, True)
    for call in (lambda e: e.plan(kw["x"], pose=kw["pose"], goal=[g[0] for g in kw["goal"]], candidates=kw["candidates"][:, 0], **KW),
                 lambda e: e.rollout(kw["x"], pose=kw["pose"], steps=2, condition=kw["candidates"][0, 0].expand(B, -1).contiguous(),
                                     targets=kw["goal"], **KW)):
        now = recorded(call)
        rec = ShapeRecorder(EmuBackendPlan())
        old = ops.set_backend(rec)
        eng = MVAEInference(PC.build(False), use_graph=False)
        del rec.ops[:]
        call(eng)
        ops.set_backend(old)
        eng.close()
        assert now[0] == [o for o in rec.ops if o not in ("random_normal", "counter_add")]
        assert "plan_select_steps" not in now[0] and "gather_best_steps" not in now[0]


def test_posterior_mean_draws_nothing_and_a_row_shares_one_draw_per_step():
    kw = request_kw(3, 2, True)
    eng = MVAEInference(PC.build(False), use_graph=False)
    eng.noise = InjectedNoise([], [])                                   # a draw would pop from an empty list
    mean = keep(eng.plan_rollout(**kw))
    eng.noise = InjectedNoise([torch.zeros(RC.BATCH, L) for _ in range(2)], [])
    zero = eng.plan_rollout(**kw, sample=True)
    assert all(torch.equal(mean[k], zero[k]) for k in ("cost", "best", "means", "kl"))
    assert not eng.noise._eps                                           # exactly T blocks of [B, L] were taken
    eng.close()


def test_argument_errors_and_graph_keys():
    """18. The refusals, and what the graph key carries: N, T, the kind, the goal's form, ``top`` and ``sample`` -- never values."""
    eng = MVAEInference(PC.build(False), use_graph=False)
    kw = request_kw(3, 2, True)
    B, T, cd = RC.BATCH, 2, CC.REAL_DIM
    bad = lambda **k: dict(kw, **k)
    for c in (None, torch.zeros(0, T, cd), torch.zeros(2, T, cd + 1), torch.zeros(2, T + 1, cd), torch.zeros(2, T, cd, dtype=torch.int64),
              torch.zeros(T, cd), torch.zeros(B + 1, 2, T, cd), torch.zeros(2, 2, 2, T, cd), [[[0.0] * cd] * T]):
        with pytest.raises(ValueError, match="candidate"):
            eng.plan_rollout(**bad(candidates=c))
    v, t, p = kw["goal"]
    for g in (None, [None, None, None], [v[:, :2], None, None], [None, None, p[:, :, :6]], v, [v[:1], None, None], [v[0, 0], None, None]):
        with pytest.raises(ValueError, match="goal"):
            eng.plan_rollout(**bad(goal=g))
    with pytest.raises(ValueError, match="mixes the two forms"):
        eng.plan_rollout(**bad(goal=[v, t[0], None]))
    with pytest.raises(ValueError, match="mixes the two forms"):
        eng.plan_rollout(**bad(goal=[v[0], None, p]))
    for s in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="steps"):
            eng.plan_rollout(**bad(steps=s))
    for k in (0, 9, 1.5, True):
        with pytest.raises(ValueError, match="top"):
            eng.plan_rollout(**bad(top=k))
    for w in (torch.ones(T + 1), torch.ones(T, 1), [1.0, 1.0], torch.ones(T, dtype=torch.int64)):
        with pytest.raises(ValueError, match="step_weight"):
            eng.plan_rollout(**bad(step_weight=w))
    with pytest.raises(ValueError, match="step_weight"):
        eng.plan_rollout(**bad(goal=[v[0], None, None], step_weight=torch.ones(T)))         # a final goal: Tg = 1
    with pytest.raises(ValueError, match="goal_available"):
        eng.plan_rollout(**bad(goal_available=torch.ones(B, 3)))                            # per-step goals want [T, B, .]
    with pytest.raises(ValueError):
        eng.plan_rollout(**bad(goal=[v[0], None, None], goal_available=torch.ones(T, B, 3)))
    with pytest.raises(ValueError, match="modality"):
        eng.plan_rollout(**bad(x=[None, None], pose=None))
    most = min((2 ** 31 - 1) // (T * B * 3 * 64 * 64), (2 ** 31 - 1) // (B * 32 * 32 * 32))
    with pytest.raises(ValueError, match=rf"largest N for B = {B} and steps = {T} is {most}\b"):
        eng.plan_rollout(**bad(candidates=torch.zeros(most + 1, T, cd)))
    # NaN / Inf weights are not looked at: they propagate
    r = eng.plan_rollout(**bad(step_weight=torch.tensor([float("nan"), 1.0])))
    assert r["best"].tolist() == [-1] * B and bool(torch.isnan(r["cost"]).all()) and bool(torch.isfinite(r["step_cost"]).all())
    assert bool(torch.isnan(r["trajectory"][0]).all()) and bool(torch.isnan(r["best_condition"]).all())
    # a backend written before the ops: an error that names one of them, before anything is launched
    ops.set_backend(EmuBackendPlan())
    with pytest.raises(RuntimeError, match="plan_select_steps"):
        eng.plan_rollout(**kw)
    ops.set_backend(EmuBackendHorizon())
    eng.close()
    cat = MVAEInference(PC.build(True), use_graph=False)
    for c in (torch.zeros(2, T), torch.zeros(B + 1, 2, T, dtype=torch.int64), torch.zeros(0, T, dtype=torch.int64),
              torch.zeros(2, T + 1, dtype=torch.int64), torch.zeros(2, 2, 2, T, dtype=torch.int64), torch.zeros(T, dtype=torch.int64)):
        with pytest.raises(ValueError, match="candidate"):
            cat.plan_rollout(**bad(candidates=c))
    r = cat.plan_rollout(**bad(candidates=torch.tensor([[1, CC.CAT_DIM], [0, 2]], dtype=torch.int32)))      # bad_condition covers the call
    assert cat.bad_condition() and r["best_condition"].dtype == torch.int64 and tuple(r["best_condition"].shape) == (B, T)
    cat.plan_rollout(**bad(candidates=torch.tensor([[[1, 2]], [[0, 4]], [[3, 3]]], dtype=torch.uint8)))     # per row: [B, N = 1, T]
    assert not cat.bad_condition()
    cat.close()
    import avail_cases as A
    plain = MVAEInference(setup_model("cnn-mvae", cross_modal=True, **A.PLAIN_KW).eval(), use_graph=False)
    with pytest.raises(ValueError, match="unconditional model"):
        plain.plan_rollout(**kw)
    plain.close()
    # graph keys (recorded by a stand-in for _run: the key is formed before anything is captured)
    eng = MVAEInference(PC.build(False), use_graph=False)
    keys = []
    eng._run = lambda key, fn, args: keys.append(key)
    w = torch.tensor([1.0, 2.0])
    calls = [kw, bad(candidates=kw["candidates"] + 1.0), bad(kl_weight=2.0),                                   # values: the same key
             bad(step_weight=w), bad(step_weight=w * 3.0),                                                     # ... and again
             bad(candidates=torch.rand(4, T, cd)), bad(steps=3, candidates=torch.rand(3, 3, cd), goal=RC.frames(1, 3, B)),
             bad(goal=[g[1] for g in kw["goal"]]), bad(top=2), bad(top=3), bad(sample=True),
             bad(candidates=torch.rand(B, 3, T, cd)), bad(pose_multiplier=10.0)]
    for c in calls:
        eng.plan_rollout(**c)
    assert keys[0] == keys[1] == keys[2] and keys[3] == keys[4] != keys[0]
    assert len(set(keys)) == len(calls) - 3
    assert all(k[0] == "plan_rollout" for k in keys)
