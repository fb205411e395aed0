"""Candidate conditions on the CPU: ``MVAEInference.plan`` through the emulation backend (tests/emu_backend_plan.py) against the
restatement on the oracle (tests/plan_cases.py: one eval-mode forward per (candidate, row), the fp64 terms against the goal, the
argmin), against N separate ``score(condition=c_n)`` requests, the selection rules of ``plan_select`` on integer-valued tables, the
launch accounting, the error paths and ``DynModeling.plan``.  The ``check_*`` functions take the device (and the backend):
tests/test_plan_gpu.py runs them on the HIP library."""
import numpy as np
import pytest
import torch

import cond_cases as CC
import plan_cases as PC
import rollout_cases as RC
import test_mixed_modal_emu as TMM
from emu_backend_iw import Recorder
from emu_backend_plan import EmuBackendPlan
from emu_backend_rollout import EmuBackendRollout
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise, setup_model
from mmdyn_hip.models.functional import availability_table
from mmdyn_hip.problems.problems import DynModeling
from test_elbo_rows_emu import REL          # engine rows against the oracle, and K * B rows against B rows (the IW suite's bound)

OUT_TOL = TMM.OUT_TOL
L = PC.L
KW = dict(kl_weight=PC.KL_WEIGHT, pose_multiplier=PC.POSE_MULTIPLIER)
TERMS = ("bce_visual", "bce_tactile", "mse_pose", "kl")
KEYS = {"cost", "best", "best_cost", "best_condition", "prediction", "means", "log_var", "recon_x"} | set(TERMS)
GAP = 10 * REL                              # the restatement's best-to-runner-up gap, relative to the best cost, that pins ``best``


@pytest.fixture(autouse=True)
def emu_plan():
    old = ops.set_backend(EmuBackendPlan())
    yield
    ops.set_backend(old)


def dev_list(ts, device):
    return None if ts is None else [None if t is None else t.to(device) for t in ts]


def keep(r):
    cl = lambda v: None if v is None else ([cl(t) for t in v] if isinstance(v, (list, tuple)) else v.detach().clone())
    return {k: cl(v) for k, v in r.items()}


def mixed_tables():
    return dict(available=torch.tensor(RC.START, dtype=torch.float64), goal_available=torch.tensor(PC.GOAL_ON, dtype=torch.float64))


def ask(eng, name, device, eps=None, cand="case", **kw):
    """One plan() call of a case; ``eps``: the [B, L] draw to inject (sample=True), None: the posterior means."""
    inputs, goal, c, _ = PC.request(name)
    inputs, goal = dev_list(inputs, device), dev_list(goal, device)
    if isinstance(cand, str):
        cand = c
    if eps is not None:
        eng.noise = InjectedNoise([eps.clone()], [])
    return keep(eng.plan([inputs[0], inputs[1]], pose=inputs[2], goal=goal, candidates=None if cand is None else cand.to(device),
                         sample=eps is not None, **dict(KW, **kw)))


def assert_gap(want, what):
    """The choice is only pinned where the restatement itself separates the best candidate from the runner-up by ten times the
    tolerance of the cost comparison: asserted for every row, no row is skipped."""
    g, low = PC.gap(want["cost"]), want["cost"].min(0).values.abs()
    print(what, "gap / |best cost| per row", (g / low).tolist(), "needed", GAP)
    assert bool((g >= GAP * low).all()), (what, g, low)


def check_against_oracle(device, name, sample, mixed=False, sigmoid_atol=0.0):
    """The tables, the cost and the posterior of every (candidate, row) against the restatement (REL / OUT_TOL, the constants of
    the rows and IW suites); ``best`` = the restatement's argmin under the gap condition; the winner's cost, condition and
    prediction are the winner's entries; an absent (row, term) is 0 in the table."""
    B, N, categorical, per_row = PC.CASES[name]
    want = PC.restated(name, sample, mixed)
    assert_gap(want, f"{name} sample={sample} mixed={mixed}")
    eng = MVAEInference(PC.build(categorical, device), use_graph=False)
    inputs, goal, cand, eps = PC.request(name)
    r = ask(eng, name, device, eps if sample else None, **(mixed_tables() if mixed else {}))
    r = {k: (v if not torch.is_tensor(v) else v.cpu()) for k, v in r.items()}
    assert set(r) == KEYS
    assert tuple(r["cost"].shape) == (N, B) and r["cost"].dtype == torch.float32
    assert tuple(r["best"].shape) == (B,) and r["best"].dtype == torch.int32
    assert tuple(r["best_cost"].shape) == (B,) and r["best_cost"].dtype == torch.float32
    assert tuple(r["means"].shape) == (N, B, L) == tuple(r["log_var"].shape)
    assert tuple(r["recon_x"][0].shape) == (N * B, 3, 64, 64) and tuple(r["recon_x"][2].shape) == (N * B, 7)
    for k in TERMS:
        assert tuple(r[k].shape) == (N, B) and r[k].dtype == torch.float64, k
        got, ref = r[k].numpy(), want[k].numpy()
        print(name, k, "largest relative deviation", float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))))
        np.testing.assert_allclose(got, ref, rtol=REL, err_msg=k)
    np.testing.assert_allclose(r["means"].numpy(), want["means"].numpy(), **OUT_TOL)
    np.testing.assert_allclose(r["log_var"].numpy(), want["log_var"].numpy(), **OUT_TOL)
    np.testing.assert_allclose(r["cost"].double().numpy(), want["cost"].numpy(), rtol=REL)
    assert torch.equal(r["best"].long(), want["best"]), (r["best"], want["best"], r["cost"], want["cost"])
    rows = torch.arange(B)
    win = r["best"].long()
    assert torch.equal(r["best_cost"], r["cost"][win, rows])
    rows_of = PC.candidate_rows(name, cand)                                     # [N][B][cd]
    if categorical:
        assert r["best_condition"].dtype == torch.int64 and torch.equal(r["best_condition"].cpu(), win)      # all classes: n is the class
    else:
        assert torch.equal(r["best_condition"].cpu(), rows_of[win, rows])
    for m, (k, logits) in enumerate((("visual", True), ("tactile", True), ("pose", False))):
        p, ref = r["prediction"][m].cpu(), want[k][win, rows]
        assert tuple(p.shape) == tuple(ref.shape)
        if logits:      # a sigmoid divides an error of its argument by at least 4 (the bound of the rollout suite's slots)
            np.testing.assert_allclose(p.numpy(), torch.sigmoid(ref).numpy(), rtol=OUT_TOL["rtol"], atol=OUT_TOL["atol"] / 4 + sigmoid_atol)
        else:
            np.testing.assert_allclose(p.numpy(), ref.numpy(), **OUT_TOL)
    if mixed:
        gon = torch.tensor(PC.GOAL_ON, dtype=torch.bool)
        for m, k in enumerate(TERMS[:3]):
            assert float(r[k][:, ~gon[:, m]].abs().sum()) == 0.0 and float(r[k][:, gon[:, m]].min()) > 0.0, k
    eng.close()
    return r


def condition_of(name, cand, n, B):
    """The condition score() takes for candidate n of a case."""
    _, N, categorical, per_row = PC.CASES[name]
    if categorical:
        return torch.full((B,), n, dtype=torch.int64)
    return cand[:, n] if per_row else cand[n].unsqueeze(0).expand(B, -1).contiguous()


def check_against_separate_requests(device, name, sigmoid_atol=0.0):
    """plan(sample=True) with the draw injected against N separate score(condition=c_n) requests with the same draw: the terms
    within REL (N * B rows against B rows: the IW suite's bound for K * B against B), the posterior and the logits within OUT_TOL.
    N = 1: best is 0 and the prediction is the sigmoid of that request's logits."""
    B, N, categorical, per_row = PC.CASES[name]
    eng = MVAEInference(PC.build(categorical, device), use_graph=False)
    inputs, goal, cand, eps = PC.request(name)
    r = ask(eng, name, device, eps)
    x, g = dev_list(inputs, device), dev_list(goal, device)
    for n in range(N):
        eng.noise = InjectedNoise([eps.clone()], [])
        one = eng.score([x[0], x[1]], pose=x[2], targets=g, condition=condition_of(name, cand, n, B).to(device), **KW)
        for k in TERMS:
            np.testing.assert_allclose(r[k][n].cpu().numpy(), one[k].cpu().numpy(), rtol=REL, err_msg=f"{k} candidate {n}")
        np.testing.assert_allclose(r["cost"][n].cpu().numpy(), one["rows"].cpu().numpy(), rtol=REL, err_msg=f"cost candidate {n}")
        np.testing.assert_allclose(r["means"][n].cpu().numpy(), one["means"].cpu().numpy(), **OUT_TOL)
        np.testing.assert_allclose(r["log_var"][n].cpu().numpy(), one["log_var"].cpu().numpy(), **OUT_TOL)
        for m in range(3):
            np.testing.assert_allclose(r["recon_x"][m][n * B:(n + 1) * B].cpu().numpy(), one["recon_x"][m].cpu().numpy(), **OUT_TOL)
        if N == 1:
            assert r["best"].tolist() == [0] * B
            for m in range(2):
                np.testing.assert_allclose(r["prediction"][m].cpu().numpy(), torch.sigmoid(one["recon_x"][m]).cpu().numpy(),
                                           rtol=OUT_TOL["rtol"], atol=OUT_TOL["atol"] / 4 + sigmoid_atol)
            np.testing.assert_allclose(r["prediction"][2].cpu().numpy(), one["recon_x"][2].cpu().numpy(), **OUT_TOL)
    eng.close()


def check_permutation(device):
    """Permuted candidates: the cost table is permuted (REL) and ``best`` maps through the permutation (the gap condition of the
    case is asserted by check_against_oracle's restatement)."""
    name = "shared"
    B, N, categorical, _ = PC.CASES[name]
    assert_gap(PC.restated(name, False), "permutation")
    eng = MVAEInference(PC.build(categorical, device), use_graph=False)
    cand = PC.request(name)[2]
    perm = torch.tensor([2, 0, 1])
    a, b = ask(eng, name, device), ask(eng, name, device, cand=cand[perm])
    np.testing.assert_allclose(b["cost"].cpu().numpy(), a["cost"][perm].cpu().numpy(), rtol=REL)
    assert torch.equal(perm[b["best"].cpu().long()], a["best"].cpu().long())
    assert torch.equal(b["best_condition"], a["best_condition"])
    eng.close()


# ---- plan_select: the rules on integer-valued tables (exact in any summation order), then random tables ----------------------
def run_select(backend, device, bce, mse, kl, table, cand, pm, klw=1.0, klw_dev=None):
    N, B = kl.shape
    mv = lambda t: None if t is None else t.clone().to(device)
    bce, mse, kl, cand = mv(bce), mv(mse), mv(kl), mv(cand)
    tab = None if table is None else availability_table(table, B, device)
    cost, best = torch.full((N, B), 7.0, device=device), torch.full((B,), 77, dtype=torch.int32, device=device)
    best_cost = torch.full((B,), 7.0, device=device)
    best_cond = torch.full((B,) + tuple(cand.shape[1:]), 7, dtype=cand.dtype, device=device)
    backend.plan_select(bce, mse, kl, tab, cand, cost, best, best_cost, best_cond, N, B, pm, klw,
                        None if klw_dev is None else torch.tensor([klw_dev], device=device))
    return dict(cost=cost.cpu(), best=best.cpu(), best_cost=best_cost.cpu(), best_cond=best_cond.cpu(),
                bce=None if bce is None else bce.cpu(), mse=None if mse is None else mse.cpu())


def check_select_rules(backend, device):
    nan, inf = float("nan"), float("inf")
    f64 = torch.float64
    N, B = 4, 6
    # rows: an exact tie (candidates 1 and 3), a NaN that would win, all NaN, +inf against finite, -inf wins, a plain row
    tot = torch.tensor([[5, 2, 9, 2], [3, nan, 1, 4], [nan, nan, nan, nan], [inf, inf, 8, inf], [1, -inf, 0, 2], [4, 3, 2, 1]], dtype=f64).t()
    kl = torch.zeros(N, B, dtype=f64)
    bce = torch.stack((tot.clone(), torch.zeros(N, B, dtype=f64)))
    cand = (torch.arange(N * B * 2, dtype=torch.float32).reshape(N * B, 2) + 1.0)
    r = run_select(backend, device, bce, None, kl, None, cand, 1000.0)
    assert r["best"].tolist() == [1, 2, -1, 2, 1, 3]
    want_cost = torch.tensor([2.0, 1.0, nan, 8.0, -inf, 1.0])
    assert torch.equal(torch.nan_to_num(r["best_cost"], nan=-7.0), torch.nan_to_num(want_cost, nan=-7.0))
    assert torch.equal(torch.nan_to_num(r["cost"], nan=-7.0), torch.nan_to_num(tot.float(), nan=-7.0))
    for b, w in enumerate(r["best"].tolist()):
        assert bool(torch.isnan(r["best_cond"][b]).all()) if w < 0 else torch.equal(r["best_cond"][b], cand[w * B + b])
    # class indices as candidates: the winner's index, -1 where every cost is NaN
    idx = (torch.arange(N * B) % 5).to(torch.int64)
    r = run_select(backend, device, bce, None, kl, None, idx, 1000.0)
    assert r["best_cond"].tolist() == [int(idx[w * B + b]) if w >= 0 else -1 for b, w in enumerate(r["best"].tolist())]
    # every term with integer values, pose_multiplier 4, the KL weight 3 taken from the device pointer (times the argument 1)
    g = torch.Generator().manual_seed(3)
    ri = lambda *s: torch.randint(0, 50, s, generator=g).to(f64)
    bce, mse, kl = ri(2, N, B), ri(N, B), ri(N, B)
    on = torch.tensor([[1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0], [0, 0, 0], [1, 1, 1]], dtype=torch.bool)
    bce[0][:, 1], mse[:, 3] = nan, inf                      # absent entries may hold anything: they are left out and become 0
    r = run_select(backend, device, bce, mse, kl, on.to(f64), cand, 4.0, 1.0, klw_dev=3.0)
    z = torch.zeros(N, B, dtype=f64)
    pick = lambda t, m: torch.where(on[:, m].unsqueeze(0), t, z)
    want = pick(bce[0], 0) + pick(bce[1], 1) + 4.0 * pick(mse, 2) + 3.0 * kl
    assert torch.equal(r["cost"], want.float()) and torch.equal(r["best"].long(), torch.argmin(want, 0))      # (seed 3: no ties)
    assert all(len(set(want[:, b].tolist())) == N for b in range(B))
    assert torch.equal(r["bce"][0], pick(bce[0], 0)) and torch.equal(r["bce"][1], pick(bce[1], 1)) and torch.equal(r["mse"], pick(mse, 2))
    # without the pointer the argument alone is the weight
    r2 = run_select(backend, device, bce, mse, kl, on.to(f64), cand, 4.0, 3.0)
    assert torch.equal(r2["cost"], r["cost"]) and torch.equal(r2["best"], r["best"])


def check_select_no_contraction(backend, device):
    """The cost is the WRITTEN order -- each product rounded before it is added -- not a fused multiply-add.  Two candidates per
    row whose written-order fp64 costs tie exactly at 1.0, so candidate 0 must win; with pm * mse (row 0) or klw * kl (row 1) fused
    into the sum, candidate 1 would come out at 1 - 2^-52 and win.  The premise is asserted in exact rational arithmetic."""
    from fractions import Fraction
    f64 = torch.float64
    w = 3.0                                                     # the multiplier: pose_multiplier in row 0, the KL weight in row 1
    m1 = 1.0 + 2.0 ** -52                                       # 3 * m1 = 3 + 3 * 2^-52 is no double: it rounds to 3 + 2^-50
    p1 = w * m1
    assert Fraction(p1) - Fraction(w) * Fraction(m1) == Fraction(1, 2 ** 52)
    v0, v1 = 1.0 - w * 1.0, 1.0 - p1                            # both exact
    assert v0 + w * 1.0 == 1.0 == v1 + p1                       # the written order: a tie
    fused = float(Fraction(v1) + Fraction(w) * Fraction(m1))    # one rounding of the exact sum
    assert fused == 1.0 - 2.0 ** -52 and fused < 1.0            # ... which the fused form would break in favour of candidate 1
    N, B = 2, 2
    bce = torch.zeros(2, N, B, dtype=f64)
    bce[0] = torch.tensor([[v0, v0], [v1, v1]], dtype=f64)
    mse = torch.tensor([[1.0, 0.0], [m1, 0.0]], dtype=f64)
    kl = torch.tensor([[0.0, 1.0], [0.0, m1]], dtype=f64)
    cand = torch.arange(N * B * 2, dtype=torch.float32).reshape(N * B, 2)
    r = run_select(backend, device, bce, mse, kl, None, cand, w, 1.0, klw_dev=w)
    assert r["best"].tolist() == [0, 0], r["best"]
    assert r["cost"].tolist() == [[1.0, 1.0], [1.0, 1.0]] and r["best_cost"].tolist() == [1.0, 1.0]
    # the mirror image: the exact sum lies ABOVE the tie (m1 = 1 + 3 * 2^-52: 3 * m1 = 3 + 9 * 2^-52 rounds down to 3 + 2^-49)
    m2 = 1.0 + 3.0 * 2.0 ** -52
    p2 = w * m2
    assert Fraction(w) * Fraction(m2) - Fraction(p2) == Fraction(1, 2 ** 52)
    u0, u1 = 1.0 - p2, 1.0 - w * 1.0
    assert u0 + p2 == 1.0 == u1 + w * 1.0 and float(Fraction(u0) + Fraction(w) * Fraction(m2)) > 1.0
    bce[0] = torch.tensor([[u0, u0], [u1, u1]], dtype=f64)      # fused: candidate 0 costs more than 1.0 and candidate 1 would win
    mse, kl = torch.tensor([[m2, 0.0], [1.0, 0.0]], dtype=f64), torch.tensor([[0.0, m2], [0.0, 1.0]], dtype=f64)
    r = run_select(backend, device, bce, mse, kl, None, cand, w, 1.0, klw_dev=w)
    assert r["best"].tolist() == [0, 0], r["best"]


def check_select_restatement(backend, device, B, N):
    """Random tables: ``cost`` is the fp32 rounding of the fp64 restatement in the same written order, exactly; ``best`` its
    argmin (every row's gap is at least 1e-9 relative: asserted, no row skipped); two runs give the same bits."""
    bce, mse, kl = PC.random_tables(B, N, 40 + B + N)
    on = torch.rand(B, 3, generator=torch.Generator().manual_seed(B)) < 0.8
    cand = torch.rand(N * B, 3, generator=torch.Generator().manual_seed(N))
    c, c32, best = PC.select_ref(bce, mse, kl, on, PC.POSE_MULTIPLIER, np.float32(PC.KL_WEIGHT))
    g = PC.gap(c)
    assert bool((g >= 1e-9 * c.min(0).values.abs()).all())
    runs = [run_select(backend, device, bce, mse, kl, on.to(torch.float64), cand, PC.POSE_MULTIPLIER, 1.0, klw_dev=PC.KL_WEIGHT)
            for _ in range(2)]
    r = runs[0]
    assert torch.equal(r["cost"], c32) and torch.equal(r["best"], best)
    assert torch.equal(r["best_cost"], c32[best.long(), torch.arange(B)])
    assert torch.equal(r["best_cond"], cand[best.long() * B + torch.arange(B)])
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in ("cost", "best", "best_cost", "best_cond"))


# ---- the CPU suite ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sample", [("classes", False), ("shared", True), ("per_row", False), ("one", True)])
def test_plan_against_the_oracle(name, sample):
    check_against_oracle("cpu", name, sample)


def test_mixed_request_and_absent_goal_terms():
    check_against_oracle("cpu", "shared", True, mixed=True)


@pytest.mark.parametrize("name", ["classes", "per_row", "one"])
def test_plan_against_separate_requests(name):
    check_against_separate_requests("cpu", name)


def test_permuted_candidates():
    check_permutation("cpu")


def test_select_rules():
    check_select_rules(EmuBackendPlan(), "cpu")


def test_select_cost_is_not_contracted():
    check_select_no_contraction(EmuBackendPlan(), "cpu")


@pytest.mark.parametrize("B,N", [(1, 1), (5, 9), (300, 2)])
def test_select_against_the_restatement(B, N):
    check_select_restatement(EmuBackendPlan(), "cpu", B, N)


def test_posterior_mean_plan_draws_nothing_and_shares_one_draw():
    """sample=False touches no noise; sample=True takes ONE [B, L] block, shared by the N candidates of a row."""
    name = "shared"
    B, N, categorical, _ = PC.CASES[name]
    eng = MVAEInference(PC.build(categorical), use_graph=False)
    eng.noise = InjectedNoise([], [])                                   # a draw would pop from an empty list
    mean = ask(eng, name, "cpu")
    eng.noise = InjectedNoise([torch.zeros(B, L)], [])
    zero = eng.plan(**plan_kw(name), sample=True)
    assert all(torch.equal(mean[k], zero[k]) for k in ("cost", "best", "means", "kl"))
    assert not eng.noise._eps                                           # exactly one block was taken
    eng.close()


def plan_kw(name, N=None):
    inputs, goal, cand, _ = PC.request(name)
    if N is not None:
        cand = torch.rand(N, CC.REAL_DIM, generator=torch.Generator().manual_seed(N))
    return dict(x=[inputs[0], inputs[1]], pose=inputs[2], goal=goal, candidates=cand, **KW)


def recorded(N):
    rec = Recorder(EmuBackendPlan())
    ops.set_backend(rec)
    eng = MVAEInference(PC.build(False), use_graph=False)
    kw = plan_kw("shared", N)
    del rec.ops[:]
    eng.plan(**kw)
    plan = list(rec.ops)
    del rec.ops[:]
    eng.noise = InjectedNoise(RC.draws(T=1), [])
    eng.forward(kw["x"], pose=kw["pose"], condition=kw["candidates"][:1].expand(3, -1).contiguous())
    fwd = [o for o in rec.ops if o not in ("random_normal", "counter_add")]
    eng.close()
    return plan, fwd


def test_launch_accounting():
    """Nothing in front of the heads scales with N: up to the decoders a request issues the calls of ONE forward, the two image
    heads' joins replaced one for one by the tiled join; the count does not depend on N up to 8 candidates; the ninth adds one
    launch per goal term; the tail is the row kernels, kl_rows, one plan_select and one gather_best."""
    runs = {N: recorded(N) for N in (1, 2, 5, 8, 9)}
    fwd = runs[1][1]
    assert fwd.count("concat_condition") == 4 and len(fwd) > 10
    tiled, seen = [], 0
    for o in fwd:                                   # the first two joins of a forward are the image encoders' heads
        if o == "concat_condition" and seen < 2:
            tiled.append("concat_condition_tiled")
            seen += 1
        else:
            tiled.append(o)
    tail = ["bce_logits_rows_groups", "bce_logits_rows_groups", "mse_rows_groups"]
    for N in (1, 2, 5, 8):
        plan = runs[N][0]
        assert plan == tiled + tail + ["kl_rows", "plan_select", "gather_best"], (N, plan)
    assert runs[9][0] == tiled + tail * 2 + ["kl_rows", "plan_select", "gather_best"]
    # a goal of one image alone: one row launch per chunk
    rec = Recorder(EmuBackendPlan())
    ops.set_backend(rec)
    eng = MVAEInference(PC.build(False), use_graph=False)
    kw = plan_kw("shared", 9)
    kw["goal"] = [kw["goal"][0], None, None]
    r = eng.plan(**kw)
    assert rec.ops.count("bce_logits_rows_groups") == 2 and rec.ops.count("mse_rows_groups") == 0
    assert r["bce_tactile"] is None and r["mse_pose"] is None and tuple(r["bce_visual"].shape) == (9, 3)
    eng.close()


def test_argument_errors():
    eng = MVAEInference(PC.build(False), use_graph=False)
    kw = plan_kw("shared")
    B, cd = 3, CC.REAL_DIM
    bad = lambda **k: dict(kw, **k)
    for c in (None, torch.zeros(0, cd), torch.zeros(2, cd + 1), torch.zeros(2, cd, dtype=torch.int64), torch.zeros(cd),
              torch.zeros(B + 1, 2, cd), torch.zeros(2, 2, 2, cd), [[0.0] * cd]):
        with pytest.raises(ValueError, match="candidate"):
            eng.plan(**bad(candidates=c))
    for g in (None, [None, None, None], [kw["goal"][0][:2], None, None], [None, None, kw["goal"][2][:, :6]], kw["goal"][0]):
        with pytest.raises(ValueError, match="goal"):
            eng.plan(**bad(goal=g))
    with pytest.raises(ValueError, match="loss_mask"):
        eng.plan(**bad(loss_mask=torch.ones(B, 1, 64, 64)))
    with pytest.raises(ValueError, match="loss_mask"):
        eng.plan(**bad(goal=[kw["goal"][0], None, None], loss_mask=torch.ones(B, 2, 64, 64)))
    with pytest.raises(ValueError, match="modality"):
        eng.plan(**bad(x=[None, None], pose=None))
    most = (2 ** 31 - 1) // (B * 32 * 32 * 32)
    with pytest.raises(ValueError, match=rf"largest N for B = {B} is {most}\b"):
        eng.plan(**bad(candidates=torch.zeros(most + 1, cd)))
    # a masked goal without the pose term is served
    r = eng.plan(**bad(goal=[kw["goal"][0], kw["goal"][1], None], loss_mask=torch.ones(B, 1, 64, 64)))
    assert r["mse_pose"] is None and tuple(r["cost"].shape) == (3, B)
    # a backend written before the ops: an error that names one of them
    ops.set_backend(EmuBackendRollout())
    with pytest.raises(RuntimeError, match="plan_select"):
        eng.plan(**kw)
    eng.close()
    ops.set_backend(EmuBackendPlan())
    cat = MVAEInference(PC.build(True), use_graph=False)
    for c in (torch.zeros(2), torch.zeros(B + 1, 2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
              torch.zeros(2, 2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="candidate"):
            cat.plan(**bad(candidates=c))
    # an index out of range is served as an all-zero block and reported
    r = cat.plan(**bad(candidates=torch.tensor([1, CC.CAT_DIM], dtype=torch.int32)))
    assert cat.bad_condition() and r["best_condition"].dtype == torch.int64
    cat.plan(**bad(candidates=torch.tensor([[1, 2], [0, 4], [3, 3]], dtype=torch.uint8)))
    assert not cat.bad_condition()
    cat.close()
    import avail_cases as A
    plain = MVAEInference(setup_model("cnn-mvae", cross_modal=True, **A.PLAIN_KW).eval(), use_graph=False)
    with pytest.raises(ValueError, match="unconditional model"):
        plain.plan(**kw)
    plain.close()


def test_hip_backend_validates_on_the_host():
    """HipBackend.concat_condition_tiled / plan_select / gather_best check shapes and dtypes before they touch the library, and
    refuse CPU tensors."""
    hip = ops.HipBackend()
    N, B, cd = 2, 3, 3
    f = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    d = lambda *s: f(*s, dtype=torch.float64)
    sel = lambda **k: dict(dict(bce_rows=d(2, N, B), mse_rows=d(N, B), kl_rows=d(N, B), tavail=None, candidates=f(N * B, cd), cost=f(N, B),
                                best=f(B, dtype=torch.int32), best_cost=f(B), best_condition=f(B, cd), N=N, B=B, pose_multiplier=1.0), **k)
    for k in (sel(bce_rows=d(1, N, B)), sel(mse_rows=f(N, B)), sel(kl_rows=d(B, N)), sel(kl_rows=None), sel(candidates=f(N * B)),
              sel(candidates=f(N * B + 1, cd)), sel(candidates=f(N * B, dtype=torch.int64)), sel(best=f(B, dtype=torch.int64)),
              sel(cost=f(B, N)), sel(best_condition=f(B, cd + 1)), sel(N=0), sel(tavail=torch.ones(B, 3, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            hip.plan_select(**k)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.plan_select(**sel())
    grp = lambda **k: dict(dict(src=f(N * B, 7), out=f(B, 7), logits=False), **k)
    best = f(B, dtype=torch.int32)
    for groups, bst, n in (([], best, N), ([grp()] * 5, best, N), ([grp(out=f(B, 8))], best, N), ([grp(src=f(N * B + 1, 7))], best, N),
                           ([grp(src=d(N * B, 7))], best, N), ([grp(out=f(B, 14)[:, ::2])], best, N), ([grp()], best.long(), N),
                           ([grp()], f(B + 1, dtype=torch.int32), N), ([grp()], best, 0), ([grp(src=f(N * B, 0), out=f(B, 0))], best, N)):
        with pytest.raises(ValueError):
            hip.gather_best(groups, bst, n, B)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.gather_best([grp()], best, N, B)
    with pytest.raises(ValueError, match="multiple"):
        hip.concat_condition_tiled(f(2, 8), f(5, cd), f(5, 32), 8, cd, 2)
    with pytest.raises(ValueError):
        hip.concat_condition_tiled(f(3, 8), f(6, cd), f(6, 32), 8, cd, 2)          # x holds three rows, not x_rows = 2


def test_emulated_ops_keep_the_untaken_side_out():
    emu, nan = EmuBackendPlan(), float("nan")
    N, B = 3, 4
    src = torch.randn(N * B, 5)
    best = torch.tensor([2, -1, 0, 7], dtype=torch.int32)          # row 1: no winner; row 3: an index out of range
    clean = torch.empty(B, 5)
    emu.gather_best([dict(src=src, out=clean, logits=True)], best, N, B)
    taken = torch.zeros(N * B, dtype=torch.bool)
    taken[2 * B + 0] = taken[0 * B + 2] = True
    src[~taken] = nan
    out = torch.zeros(B, 5)
    emu.gather_best([dict(src=src, out=out, logits=True)], best, N, B)
    assert torch.isnan(out[1]).all() and torch.isnan(out[3]).all() and torch.isfinite(out[[0, 2]]).all()
    assert torch.equal(out[[0, 2]], clean[[0, 2]]) and torch.equal(out[0], torch.sigmoid(src[2 * B]))
    x, cond, o = torch.randn(2, 8), torch.rand(6, 3), torch.full((6, 32), nan)
    emu.concat_condition_tiled(x, cond, o, 8, 3, 2)
    assert torch.equal(o[:, :8], x.repeat(3, 1)) and torch.equal(o[:, 8:11], cond) and float(o[:, 11:].abs().sum()) == 0.0


def loader_batch(n, l, cd, seed=931):
    """A loader batch of n sequences of l frames, flat: (data [visual, tactile, pose, available [n*l, 2], shock [n*l, cd]], target
    [visual, tactile, pose, mask])."""
    from mmdyn_hip.utils.seeded_init import seeded_batch
    a, b = seeded_batch(n * l, seed, with_pose=True)
    has = torch.ones(n * l, 2, dtype=torch.float64)
    has[1, 0] = 0.0                                                       # frame 1 of sequence 0 lacks vision
    shock = torch.rand(n * l, cd, generator=torch.Generator().manual_seed(seed))
    return a + [has, shock], b + [torch.ones(n * l, 1, 64, 64)]


def check_problem_layer(device):
    """DynModeling.plan on a loader batch of n = 2 sequences of l = 2 frames with a shock column: the shapes, ``recorded``, the
    goal availability from the dataset's column (the goal of frame 0 is frame 1, which lacks vision), the model's mode, and the
    refusals."""
    n, l, N = 2, 2, 3
    model = PC.build(False, device)
    prob = TMM.problem_of(model, "cnn-mvae", True, device, DynModeling)
    prob._seq_length, prob._kl_weight, prob._pose_multiplier = l, PC.KL_WEIGHT, PC.POSE_MULTIPLIER
    data, target = loader_batch(n, l, CC.REAL_DIM)
    cand = torch.rand(N, CC.REAL_DIM, generator=torch.Generator().manual_seed(4))
    model.train()
    res = prob.plan(data, target, cand)
    assert model.training
    model.eval()
    assert set(res) == KEYS | {"recorded"}
    Bt = n * l
    assert tuple(res["cost"].shape) == (N, Bt) and tuple(res["best"].shape) == (Bt,) and tuple(res["best_condition"].shape) == (Bt, CC.REAL_DIM)
    assert [tuple(p.shape) for p in res["prediction"]] == [(Bt, 3, 64, 64), (Bt, 3, 64, 64), (Bt, 7)]
    assert torch.equal(res["recorded"].cpu(), data[4]) and tuple(res["means"].shape) == (N, Bt, L)
    assert float(res["bce_visual"][:, 0].abs().sum()) == 0.0 and float(res["bce_visual"][:, 1:].min()) > 0.0
    assert float(res["bce_tactile"].min()) > 0.0 and float(res["mse_pose"].min()) > 0.0
    assert int(res["best"].min()) >= 0 and int(res["best"].max()) < N
    # the engine beside it gives the same table
    eng = MVAEInference(model, use_graph=False)
    x, tg = prob.parse_input(data, target)
    gav = torch.ones(Bt, 3)
    gav[0, 0] = 0.0
    want = eng.plan(list(x["model_input"]), pose=x["input_object_pose"][0], goal=list(tg["target_output"]) + [tg["target_object_pose"][0]],
                    candidates=cand.to(device), available=x["input_available_modals"], goal_available=gav, **KW)
    np.testing.assert_allclose(res["cost"].cpu().numpy(), want["cost"].cpu().numpy(), rtol=REL)
    eng.close()
    prob._planner.close()
    with pytest.raises(ValueError, match="shock"):
        prob.plan(data[:4], target, cand)
    with pytest.raises(ValueError):
        prob.plan(data[0], target[0], cand)
    import avail_cases as A
    plain = TMM.problem_of(setup_model("cnn-mvae", cross_modal=True, **A.PLAIN_KW).to(device).eval(), "cnn-mvae", False, device, DynModeling)
    plain._seq_length = l
    with pytest.raises(ValueError, match="unconditional"):
        plain.plan(data, target, cand)
    vae = TMM.problem_of(model, "cnn-vae", True, device, DynModeling)
    vae._seq_length = l
    with pytest.raises(ValueError, match="cnn-vae"):
        vae.plan(data, target, cand)


def test_problem_layer():
    check_problem_layer("cpu")
