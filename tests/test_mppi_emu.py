"""MPPI weights and the receding-horizon warm start on the CPU: mmdyn_plan_refit_weighted / mmdyn_plan_shift through the emulation
backend (tests/emu_backend_mppi.py) against the one-operation-per-rounding restatements of tests/mppi_cases.py, then
``MVAEInference.plan_refine(temperature=..., warm_start=...)`` against the chain of existing requests, the warm start's incumbent and
shifted mean, the launch accounting, the error paths and ``DynModeling.plan_refine``.  The ``check_*`` functions take the backend and /
or the device: tests/test_mppi_gpu.py runs them on the HIP library."""
import pytest
import torch

import dirty
import mppi_cases as MC
import plan_cases as PC
import refine_cases as RF
import rollout_cases as RC
import test_horizon_emu as H
import test_mixed_modal_emu as TMM
import test_refine_emu as R
from emu_backend_mppi import EmuBackendMppi
from emu_backend_refine import EmuBackendRefine
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.problems.problems import DynModeling
from test_elbo_rows_emu import REL
from test_ensemble_emu import ShapeRecorder

CD = RF.CD
nan, inf = float("nan"), float("inf")
same_bits, ulps, placed, cpu, keep = R.same_bits, R.ulps, R.placed, R.cpu, R.keep
KEYS = R.KEYS | {"ess", "weight"}
SEEN = {"weight ulps": 0, "std ulps": 0}         # the largest distances of this process, printed by the checks


@pytest.fixture(autouse=True)
def emu_mppi():
    old = ops.set_backend(EmuBackendMppi())
    yield
    ops.set_backend(old)


# ---- plan_refit_weighted -------------------------------------------------------------------------------------------------------
def run_weighted(backend, device, cost, cand, mean_in, std_in, K, temperature, alpha=0.0, std_min=0.0, in_place=False):
    """(mean_out, std_out, elite, count, weight, ess) of one launch on copies, every destination pre-filled with sevens."""
    N, B = cost.shape
    T = cand.shape[0]
    mv = lambda t: t.clone().to(device)
    cost, cand, mean_in, std_in = mv(cost), mv(cand), mv(mean_in), mv(std_in)
    mean_out, std_out = (mean_in, std_in) if in_place else (torch.full_like(mean_in, 7.0), torch.full_like(std_in, 7.0))
    elite, count = torch.full((N, B), 7, dtype=torch.uint8, device=device), torch.full((B,), 7, dtype=torch.int32, device=device)
    weight, ess = torch.full((N, B), 7.0, dtype=torch.float64, device=device), torch.full((B,), 7.0, device=device)
    backend.plan_refit_weighted(cost, cand, mean_in, std_in, mean_out, std_out, elite, count, weight, ess, K, N, B, T, temperature,
                                alpha, std_min)
    return tuple(t.cpu() for t in (mean_out, std_out, elite, count, weight, ess))


def check_weights(got, cost, K, temperature, exact, what):
    """The weight table against torch's fp64 exp of the same arguments: where the header fixes the value (0 for a non-elite and
    from q = 800 on, 1 at the minimum) the bits; where it comes from exp with q <= 700, the bits on the emulation and at most
    MC.EXP_ULPS fp64 ulps on the device.  Returns (the reference weights, elite, count)."""
    want, q, elite, count = MC.weights_ref(cost, K, temperature)
    from_exp = q == q
    assert not bool(((q > MC.Q_ULP_MAX) & (q < MC.Q_ZERO_MIN)).any()), "a test column between the two ranges of q"
    fixed = ~from_exp | (q >= MC.Q_ZERO_MIN)
    assert same_bits(got[fixed], want[fixed]), (what, got[fixed], want[fixed])
    assert bool((want[from_exp & (q >= MC.Q_ZERO_MIN)] == 0).all())
    rest = from_exp & (q <= MC.Q_ULP_MAX)
    far = MC.ulps64(got[rest], want[rest])
    SEEN["weight ulps"] = max(SEEN["weight ulps"], far)
    print("plan_refit_weighted", what, "weights from exp:", int(rest.sum()), "largest distance to torch's fp64 exp in ulps", far,
          "allowed", 0 if exact else MC.EXP_ULPS, "| largest so far", SEEN["weight ulps"])
    assert far <= (0 if exact else MC.EXP_ULPS), (what, far)
    return want, elite, count


def check_weight_rules(backend, device, exact):
    """Hand-written cost columns: (column, K, temperature, the weights where they are 0 or 1 / None where exp decides).  Ties at the
    minimum, c_min = -Inf, all elites +Inf, NaN costs, K' = 0, K' < K, q >= 800 (exactly 0) and q <= 700."""
    e = None
    rows = [([2, 5, 2, 9, 2], 5, 1.0, [1, e, 1, e, 1]), ([2, 5, 2, 9, 2], 3, 1.0, [1, 0, 1, 0, 1]), ([2, 5, 2, 9, 2], 4, 2.0, [1, e, 1, 0, 1]),
            ([3, -inf, 4, -inf, inf], 5, 1.0, [0, 1, 0, 1, 0]), ([3, -inf, 4, -inf, inf], 1, 1.0, [0, 1, 0, 0, 0]),
            ([inf] * 5, 2, 1.0, [1, 1, 0, 0, 0]), ([inf] * 5, 5, 0.5, [1] * 5), ([3, inf, 1, inf, 2], 5, 1.0, [e, 0, 1, 0, e]),
            ([nan, 1, nan, 0, 7], 5, 1.0, [0, e, 0, 1, e]), ([nan, 1, nan, 0, 7], 2, 1.0, [0, e, 0, 1, 0]),
            ([nan] * 5, 3, 1.0, [0] * 5), ([nan] * 5, 5, 1.0, [0] * 5), ([nan, 1, nan, 0, nan], 4, 1.0, [0, e, 0, 1, 0]),
            ([0, 800, 1000, 1e30, 900], 5, 1.0, [1, 0, 0, 0, 0]), ([1, 401, 1.5, 501, 351], 5, 0.5, [1, 0, e, 0, e]),
            ([0, 700, 350.25, 0.001, 699.5], 5, 1.0, [1, e, e, e, e]), ([-3, 0.5, 4, -3, 100], 4, 0.125, [1, e, e, 1, 0]),
            ([2.5], 1, 1.0, [1]), ([nan], 1, 1.0, [0]), ([0.0, -0.0, 1], 3, 1.0, [1, 1, e])]
    T, cd = 2, 3
    for col, K, temp, fixed in rows:
        N, B = len(col), 2                                               # the column in row 1; row 0 holds it reversed
        cost = torch.tensor([col[::-1], col], dtype=torch.float32).t().contiguous()
        cand, mean_in, std_in = R.refit_operands(B, N, T, cd, 40 + N + K)
        mean, std, elite, count, weight, ess = run_weighted(backend, device, cost, cand, mean_in, std_in, K, temp, 0.25, 0.0)
        want, re_, rc = check_weights(weight, cost, K, temp, exact, (col, K, temp))
        for n, v in enumerate(fixed):
            if v is not None:
                assert float(weight[n, 1]) == float(v) == float(want[n, 1]), (col, K, n, weight[:, 1])
            else:
                assert 0.0 < float(weight[n, 1]) < 1.0, (col, K, n, weight[:, 1])
        assert torch.equal(elite, re_) and torch.equal(count, rc), (col, K)
        kp = int(count[1])
        rm, rs, _, _, _, ress = MC.refit_weighted_ref(cost, cand, mean_in, std_in, K, temp, 0.25, 0.0, weights=weight)
        assert same_bits(mean, rm) and ulps(std, rs) <= 1 and same_bits(ess, ress), (col, K)
        if kp == 0:
            assert same_bits(mean[1], mean_in[1]) and same_bits(std[1], std_in[1]) and float(ess[1]) == 0.0
        else:
            assert 1.0 <= float(ess[1]) <= kp, (col, K, ess)


def weighted_costs(B, N, temperature, seed):
    """A cost table whose q = (cost - c_min) / temperature stays below 700: half the candidates within a few temperatures of the best
    (weights of the order of one), half up to ~600 temperatures away, exact ties at the minimum of row 0, and -- for N >= 5 -- a NaN
    and a +Inf, which both end with weight zero."""
    g = torch.Generator().manual_seed(seed)
    q = torch.where(torch.rand(N, B, generator=g) < 0.5, 4.0 * torch.rand(N, B, generator=g), 600.0 * torch.rand(N, B, generator=g))
    cost = 3.0 + f32(temperature) * q
    if N >= 5:
        cost[0, 0] = cost[N - 1, 0] = float(cost[:, 0].min())
        cost[1, 0], cost[2, B - 1] = nan, inf
    return cost


f32 = RF.f32


def check_refit_weighted(backend, device, B, N, K, T, cd, exact):
    """Against the restatements: the weights (check_weights), elite / count equal to plan_refit's on the same table, mean_out
    bit-equal to the restatement fed the backend's own weights, std_out within one fp32 ulp of it (plan_refit's bound: the device's
    fp64 sqrt), ess bit-equal to its restatement; in place == out of place; NaN over every candidate of weight zero changes
    nothing.  The candidates are N(0, 1) draws: their spread among the elites is of the order of their magnitude, far above the
    1e-3 from which on the bound is a property of the arithmetic and not of cancellation."""
    for temp, alpha, std_min in ((0.75, 0.0, 0.0), (3.0, 0.25, 0.125)):
        cost = weighted_costs(B, N, temp, 60 + B + N)
        cand, mean_in, std_in = R.refit_operands(B, N, T, cd, 61 + B + N + K)
        mean, std, elite, count, weight, ess = run_weighted(backend, device, cost, cand, mean_in, std_in, K, temp, alpha, std_min)
        want_w, re_, rc = check_weights(weight, cost, K, temp, exact, (B, N, K, T, cd, temp))
        plain = R.run_refit(backend, device, cost, cand, mean_in, std_in, K, alpha, std_min)
        assert torch.equal(elite, plain[2]) and torch.equal(count, plain[3]) and torch.equal(elite, re_) and torch.equal(count, rc)
        rm, rs, _, _, _, ress = MC.refit_weighted_ref(cost, cand, mean_in, std_in, K, temp, alpha, std_min, weights=weight)
        assert same_bits(mean, rm), (B, N, K, T, cd, temp, dirty.first_diff(mean, rm))
        far = ulps(std, rs)
        SEEN["std ulps"] = max(SEEN["std ulps"], far)
        print("plan_refit_weighted", (B, N, K, T, cd), "temperature", temp, "std_out: largest distance to the restatement in ulps", far,
              "allowed 1 | ess", ess.tolist())
        assert far <= 1
        assert same_bits(ess, ress) and bool((ess >= 1.0).all()) and bool((ess <= count.float()).all())
        again = run_weighted(backend, device, cost, cand, mean_in, std_in, K, temp, alpha, std_min, in_place=True)
        assert all(same_bits(a, b) for a, b in zip(again, (mean, std, elite, count, weight, ess)))
        dead = (weight == 0).view(1, N, B, 1).expand(T, N, B, cd).reshape(T, N * B, cd)
        assert bool(dead.any())
        poisoned = run_weighted(backend, device, cost, torch.where(dead, torch.full_like(cand, nan), cand), mean_in, std_in, K, temp,
                                alpha, std_min)
        assert all(same_bits(a, b) for a, b in zip(poisoned, (mean, std, elite, count, weight, ess)))


def check_tie_identity(backend, device, B, N, K, T, cd):
    """A table whose K smallest costs are equal in every row: every weight is 1, and mean_out / std_out have the bits
    mmdyn_plan_refit writes on the same inputs -- whatever the temperature."""
    g = torch.Generator().manual_seed(70 + N + K)
    cost = 5.0 + torch.rand(N, B, generator=g)
    for b in range(B):
        cost[torch.randperm(N, generator=g)[:K], b] = 1.25
    cand, mean_in, std_in = R.refit_operands(B, N, T, cd, 71 + N)
    plain = R.run_refit(backend, device, cost, cand, mean_in, std_in, K, 0.25, 0.0625)
    for temp in (1e-3, 1.0, 1e6):
        got = run_weighted(backend, device, cost, cand, mean_in, std_in, K, temp, 0.25, 0.0625)
        assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[1]) and torch.equal(got[2], plain[2]) and torch.equal(got[3], plain[3])
        assert torch.equal(got[4], got[2].double()) and torch.equal(got[5], torch.full((B,), float(K)))


def check_weighted_dirty(backend, device):
    B, N, K, T, cd = 5, 9, 4, 3, 3
    cost = weighted_costs(B, N, 1.5, 8)
    cand, mean_in, std_in = R.refit_operands(B, N, T, cd, 9)
    args = (cost, cand, mean_in, std_in, torch.empty(B, T, cd), torch.empty(B, T, cd), torch.empty(N, B, dtype=torch.uint8),
            torch.empty(B, dtype=torch.int32), torch.empty(N, B, dtype=torch.float64), torch.empty(B), K, N, B, T, 1.5, 0.25, 0.125)
    dirty.assert_same_bits(dirty.run_dirty(backend, "plan_refit_weighted", args, outs=[4, 5, 6, 7, 8, 9], device=device),
                           what="plan_refit_weighted: ")


# ---- plan_shift ----------------------------------------------------------------------------------------------------------------
def shift_operands(B, T, cd, seed):
    """(prev_mean, prev_std, prev_keep, init_mean, init_std) with NaN / Inf planted in the previous plan and a NaN std in the tail
    source (no element holds a NaN on both sides of the fmax, and no Inf meets widen = 0)."""
    g = torch.Generator().manual_seed(seed)
    pm, pk, im = (torch.randn(B, T, cd, generator=g) for _ in range(3))
    ps, is_ = 0.05 + torch.rand(B, T, cd, generator=g), 0.05 + torch.rand(B, T, cd, generator=g)
    pm.view(-1)[0], pm.view(-1)[-1], pk.view(-1)[1 % pk.numel()] = nan, -inf, inf
    ps.view(-1)[-1] = inf
    if B * T * cd > 2:
        ps.view(-1)[2], pk.view(-1)[-2] = nan, nan
        is_.view(-1)[-2] = nan
    return pm, ps, pk, im, is_


def run_shift(backend, device, ops_, shift, widen, with_keep=True, offset=0):
    pm, ps, pk, im, is_ = ops_
    B, T, cd = pm.shape
    if not with_keep:
        pk = None
    new = lambda: (H.shifted(device, (B, T, cd), offset) if offset else torch.empty(B, T, cd, device=device)).fill_(7.0)
    outs = [new(), new(), new() if with_keep else None]
    backend.plan_shift(*(placed(t, device, offset) for t in (pm, ps, pk, im, is_)), *outs, B, T, shift, widen)
    return [None if t is None else t.cpu() for t in outs]


def check_shift_exact(backend, device, B, T, cd, offset=0):
    """Bit-equal to shift_ref: shift 0, 1 and T (and one in between), widen 0 and 0.5, with and without keep."""
    operands = shift_operands(B, T, cd, 80 + B + T + cd)
    for shift in sorted({0, 1, T // 2, T}):
        for widen in (0.0, 0.5):
            for with_keep in (True, False):
                got = run_shift(backend, device, operands, shift, widen, with_keep, offset)
                want = MC.shift_ref(operands[0], operands[1], operands[2] if with_keep else None, operands[3], operands[4], shift, widen)
                for k, a, b in zip(("mean_out", "std_out", "keep_out"), got, want):
                    assert (a is None) == (b is None) and (a is None or same_bits(a, b)), (B, T, cd, offset, shift, widen, with_keep, k)
    whole = run_shift(backend, device, operands, T, 0.5)                  # shift = T: the initial distribution, the incumbent at its mean
    assert same_bits(whole[0], operands[3]) and same_bits(whole[1], operands[4]) and same_bits(whole[2], operands[3])
    still = run_shift(backend, device, operands, 0, 0.0)                  # shift = 0, widen = 0: the previous plan (its NaN std gives way to 0)
    assert same_bits(still[0], operands[0]) and same_bits(still[2], operands[2])
    seen = ~torch.isnan(operands[1])
    assert same_bits(still[1][seen], operands[1][seen]) and bool((still[1][~seen] == 0).all())


def check_shift_dirty(backend, device):
    B, T, cd = 5, 3, 3
    pm, ps, pk, im, is_ = (torch.nan_to_num(t, nan=0.5, posinf=2.0, neginf=-2.0) for t in shift_operands(B, T, cd, 5))
    args = (pm, ps, pk, im, is_, torch.empty(B, T, cd), torch.empty(B, T, cd), torch.empty(B, T, cd), B, T, 1, 0.5)
    dirty.assert_same_bits(dirty.run_dirty(backend, "plan_shift", args, outs=[5, 6, 7], device=device), what="plan_shift: ")


def check_shift_overlaps(backend, device):
    """An output over an input or over another output is refused; the inputs may be one tensor."""
    B, T, cd = 2, 3, 4
    z = lambda: torch.zeros(B, T, cd, device=device)
    big = torch.zeros(2 * B * T * cd, device=device)
    a, b = big[:B * T * cd].view(B, T, cd), big[cd:cd + B * T * cd].view(B, T, cd)
    one = z()
    backend.plan_shift(one, one, one, one, one, z(), z(), z(), B, T, 1, 0.0)
    for k in (dict(mean_out=one), dict(std_out=one), dict(keep_out=one), dict(prev_std=a, std_out=b), dict(init_std=a, mean_out=b),
              dict(mean_out=a, std_out=b), dict(mean_out=a, keep_out=b), dict(std_out=a, keep_out=a)):
        kw = dict(dict(prev_mean=one, prev_std=one, prev_keep=one, init_mean=one, init_std=one, mean_out=z(), std_out=z(), keep_out=z()), **k)
        with pytest.raises(ValueError, match="overlaps"):
            backend.plan_shift(B=B, T=T, shift=1, widen=0.0, **kw)


# ---- the engine ----------------------------------------------------------------------------------------------------------------
TEMPERATURE = 100.0   # the costs of these requests are a few 1e4 and the candidates of a row a few hundred apart: q up to about six


def ask(eng, name, device, **over):
    return R.ask(eng, name, device, **over)


def mppi_chain(eng, name, device, temperature, exact):
    """The loop on the host around plan_rollout: per iteration the restated candidates, one request, the restated weighted refit
    from the weights plan_refine returned for that iteration (the last iteration of the request cut short there).  Returns the chain's
    result and plan_refine's."""
    B, N, K, T, I = RF.CASES[name][:5]
    runs = [cpu(ask(eng, name, device, iterations=i + 1, temperature=temperature)) for i in range(I)]
    _, _, mean, std, bounds, draws = RF.request(name)
    mean, std = mean.expand(B, T, CD).contiguous(), std.expand(B, T, CD).contiguous()
    lo, hi = bounds if bounds is not None else (None, None)
    rollout = R.rollout_of(eng, name, device)
    keep_, history, esses, r = None, [], [], None
    for i in range(I):
        cand = RF.sample_ref(mean, std, draws[i], keep_, lo, hi)
        r = rollout(cand.view(T, N, B, CD).permute(2, 1, 0, 3).contiguous())
        keep_ = r["best_condition"]
        w = runs[i]["weight"]
        want_w, q, _, count = MC.weights_ref(r["cost"], K, temperature)
        near = (q != q) | (q <= MC.Q_ULP_MAX) | (q >= MC.Q_ZERO_MIN)
        far = MC.ulps64(w[near], want_w[near])
        print(name, "iteration", i, "weights: largest distance to torch's fp64 exp in ulps", far, "| q up to", float(torch.nan_to_num(q).max()))
        assert far <= (0 if exact else MC.EXP_ULPS)
        mean, std, _, _, _, ess = MC.refit_weighted_ref(r["cost"], cand, mean, std, K, temperature, weights=w)
        history.append(r["best_cost"])
        esses.append(ess)
        assert bool((ess >= 1.0).all()) and bool((ess <= count.float()).all())
    return dict(r, mean=mean, std=std, candidates=cand, history=torch.stack(history), ess=torch.stack(esses)), runs[-1]


def check_mppi_chain(device, name, exact):
    B, N, K, T, I = RF.CASES[name][:5]
    eng = MVAEInference(PC.build(False, device), use_graph=False)
    want, r = mppi_chain(eng, name, device, TEMPERATURE, exact)
    assert set(r) == KEYS and tuple(r["ess"].shape) == (I, B) and tuple(r["weight"].shape) == (N, B) and r["weight"].dtype == torch.float64
    pairs = [("candidates", r["candidates"].reshape(T, N * B, CD), want["candidates"])]
    pairs += [(k, r[k], want[k]) for k in ("cost", "best", "best_cost", "best_condition", "mean", "history", "ess")]
    print(name, "MPPI against the chain: bit-equal", {k: same_bits(a, b) for k, a, b in pairs}, "std ulps", ulps(r["std"], want["std"]),
          "ess", r["ess"].tolist())
    for k, a, b in pairs:
        assert same_bits(a, b), (name, k, dirty.first_diff(a, b))
    assert ulps(r["std"], want["std"]) <= 1
    assert r["elite_count"].tolist() == [[K] * B] * I
    assert bool((r["ess"] >= 1.0).all()) and bool((r["ess"] <= K).all())
    eng.close()


def check_large_temperature_is_cem(device, name):
    """K = N and a temperature of 1e30: q = (cost - c_min) / 1e30 lies below 2^-54 for every cost difference below 5e13, so every
    exp(-q) rounds to exactly 1 and the request has the bits of CEM with K = N (no cost is a NaN here: asserted)."""
    N = RF.CASES[name][1]
    eng = MVAEInference(PC.build(False, device), use_graph=False)
    a, b = cpu(ask(eng, name, device, elites=N, temperature=1e30)), cpu(ask(eng, name, device, elites=N))
    assert not bool(torch.isnan(b["cost"]).any()) and float(b["cost"].max() - b["cost"].min()) < 5e13
    assert bool((a["weight"] == 1.0).all()) and bool((a["ess"] == float(N)).all())
    for k in ("candidates", "cost", "best", "mean", "std", "history", "elite_count", "best_condition"):
        assert same_bits(a[k], b[k]), k
    eng.close()


def check_warm_start(device, name="steps"):
    """warm_start = the previous result.  shift = 0, widen = 0: round 0's slot 0 is the previous winner and its cost does not rise
    above the previous best (judged as the non-rising history is: REL).  shift = 1: slot 0 is shift_ref of the previous winner, and
    on draws of zeros every other candidate is shift_ref of the previous mean."""
    B, N, K, T, I = RF.CASES[name][:5]
    eng = MVAEInference(PC.build(False, device), use_graph=False)
    prev = cpu(ask(eng, name, device))
    warm = {k: prev[k].to(device) for k in ("mean", "std", "best_condition")}
    _, _, mean0, std0, bounds, _ = RF.request(name)
    assert bounds is None
    init = [t.expand(B, T, CD).contiguous() for t in (mean0, std0)]
    same = cpu(ask(eng, name, device, iterations=1, warm_start=warm, shift=0, widen=0.0))
    assert same_bits(same["candidates"][:, 0].transpose(0, 1), prev["best_condition"])
    h, before = same["history"][0].double(), prev["best_cost"].double()
    print(name, "warm start: round 0", h.tolist(), "the previous best", before.tolist())
    assert bool((h <= before * (1.0 + REL)).all())
    wm, ws, wk = MC.shift_ref(prev["mean"], prev["std"], prev["best_condition"], *init, 1, 0.5)
    moved = cpu(ask(eng, name, device, iterations=1, warm_start=warm, shift=1, widen=0.5))
    assert same_bits(moved["candidates"][:, 0].transpose(0, 1), wk)
    want = RF.sample_ref(wm, ws, RF.request(name)[5][0], wk).view(T, N, B, CD)
    assert same_bits(moved["candidates"], want)
    eng.noise = InjectedNoise([torch.zeros(N, B, T, CD)], [])
    still = cpu(keep(eng.plan_refine(**R.call_kw(name, device, iterations=1, warm_start=warm, shift=1, widen=0.5))))
    assert same_bits(still["candidates"][:, 1:], wm.transpose(0, 1).unsqueeze(1).expand(T, N - 1, B, CD).contiguous())
    assert same_bits(still["candidates"][:, 0].transpose(0, 1), wk)
    # the dict of a CPU-side copy, fp64 tensors and MPPI together: the same request
    both = cpu(ask(eng, name, device, iterations=1, warm_start={k: v.double() for k, v in prev.items() if torch.is_tensor(v)}, shift=1,
                   widen=0.5, temperature=TEMPERATURE))
    assert same_bits(both["candidates"], moved["candidates"]) and set(both) == KEYS
    eng.close()


def check_problem_layer(device, root):
    """DynModeling.plan_refine passes temperature / warm_start / shift / widen through: the engine beside it gives the same bits."""
    data, target, l = H.tree_batch(root, device)
    n = data[0].shape[0] // l
    model = PC.build(False, device)
    prob = TMM.problem_of(model, "cnn-mvae", True, device, DynModeling)
    prob._seq_length, prob._kl_weight, prob._pose_multiplier = l, H.HC.KL_WEIGHT, H.HC.POSE_MULTIPLIER
    N, K, I = 4, 4, 1
    draws = lambda: [torch.randn(N, n, l, CD, generator=torch.Generator().manual_seed(90))]
    first = prob.plan_refine(data, target, candidates=N, elites=K, iterations=I, temperature=TEMPERATURE)
    assert set(first) == KEYS | {"recorded"} and tuple(first["ess"].shape) == (I, n)
    prob._refiner.use_graph = False
    prob._refiner.noise = InjectedNoise(draws(), [])
    res = prob.plan_refine(data, target, candidates=N, elites=K, iterations=I, temperature=TEMPERATURE, warm_start=first, shift=1, widen=0.25)
    rec = data[4].reshape(n, l, -1).float()
    init = [rec.mean(0).expand(n, l, CD).contiguous(), rec.std(0, unbiased=False).expand(n, l, CD).contiguous()]
    wm, ws, wk = MC.shift_ref(first["mean"].cpu(), first["std"].cpu(), first["best_condition"].cpu(), *init, 1, 0.25)
    lo, hi = rec.reshape(-1, CD).min(0).values, rec.reshape(-1, CD).max(0).values
    assert same_bits(res["candidates"].cpu(), RF.sample_ref(wm, ws, draws()[0], wk, lo, hi).view(l, N, n, CD))
    prob._refiner.close()
    with pytest.raises(ValueError, match="temperature"):
        prob.plan_refine(data, target, temperature=0.0)
    with pytest.raises(ValueError, match="warm_start"):
        prob.plan_refine(data, target, shift=2)


# ---- the CPU suite -------------------------------------------------------------------------------------------------------------
WEIGHTED_SHAPES = [(3, 5, 5, 2, 3), (2, 8, 3, 1, 4), (2, 260, 260, 9, 32), (1, 4096, 64, 1, 4)]
SHIFT_SHAPES = [(3, 4, 4, 0), (3, 4, 3, 0), (3, 4, 4, 1), (1, 1, 1, 0), (70, 5, 8, 0)]
TIE_SHAPES = [(3, 9, 4, 2, 3), (2, 6, 6, 1, 4), (2, 300, 40, 2, 2)]


def test_weight_rules():
    check_weight_rules(EmuBackendMppi(), "cpu", exact=True)


@pytest.mark.parametrize("B,N,K,T,cd", WEIGHTED_SHAPES)
def test_refit_weighted_against_the_restatement(B, N, K, T, cd):
    check_refit_weighted(EmuBackendMppi(), "cpu", B, N, K, T, cd, exact=True)


@pytest.mark.parametrize("B,N,K,T,cd", WEIGHTED_SHAPES[:3])
def test_bound_holds_under_perturbed_weights(B, N, K, T, cd):
    """The inputs of check_refit_weighted, restated under two weight sets that differ as two exp implementations may -- every
    weight from exp moved MC.EXP_ULPS fp64 ulps up, and down: mean_out and std_out stay within one fp32 ulp of the restatement
    under torch's weights.  So a std_out more than one ulp off on the device is the arithmetic's doing, not exp's."""
    for temp, alpha, std_min in ((0.75, 0.0, 0.0), (3.0, 0.25, 0.125)):
        cost = weighted_costs(B, N, temp, 60 + B + N)
        cand, mean_in, std_in = R.refit_operands(B, N, T, cd, 61 + B + N + K)
        w = MC.weights_ref(cost, K, temp)[0]
        base = MC.refit_weighted_ref(cost, cand, mean_in, std_in, K, temp, alpha, std_min)
        assert same_bits(base[4], w)
        for k in (MC.EXP_ULPS, -MC.EXP_ULPS):
            moved = MC.stepped(w, k)
            assert MC.ulps64(moved, w) == MC.EXP_ULPS
            other = MC.refit_weighted_ref(cost, cand, mean_in, std_in, K, temp, alpha, std_min, weights=moved)
            print((B, N, K, T, cd), "weights moved", k, "ulps: mean", ulps(other[0], base[0]), "std", ulps(other[1], base[1]), "fp32 ulps")
            assert ulps(other[0], base[0]) <= 1 and ulps(other[1], base[1]) <= 1


@pytest.mark.parametrize("B,N,K,T,cd", TIE_SHAPES)
def test_equal_elite_costs_give_plan_refit(B, N, K, T, cd):
    check_tie_identity(EmuBackendMppi(), "cpu", B, N, K, T, cd)


def test_refit_weighted_on_dirty_destinations():
    check_weighted_dirty(EmuBackendMppi(), "cpu")


@pytest.mark.parametrize("B,T,cd,offset", SHIFT_SHAPES)
def test_shift_exact(B, T, cd, offset):
    check_shift_exact(EmuBackendMppi(), "cpu", B, T, cd, offset)


def test_shift_on_dirty_destinations_and_overlaps():
    check_shift_dirty(EmuBackendMppi(), "cpu")
    check_shift_overlaps(EmuBackendMppi(), "cpu")


@pytest.mark.parametrize("name", ["steps", "nine"])
def test_mppi_equal_to_the_chain_of_existing_requests(name):
    check_mppi_chain("cpu", name, exact=True)


def test_large_temperature_is_cem():
    check_large_temperature_is_cem("cpu", "steps")


def test_warm_start():
    check_warm_start("cpu")


def test_problem_layer(tmp_path):
    check_problem_layer("cpu", tmp_path)


# ---- emulation only ------------------------------------------------------------------------------------------------------------
def test_hip_backend_validates_on_the_host():
    """HipBackend.plan_refit_weighted / plan_shift check shapes, dtypes, ranges and overlaps before they touch the library, and
    refuse CPU tensors."""
    hip = ops.HipBackend()
    N, B, T, cd, K = 4, 3, 2, 3, 2
    f = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    i32, u8, f64 = torch.int32, torch.uint8, torch.float64
    fit = lambda **k: dict(dict(cost=f(N, B), cand=f(T, N * B, cd), mean_in=f(B, T, cd), std_in=f(B, T, cd), mean_out=f(B, T, cd),
                                std_out=f(B, T, cd), elite=f(N, B, dtype=u8), count=f(B, dtype=i32), weight=f(N, B, dtype=f64), ess=f(B),
                                K=K, N=N, B=B, T=T, temperature=1.0, alpha=0.5, std_min=0.0), **k)
    two, shared, wide = f(2 * B * T * cd), f(B, T, cd), f(2 * N * B, dtype=f64)
    for k in (fit(cost=None), fit(mean_out=None), fit(cost=f(B, N)), fit(cand=f(T, N * B)), fit(mean_in=f(B, T, cd + 1)), fit(elite=f(N, B)),
              fit(count=f(B + 1, dtype=i32)), fit(weight=f(N, B)), fit(weight=f(B, N, dtype=f64)), fit(ess=f(B, dtype=f64)), fit(ess=f(B + 1)),
              fit(K=0), fit(K=N + 1), fit(N=0), fit(B=0), fit(T=0), fit(alpha=1.0), fit(alpha=nan), fit(std_min=-1.0),
              fit(temperature=0.0), fit(temperature=-1.0), fit(temperature=nan), fit(temperature=inf),
              fit(mean_in=two[:B * T * cd].view(B, T, cd), mean_out=two[cd:cd + B * T * cd].view(B, T, cd)),
              fit(mean_in=shared, std_out=shared), fit(mean_out=shared, std_out=shared),
              fit(weight=wide[:N * B].view(N, B), ess=wide[N * B - 2:N * B + 1].view(torch.float32)[:B]),
              fit(ess=shared.view(-1)[:B], mean_in=shared), fit(ess=shared.view(-1)[:B], std_out=shared)):
        with pytest.raises(ValueError):
            hip.plan_refit_weighted(**k)
    for k in (fit(), fit(mean_in=shared, mean_out=shared), fit(elite=None, count=None, weight=None, ess=None)):
        with pytest.raises(RuntimeError, match="GPU tensors"):
            hip.plan_refit_weighted(**k)
    z = lambda: f(B, T, cd)
    sh = lambda **k: dict(dict(prev_mean=z(), prev_std=z(), prev_keep=z(), init_mean=z(), init_std=z(), mean_out=z(), std_out=z(),
                               keep_out=z(), B=B, T=T, shift=1, widen=0.0), **k)
    for k in (sh(prev_mean=None), sh(std_out=None), sh(prev_keep=None), sh(keep_out=None), sh(prev_std=f(T, B, cd)), sh(init_std=f(B, T, cd + 1)),
              sh(mean_out=f(B, T, cd, dtype=f64)), sh(keep_out=f(B, T, 2 * cd)[:, :, ::2]), sh(B=0), sh(T=0), sh(shift=-1), sh(shift=T + 1),
              sh(widen=-0.5), sh(widen=nan), sh(widen=inf), sh(prev_mean=shared, mean_out=shared), sh(init_std=shared, keep_out=shared),
              sh(mean_out=shared, std_out=shared), sh(prev_std=two[:B * T * cd].view(B, T, cd), std_out=two[cd:cd + B * T * cd].view(B, T, cd))):
        with pytest.raises(ValueError):
            hip.plan_shift(**k)
    for k in (sh(), sh(prev_keep=None, keep_out=None), sh(shift=0), sh(shift=T, widen=2.0), sh(prev_mean=shared, prev_std=shared, init_mean=shared)):
        with pytest.raises(RuntimeError, match="GPU tensors"):
            hip.plan_shift(**k)


def test_launch_accounting():
    """By name: one plan_shift in front of the loop and only with warm_start; I plan_refit_weighted and no plan_refit with
    temperature; the plain request's record is what a backend without the new ops records; such a backend raises the RuntimeError
    that names the missing op before anything is launched."""
    for N, K, I, T, every in ((3, 2, 2, 2, True), (9, 9, 3, 2, False)):
        kw = R.refine_kw(N, K, I, T, every)
        B = RC.BATCH
        plain = R.recorded(lambda e: e.plan_refine(**kw), backend=EmuBackendMppi())
        assert plain == R.recorded(lambda e: e.plan_refine(**kw), backend=EmuBackendRefine())
        names = lambda sigs: [s[0] for s in sigs]
        assert not {"plan_shift", "plan_refit_weighted"} & set(names(plain))
        mppi = R.recorded(lambda e: e.plan_refine(temperature=2.0, **kw), backend=EmuBackendMppi())
        assert [n.replace("plan_refit_weighted", "plan_refit") for n in names(mppi)] == names(plain)
        assert names(mppi).count("plan_refit_weighted") == I and "plan_refit" not in names(mppi)
        assert [s[1][-2:] for s in mppi if s[0] == "plan_refit_weighted"] == [((N, B), (B,))] * I          # the weights and a row of ess
        prev = {k: torch.rand(B, T, CD) for k in ("mean", "std", "best_condition")}
        warm = R.recorded(lambda e: e.plan_refine(warm_start=prev, shift=1, widen=0.5, **kw), backend=EmuBackendMppi())
        assert names(warm).count("plan_shift") == 1 and names(warm).count("plan_refit") == I
        at = names(warm).index("plan_shift")
        assert at == names(plain).index("random_normal") and names(warm)[:at] + names(warm)[at + 1:] == names(plain)
        assert warm[at][1] == ((B, T, CD),) * 8
        samples = [s for s in warm if s[0] == "plan_sample"]
        assert all(len(s[1]) == 5 for s in samples)                      # every round has an incumbent: mean, std, eps, keep, cand
        both = R.recorded(lambda e: e.plan_refine(temperature=2.0, warm_start=prev, **kw), backend=EmuBackendMppi())
        assert names(both).count("plan_shift") == 1 and names(both).count("plan_refit_weighted") == I and "plan_refit" not in names(both)
        for extra, op in ((dict(temperature=2.0), "plan_refit_weighted"), (dict(warm_start=prev), "plan_shift")):
            rec = ShapeRecorder(EmuBackendRefine())
            old = ops.set_backend(rec)
            eng = MVAEInference(PC.build(False), use_graph=False)
            del rec.ops[:], rec.sigs[:]
            try:
                with pytest.raises(RuntimeError, match=op):
                    eng.plan_refine(**kw, **extra)
                assert rec.sigs == []
            finally:
                ops.set_backend(old)
                eng.close()


def test_argument_errors_and_graph_keys():
    eng = MVAEInference(PC.build(False), use_graph=False)
    B, T = RC.BATCH, 2
    kw = R.refine_kw(3, 2, 2, T, True)
    bad = lambda **k: dict(kw, **k)
    prev = {k: torch.rand(B, T, CD) for k in ("mean", "std", "best_condition")}
    for v in (0, 0.0, -1.0, nan, inf, True, "1", 1e-60, 1e60):
        with pytest.raises(ValueError, match="temperature"):
            eng.plan_refine(**bad(temperature=v))
    for v in (-1, T + 1, 1.5, True, None):
        with pytest.raises(ValueError, match="shift"):
            eng.plan_refine(**bad(warm_start=prev, shift=v))
    for v in (-0.5, nan, inf, True, None, 1e60):
        with pytest.raises(ValueError, match="widen"):
            eng.plan_refine(**bad(warm_start=prev, widen=v))
    for k in (dict(shift=0), dict(shift=2), dict(widen=0.5)):
        with pytest.raises(ValueError, match="warm_start"):
            eng.plan_refine(**bad(**k))
    for w in ([prev["mean"]] * 3, {"mean": prev["mean"], "std": prev["std"]}, dict(prev, mean=torch.zeros(T, CD)), dict(prev, std=None),
              dict(prev, best_condition=torch.zeros(B, T, CD, dtype=torch.int64)), dict(prev, mean=torch.zeros(B, T + 1, CD))):
        with pytest.raises(ValueError, match="warm_start"):
            eng.plan_refine(**bad(warm_start=w))
    keys = []
    eng._run = lambda key, fn, args: keys.append(key)
    calls = [kw, bad(temperature=2.0), bad(temperature=2.0 + 1e-12), bad(temperature=3.0), bad(warm_start=prev),
             bad(warm_start={k: v + 1.0 for k, v in prev.items()}), bad(warm_start=prev, shift=1, widen=0.0), bad(warm_start=prev, shift=0),
             bad(warm_start=prev, widen=0.5), bad(warm_start=prev, temperature=2.0)]
    for c in calls:
        eng.plan_refine(**c)
    assert keys[1] == keys[2] and keys[4] == keys[5] == keys[6] and len(set(keys)) == len(calls) - 3
    assert keys[1] == keys[0] + (("mppi", 2.0),) and keys[4] == keys[0] + (("warm", 1, 0.0),) and keys[8] == keys[0] + (("warm", 1, 0.5),)
    assert keys[9] == keys[0] + (("mppi", 2.0), ("warm", 1, 0.0))
    eng.close()
