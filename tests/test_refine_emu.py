"""Iterative plan refinement on the CPU: mmdyn_plan_sample / mmdyn_plan_refit through the emulation backend
(tests/emu_backend_refine.py) against the one-operation-per-rounding restatements of tests/refine_cases.py, the refinement loop on a
model-free cost, and ``MVAEInference.plan_refine`` against the chain of existing requests a caller of ``plan_rollout`` would write on
the host -- bit for bit --, its incumbent slot, its history, the launch accounting, the error paths and ``DynModeling.plan_refine``.
The ``check_*`` functions take the backend and / or the device: tests/test_refine_gpu.py runs them on the HIP library."""
import json
import os

import numpy as np
import pytest
import torch

import cond_cases as CC
import dirty
import plan_cases as PC
import refine_cases as RF
import rollout_cases as RC
import test_horizon_emu as E
import test_mixed_modal_emu as TMM
from emu_backend_horizon import EmuBackendHorizon
from emu_backend_refine import EmuBackendRefine
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise, setup_model
from mmdyn_hip.problems.problems import DynModeling
from test_elbo_rows_emu import REL          # one candidate in another slot: the bound test_permuted_candidates of the horizon tests applies
from test_ensemble_emu import ShapeRecorder

CD = RF.CD
KW = E.KW
nan, inf = float("nan"), float("inf")
PLAN_KEYS = E.KEYS
KEYS = PLAN_KEYS | {"mean", "std", "candidates", "history", "elite_count"}


@pytest.fixture(autouse=True)
def emu_refine():
    old = ops.set_backend(EmuBackendRefine())
    yield
    ops.set_backend(old)


same_bits, dev_list, keep, cpu = E.same_bits, E.dev_list, E.keep, E.cpu


def placed(t, device, shift=0):
    """``t`` on the device, contiguous, starting ``shift`` floats past a 16-byte boundary."""
    if t is None:
        return None
    out = E.shifted(device, tuple(t.shape), shift) if shift else torch.empty(t.shape, device=device)
    out.copy_(t)
    return out


def ulps(a, b):
    """Largest distance of two fp32 tensors of one sign in units in the last place."""
    return int((dirty.bits(a).long() - dirty.bits(b).long()).abs().max())


# ---- plan_sample ---------------------------------------------------------------------------------------------------------------
def sample_operands(B, N, T, cd, seed):
    g = torch.Generator().manual_seed(seed)
    mean, std = torch.randn(B, T, cd, generator=g), 0.5 + torch.rand(B, T, cd, generator=g)
    eps, keep_ = torch.randn(N, B, T, cd, generator=g), torch.randn(B, T, cd, generator=g)
    lo, hi = -0.5 - torch.rand(cd, generator=g), 0.5 + torch.rand(cd, generator=g)
    return mean, std, eps, keep_, lo, hi


def run_sample(backend, device, mean, std, eps, keep_, lo, hi, shift=0):
    N, B, T, cd = eps.shape
    cand = E.shifted(device, (T, N * B, cd), shift) if shift else torch.empty(T, N * B, cd, device=device)
    cand.fill_(7.0)
    backend.plan_sample(*(placed(t, device, shift) for t in (mean, std, eps, keep_, lo, hi)), cand, N, B, T)
    return cand.cpu()


def check_sample_exact(backend, device, B, N, T, cd, shift=0):
    """cand against the fp32 restatement, bit for bit: plain; with the incumbent and bounds; NaN in ``keep`` falling back to the mean
    element by element; Inf / NaN in std and eps propagating; lo == hi; slot 0 untouched by a NaN in its eps."""
    mean, std, eps, keep_, lo, hi = sample_operands(B, N, T, cd, 11 + B + N + T + cd)
    for k, l, h in ((None, None, None), (keep_, None, None), (None, lo, hi), (keep_, lo, hi)):
        got, want = run_sample(backend, device, mean, std, eps, k, l, h, shift), RF.sample_ref(mean, std, eps, k, l, h)
        assert same_bits(got, want), (B, N, T, cd, shift, dirty.first_diff(got, want))
    holes = keep_.clone()
    holes.view(-1)[::2] = nan                                            # every other element of the incumbent is missing
    got = run_sample(backend, device, mean, std, eps, holes, lo, hi, shift)
    assert same_bits(got, RF.sample_ref(mean, std, eps, holes, lo, hi)) and not bool(torch.isnan(got).any())
    slot0 = got.view(T, N, B, cd)[:, 0].transpose(0, 1)
    clamp = lambda c: torch.where(c < lo, lo.expand_as(c), torch.where(c > hi, hi.expand_as(c), c))
    assert same_bits(slot0, clamp(torch.where(torch.isnan(holes), mean, holes)))
    wild_std, wild_eps = std.clone(), eps.clone()
    wild_std.view(-1)[0], wild_eps.view(-1)[-1] = inf, nan
    if B * T * cd > 1:
        wild_std.view(-1)[1] = nan
    wild_eps[0] = nan                                                    # the incumbent's draw is never read
    got = run_sample(backend, device, mean, wild_std, wild_eps, None, lo, hi, shift)
    assert same_bits(got, RF.sample_ref(mean, wild_std, wild_eps, None, lo, hi))
    assert same_bits(got.view(T, N, B, cd)[:, 0].transpose(0, 1), clamp(mean))
    if N > 1:
        assert bool(torch.isnan(got.view(T, N, B, cd)[T - 1, N - 1, B - 1, cd - 1]))       # a NaN passes the clamp
    pin = lo.clone()
    got = run_sample(backend, device, mean, std, eps, keep_, pin, pin.clone(), shift)  # lo == hi: every candidate is the bound
    assert same_bits(got, pin.expand(T, N * B, cd).contiguous())


def check_sample_dirty(backend, device):
    B, N, T, cd = 5, 9, 3, 3
    mean, std, eps, keep_, lo, hi = sample_operands(B, N, T, cd, 3)
    args = (mean, std, eps, keep_, lo, hi, torch.empty(T, N * B, cd), N, B, T)
    dirty.assert_same_bits(dirty.run_dirty(backend, "plan_sample", args, outs=[6], device=device), what="plan_sample: ")


# ---- plan_refit ----------------------------------------------------------------------------------------------------------------
def run_refit(backend, device, cost, cand, mean_in, std_in, K, alpha=0.0, std_min=0.0, in_place=False):
    N, B = cost.shape
    T = cand.shape[0]
    mv = lambda t: t.clone().to(device)
    cost, cand, mean_in, std_in = mv(cost), mv(cand), mv(mean_in), mv(std_in)
    mean_out, std_out = (mean_in, std_in) if in_place else (torch.full_like(mean_in, 7.0), torch.full_like(std_in, 7.0))
    elite, count = torch.full((N, B), 7, dtype=torch.uint8, device=device), torch.full((B,), 7, dtype=torch.int32, device=device)
    backend.plan_refit(cost, cand, mean_in, std_in, mean_out, std_out, elite, count, K, N, B, T, alpha, std_min)
    return mean_out.cpu(), std_out.cpu(), elite.cpu(), count.cpu()


def refit_operands(B, N, T, cd, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, N * B, cd, generator=g), torch.randn(B, T, cd, generator=g), 0.5 + torch.rand(B, T, cd, generator=g))


def check_refit_rules(backend, device):
    """Hand-written cost columns: (column, K, the elites).  Ties to the lower n, +-Inf ordinary, NaN never, K' < K, K' = 0 (the
    outputs are the inputs bit for bit), K = N, K = 1, N = 1."""
    rows = [([5, 2, 9, 2, 2], 2, [1, 3]), ([5, 2, 9, 2, 2], 3, [1, 3, 4]), ([3, inf, -inf, 4, inf], 3, [0, 2, 3]),
            ([3, inf, -inf, 4, inf], 4, [0, 1, 2, 3]), ([nan, 1, nan, 0, 7], 2, [1, 3]), ([nan, 1, nan, 0, nan], 4, [1, 3]),
            ([nan] * 5, 3, []), ([4, 3, 2, 1, 0], 5, [0, 1, 2, 3, 4]), ([4, 3, nan, 1, 1], 1, [3]), ([0.0, -0.0, 1, 1, 1], 1, [0]),
            ([inf] * 5, 2, [0, 1]), ([2.5], 1, [0]), ([nan], 1, [])]
    T, cd = 2, 3
    for col, K, want in rows:
        N, B = len(col), 2                                               # the column in row 1; row 0 holds it reversed
        cost = torch.tensor([col[::-1], col], dtype=torch.float32).t().contiguous()
        cand, mean_in, std_in = refit_operands(B, N, T, cd, 20 + N + K)
        mean, std, elite, count = run_refit(backend, device, cost, cand, mean_in, std_in, K, 0.25, 0.0)
        assert elite[:, 1].nonzero().reshape(-1).tolist() == want and int(count[1]) == len(want), (col, K, elite[:, 1], count)
        rm, rs, re_, rc = RF.refit_ref(cost, cand, mean_in, std_in, K, 0.25, 0.0)
        assert torch.equal(elite, re_) and torch.equal(count, rc) and same_bits(mean, rm), (col, K)
        assert ulps(std, rs) <= 1
        if not want:
            assert same_bits(mean[1], mean_in[1]) and same_bits(std[1], std_in[1])
        if len(want) == 1:                                               # one elite: the mean is that candidate, the spread is zero
            assert same_bits(run_refit(backend, device, cost, cand, mean_in, std_in, K)[0][1], cand.view(T, N, B, cd)[:, want[0], 1])
            assert float(run_refit(backend, device, cost, cand, mean_in, std_in, K)[1][1].abs().max()) == 0.0


def refit_costs(B, N, seed):
    """A cost table with ties, NaN and +-Inf in it (and none of them for N = 1)."""
    g = torch.Generator().manual_seed(seed)
    cost = torch.randint(0, max(2, N // 2), (N, B), generator=g).float() + 0.5          # many exact ties
    if N >= 9:
        cost[1, 0], cost[2, 0], cost[3, B - 1], cost[N - 1, B - 1] = nan, inf, -inf, nan
    return cost


def check_refit_restatement(backend, device, B, N, K, T, cd):
    """mean_out bit-equal to the fp64 restatement, elite and count exact, std_out within one fp32 ulp (the device's fp64 sqrt may
    differ from the host's by one fp64 ulp) and bit-equal where std_min wins; in place gives the bits of out of place."""
    cost = refit_costs(B, N, 30 + B + N)
    cand, mean_in, std_in = refit_operands(B, N, T, cd, 31 + B + N + K)
    for alpha, std_min in ((0.0, 0.0), (0.25, 0.125)):
        mean, std, elite, count = run_refit(backend, device, cost, cand, mean_in, std_in, K, alpha, std_min)
        rm, rs, re_, rc = RF.refit_ref(cost, cand, mean_in, std_in, K, alpha, std_min)
        assert torch.equal(elite, re_) and torch.equal(count, rc), (B, N, K)
        assert same_bits(mean, rm), (B, N, K, T, cd, alpha, dirty.first_diff(mean, rm))
        print("plan_refit", (B, N, K, T, cd), "alpha", alpha, "std_out: largest distance to the restatement in ulps", ulps(std, rs))
        assert ulps(std, rs) <= 1
        floor = rs == RF.f32(std_min)
        assert same_bits(std[floor], rs[floor])
        again = run_refit(backend, device, cost, cand, mean_in, std_in, K, alpha, std_min, in_place=True)
        assert same_bits(again[0], mean) and same_bits(again[1], std) and torch.equal(again[2], elite) and torch.equal(again[3], count)
    floor = run_refit(backend, device, cost, cand, mean_in, std_in, K, 0.0, 1e6)[1]        # the floor wins everywhere
    want = torch.where(rc.reshape(B, 1, 1) > 0, torch.full_like(std_in, 1e6), std_in)      # (a row without elites keeps its input)
    assert same_bits(floor, want)


def check_refit_is_top(backend, device, B, N, K):
    """K <= 8, distinct fp32 costs: the elites are the ``top`` list of mmdyn_plan_select_steps on tables that produce those costs
    (the KL table alone under a weight of one: c = ((0 + 0) + pm * 0) + 1 * kl)."""
    g = torch.Generator().manual_seed(50 + B + N + K)
    cost = (torch.randperm(N * B, generator=g).float() * 0.37 + 1.0).reshape(N, B)
    cand, mean_in, std_in = refit_operands(B, N, 1, CD, 51)
    elite = run_refit(backend, device, cost, cand, mean_in, std_in, K)[2]
    r = E.run_steps(backend, device, None, None, cost.double().unsqueeze(0), None, None, cand, 1000.0, 1.0, top=K)
    assert same_bits(r["cost"], cost)
    for b in range(B):
        assert sorted(r["top"][:, b].tolist()) == elite[:, b].nonzero().reshape(-1).tolist(), b


def check_refit_dirty(backend, device):
    B, N, K, T, cd = 5, 9, 3, 3, 3
    cost = refit_costs(B, N, 8)
    cand, mean_in, std_in = refit_operands(B, N, T, cd, 9)
    args = (cost, cand, mean_in, std_in, torch.empty(B, T, cd), torch.empty(B, T, cd), torch.empty(N, B, dtype=torch.uint8),
            torch.empty(B, dtype=torch.int32), K, N, B, T, 0.25, 0.125)
    dirty.assert_same_bits(dirty.run_dirty(backend, "plan_refit", args, outs=[4, 5, 6, 7], device=device), what="plan_refit: ")


# ---- the loop without the model -----------------------------------------------------------------------------------------------
def check_loop(backend, device):
    """Ten iterations of sample -> cost -> refit on injected draws: every iteration's mean has the bits of the CPU restatement of the
    same loop (which, by its own assertion, ends closer to the target than it began in every row)."""
    B, N, K, T, cd = (RF.LOOP[k] for k in ("B", "N", "K", "T", "cd"))
    want = RF.loop_ref()
    mean0, std0, target, draws = RF.loop_inputs()
    mean, std, target = mean0.to(device), std0.to(device), target.to(device)
    cand, best_cond = torch.empty(T, N * B, cd, device=device), None
    for i, eps in enumerate(draws):
        backend.plan_sample(mean, std, eps.to(device), best_cond, None, None, cand, N, B, T)
        cost = RF.distance_cost(cand, target, N, B)
        col = cost.cpu()
        win = [min(range(N), key=lambda n: (float(col[n, b]), n)) for b in range(B)]
        best_cond = torch.stack([cand.view(T, N, B, cd)[:, win[b], b] for b in range(B)]).contiguous()
        backend.plan_refit(cost, cand, mean, std, mean, std, None, None, K, N, B, T, 0.0, 0.0)
        assert same_bits(mean, want[i][0]), (i, dirty.first_diff(mean, want[i][0]))
        assert ulps(std, want[i][1]) <= 1, i


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def call_kw(name, device, iterations=None, **over):
    B, N, K, T, I = RF.CASES[name][:5]
    inputs, goal, mean, std, bounds, _ = RF.request(name)
    kw = dict(x=dev_list(inputs[:2], device), pose=inputs[2].to(device), steps=T, goal=dev_list(goal, device), init_mean=mean.to(device),
              init_std=std.to(device), candidates=N, elites=K, iterations=I if iterations is None else iterations,
              bounds=None if bounds is None else tuple(b.to(device) for b in bounds), **KW)
    kw.update(over)
    return kw


def ask(eng, name, device, iterations=None, latent=None, **over):
    """One plan_refine() call of a case on the case's injected candidate draws; ``latent``: the [B, L] draws of sample=True, one per
    step and iteration, interleaved behind each iteration's candidate block."""
    T, I = RF.CASES[name][3], RF.CASES[name][4] if iterations is None else iterations
    draws = [d.clone() for d in RF.request(name)[5][:I]]
    if latent is not None:
        draws = [x for i in range(I) for x in [draws[i]] + [e.clone() for e in latent[i * T:(i + 1) * T]]]
    eng.noise = InjectedNoise(draws, [])
    r = keep(eng.plan_refine(**call_kw(name, device, iterations, sample=latent is not None, **over)))
    assert not eng.noise._eps
    return r


def rollout_of(eng, name, device, **over):
    """``plan_rollout`` of the case's request for given per-row candidates, as the host loop of refine_cases.chain calls it."""
    kw = call_kw(name, device, **over)
    for k in ("init_mean", "init_std", "candidates", "elites", "iterations", "bounds"):
        kw.pop(k)
    return lambda cand: cpu(keep(eng.plan_rollout(candidates=cand.to(device), **kw)))


def check_chain(device, name):
    """plan_refine against the chain of existing requests -- per iteration the restated candidates, one plan_rollout, the restated
    refit --, bit for bit, eager."""
    B, N, K, T, I = RF.CASES[name][:5]
    eng = MVAEInference(PC.build(False, device), use_graph=False)
    r = cpu(ask(eng, name, device))
    assert set(r) == KEYS
    assert tuple(r["mean"].shape) == (B, T, CD) == tuple(r["std"].shape) and tuple(r["candidates"].shape) == (T, N, B, CD)
    assert tuple(r["history"].shape) == (I, B) == tuple(r["elite_count"].shape) and r["elite_count"].dtype == torch.int32
    want = RF.chain(rollout_of(eng, name, device), name)
    pairs = [("candidates", r["candidates"].reshape(T, N * B, CD), want["candidates"])]
    pairs += [(k, r[k], want[k]) for k in ("cost", "step_cost", "best", "best_cost", "best_condition", "mean", "history", "elite_count")]
    pairs += [(f"trajectory {m}", r["trajectory"][m], want["trajectory"][m]) for m in range(3)]
    print(name, "against the chain: bit-equal", {k: same_bits(a, b) for k, a, b in pairs}, "std ulps", ulps(r["std"], want["std"]))
    for k, a, b in pairs:
        assert same_bits(a, b), (name, k, dirty.first_diff(a, b))
    assert ulps(r["std"], want["std"]) <= 1
    assert torch.equal(r["history"][I - 1], r["best_cost"]) and r["elite_count"].tolist() == [[K] * B] * I
    eng.close()
    return r


def check_incumbent(device, name):
    """Slot 0 of the last iteration's candidates is the best_condition of the same request run with one iteration less."""
    B, N, K, T, I = RF.CASES[name][:5]
    eng = MVAEInference(PC.build(False, device), use_graph=False)
    full, short = ask(eng, name, device), ask(eng, name, device, iterations=I - 1)
    assert same_bits(full["candidates"][:, 0].transpose(0, 1), short["best_condition"])
    assert same_bits(full["history"][:I - 1], short["history"])
    eng.close()


def check_history(device, name):
    """The winner of an iteration is a candidate of the next one (slot 0), so the best cost does not rise -- beyond what one
    candidate costs in another slot: REL, the bound of the horizon tests' permuted candidates."""
    eng = MVAEInference(PC.build(False, device), use_graph=False)
    h = ask(eng, name, device)["history"].double().cpu()
    print(name, "history", h.tolist())
    assert bool((h > 0).all()) and bool((h[1:] <= h[:-1] * (1.0 + REL)).all()), h
    eng.close()


def check_mixed_request(device):
    """The mixed start with a per-step goal_available: NaN planted in the absent goal rows reaches nothing."""
    B, N, K, T, I = RC.BATCH, 3, 2, 2, 2
    eng = MVAEInference(PC.build(False, device), use_graph=False)
    inputs, av = RC.start()
    goal, gav = RC.frames(1402, T, B), RC.mixed_table(8, T, B)
    g = torch.Generator().manual_seed(16)
    mean, std = torch.rand(T, CD, generator=g), 0.1 + 0.1 * torch.rand(B, T, CD, generator=g)
    draws = [torch.randn(N, B, T, CD, generator=g) for _ in range(I)]

    def call(gl):
        eng.noise = InjectedNoise([d.clone() for d in draws], [])
        return cpu(keep(eng.plan_refine(dev_list(inputs[:2], device), pose=inputs[2].to(device), steps=T, goal=dev_list(gl, device),
                                        init_mean=mean, init_std=std, candidates=N, elites=K, iterations=I, available=av,
                                        goal_available=gav, **KW)))
    r = call(goal)
    on = gav != 0
    for m, k in enumerate(E.TERMS[:3]):
        assert float(r[k].transpose(1, 2)[~on[:, :, m]].abs().sum()) == 0.0 and float(r[k].transpose(1, 2)[on[:, :, m]].min()) > 0.0, k
    E.check_own_tables(r, None)
    dirty_goal = [x.clone() for x in goal]
    for m in range(3):
        dirty_goal[m][~on[:, :, m]] = nan
    r2 = call(dirty_goal)
    for k in ("cost", "best", "history", "mean", "std", "candidates") + E.TERMS:
        assert same_bits(r[k], r2[k]) and bool(torch.isfinite(r2[k].double()).all()), k
    eng.close()


def check_problem_layer(device, root):
    """DynModeling.plan_refine on a batch of the synthetic tree: the default distribution and bounds are those of the batch's own
    recorded shock sequences, the engine beside it gives the same bits, the refusals."""
    data, target, l = E.tree_batch(root, device)
    n = data[0].shape[0] // l
    model = PC.build(False, device)
    prob = TMM.problem_of(model, "cnn-mvae", True, device, DynModeling)
    prob._seq_length, prob._kl_weight, prob._pose_multiplier = l, E.HC.KL_WEIGHT, E.HC.POSE_MULTIPLIER
    N, K, I = 4, 2, 2
    draws = [torch.randn(N, n, l, CD, generator=torch.Generator().manual_seed(60 + i)) for i in range(I)]
    model.train()
    res = prob.plan_refine(data, target, candidates=N, elites=K, iterations=I)            # the engine's own Philox stream
    assert model.training
    model.eval()
    assert set(res) == KEYS | {"recorded"}
    rec = data[4].reshape(n, l, -1)
    assert torch.equal(res["recorded"].cpu(), rec) and tuple(res["mean"].shape) == (n, l, CD) and tuple(res["history"].shape) == (I, n)
    lo, hi = rec.reshape(-1, CD).min(0).values, rec.reshape(-1, CD).max(0).values
    c = res["candidates"].cpu()
    assert bool((c >= lo).all()) and bool((c <= hi).all())
    prob._refiner.use_graph = False                                     # (given draws cannot be replayed by a captured graph)
    prob._refiner.noise = InjectedNoise([d.clone() for d in draws], [])
    res = prob.plan_refine(data, target, candidates=N, elites=K, iterations=I)
    fr = lambda t: t.reshape((n, l) + tuple(t.shape[1:]))
    goal = [torch.cat((fr(data[m])[:, 1:].transpose(0, 1), target[m][l - 1::l].unsqueeze(0).to(data[m].dtype))).to(device) for m in range(3)]
    gav = torch.cat((torch.cat((fr(data[3])[:, 1:].transpose(0, 1).float(), torch.ones(1, n, 2))), torch.ones(l, n, 1)), 2)
    eng = MVAEInference(model, use_graph=False)
    eng.noise = InjectedNoise([d.clone() for d in draws], [])
    want = eng.plan_refine([data[0][::l].to(device), data[1][::l].to(device)], pose=data[2][::l].to(device), steps=l, goal=goal,
                           init_mean=rec.mean(0), init_std=rec.std(0, unbiased=False), candidates=N, elites=K, iterations=I,
                           bounds=(lo, hi), available=data[3][::l].to(device), goal_available=gav, **KW)
    assert same_bits(res["candidates"], want["candidates"]) and same_bits(res["mean"], want["mean"])
    np.testing.assert_allclose(res["cost"].cpu().numpy(), want["cost"].cpu().numpy(), rtol=REL)
    eng.close()
    prob._refiner.noise = InjectedNoise([torch.randn(3, n, 2, CD, generator=torch.Generator().manual_seed(70))], [])
    short = prob.plan_refine(data, target, steps=2, candidates=3, elites=1, iterations=1, init_mean=torch.zeros(2, CD),
                             init_std=torch.ones(n, 2, CD), bounds=(torch.zeros(CD), torch.ones(CD)))
    assert tuple(short["candidates"].shape) == (2, 3, n, CD) and tuple(short["recorded"].shape) == (n, 2, CD)
    prob._refiner.close()
    for bad in (0, l + 1, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            prob.plan_refine(data, target, steps=bad)
    with pytest.raises(ValueError, match="shock"):
        prob.plan_refine(data[:4], target)
    with pytest.raises(ValueError, match="whole sequences"):
        prob.plan_refine([t[:-1] for t in data], target)
    import avail_cases as A
    plain = TMM.problem_of(setup_model("cnn-mvae", cross_modal=True, **A.PLAIN_KW).to(device).eval(), "cnn-mvae", False, device, DynModeling)
    plain._seq_length = l
    with pytest.raises(ValueError, match="unconditional"):
        plain.plan_refine(data, target)
    vae = TMM.problem_of(model, "cnn-vae", True, device, DynModeling)
    vae._seq_length = l
    with pytest.raises(ValueError, match="cnn-vae"):
        vae.plan_refine(data, target)


# ---- the CPU suite -------------------------------------------------------------------------------------------------------------
SAMPLE_SHAPES = [(1, 1, 1, 1, 0), (5, 9, 3, 3, 0), (3, 2, 2, 4, 0), (300, 2, 2, 2, 0), (3, 2, 2, 4, 1)]
# (the last three: K == N, where nothing is ranked -- N = one walk group of eight and a tail of one, two groups and a tail, one group)
REFIT_SHAPES = [(1, 1, 1, 1, 1), (5, 9, 3, 3, 3), (2, 300, 40, 2, 2), (3, 4096, 64, 1, 1), (2, 9, 9, 2, 3), (2, 17, 17, 1, 4),
                (3, 8, 8, 2, 1)]


@pytest.mark.parametrize("B,N,T,cd,shift", SAMPLE_SHAPES)
def test_sample_exact(B, N, T, cd, shift):
    check_sample_exact(EmuBackendRefine(), "cpu", B, N, T, cd, shift)


def test_sample_on_dirty_destinations():
    check_sample_dirty(EmuBackendRefine(), "cpu")


def test_refit_rules():
    check_refit_rules(EmuBackendRefine(), "cpu")


@pytest.mark.parametrize("B,N,K,T,cd", REFIT_SHAPES)
def test_refit_against_the_restatement(B, N, K, T, cd):
    check_refit_restatement(EmuBackendRefine(), "cpu", B, N, K, T, cd)


@pytest.mark.parametrize("B,N,K", [(5, 9, 3), (3, 40, 8), (1, 2, 1)])
def test_refit_elites_are_the_top_list(B, N, K):
    check_refit_is_top(EmuBackendRefine(), "cpu", B, N, K)


def test_refit_on_dirty_destinations():
    check_refit_dirty(EmuBackendRefine(), "cpu")


def test_loop_without_the_model():
    check_loop(EmuBackendRefine(), "cpu")


@pytest.mark.parametrize("name", list(RF.CASES))
def test_equal_to_the_chain_of_existing_requests(name):
    check_chain("cpu", name)


@pytest.mark.parametrize("name", ["steps", "one"])
def test_incumbent(name):
    check_incumbent("cpu", name)


@pytest.mark.parametrize("name", list(RF.CASES))
def test_history_does_not_rise(name):
    check_history("cpu", name)


def test_mixed_request_and_absent_goal_terms():
    check_mixed_request("cpu")


def test_problem_layer(tmp_path):
    check_problem_layer("cpu", tmp_path)


# ---- emulation only ------------------------------------------------------------------------------------------------------------
def test_hip_backend_validates_on_the_host():
    """HipBackend.plan_sample / plan_refit check shapes, dtypes, ranges and overlaps before they touch the library, and refuse CPU
    tensors."""
    hip = ops.HipBackend()
    N, B, T, cd, K = 4, 3, 2, 3, 2
    f = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    smp = lambda **k: dict(dict(mean=f(B, T, cd), std=f(B, T, cd), eps=f(N, B, T, cd), keep=None, lo=None, hi=None, cand=f(T, N * B, cd),
                                N=N, B=B, T=T), **k)
    big = f(T * N * B * cd + B * T * cd)
    for k in (smp(mean=None), smp(cand=None), smp(lo=f(cd)), smp(hi=f(cd)), smp(mean=f(T, B, cd)), smp(std=f(B, T, cd + 1)),
              smp(eps=f(B, N, T, cd)), smp(eps=f(N, B, T, cd, dtype=torch.float64)), smp(keep=f(B, T)), smp(lo=f(cd + 1), hi=f(cd + 1)),
              smp(cand=f(N * B, T, cd)), smp(cand=f(T, N * B, 2 * cd)[:, :, ::2]), smp(N=0), smp(B=0), smp(T=0), smp(mean=f(B, T)),
              smp(cand=big[:T * N * B * cd].view(T, N * B, cd), mean=big[T * N * B * cd - 1:][:B * T * cd].view(B, T, cd))):
        with pytest.raises(ValueError):
            hip.plan_sample(**k)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.plan_sample(**smp())
    i32, u8 = torch.int32, torch.uint8
    fit = lambda **k: dict(dict(cost=f(N, B), cand=f(T, N * B, cd), mean_in=f(B, T, cd), std_in=f(B, T, cd), mean_out=f(B, T, cd),
                                std_out=f(B, T, cd), elite=f(N, B, dtype=u8), count=f(B, dtype=i32), K=K, N=N, B=B, T=T, alpha=0.5,
                                std_min=0.0), **k)
    two = f(2 * B * T * cd)
    shared = f(B, T, cd)
    for k in (fit(cost=None), fit(mean_out=None), fit(cost=f(B, N)), fit(cost=f(N, B, dtype=torch.float64)), fit(cand=f(T, N * B)),
              fit(mean_in=f(B, T, cd + 1)), fit(std_out=f(T, B, cd)), fit(elite=f(N, B)), fit(count=f(B, dtype=torch.int64)),
              fit(count=f(B + 1, dtype=i32)), fit(K=0), fit(K=N + 1), fit(N=0), fit(N=4097, cost=f(4097, B), cand=f(T, 4097 * B, cd),
                                                                                  elite=None), fit(B=0), fit(T=0),
              fit(alpha=1.0), fit(alpha=-0.1), fit(alpha=nan), fit(std_min=-1.0), fit(std_min=nan),
              fit(mean_in=two[:B * T * cd].view(B, T, cd), mean_out=two[cd:cd + B * T * cd].view(B, T, cd)),      # a partial overlap
              fit(mean_in=shared, std_out=shared), fit(mean_out=shared, std_out=shared), fit(std_in=shared, mean_out=shared)):
        with pytest.raises(ValueError):
            hip.plan_refit(**k)
    for k in (fit(), fit(mean_in=shared, mean_out=shared), fit(elite=None, count=None)):    # valid: only the CPU tensors are refused
        with pytest.raises(RuntimeError, match="GPU tensors"):
            hip.plan_refit(**k)


def recorded(fn, backend=None, quiet=()):
    rec = ShapeRecorder(backend or EmuBackendRefine())
    old = ops.set_backend(rec)
    eng = MVAEInference(PC.build(False), use_graph=False)
    del rec.ops[:], rec.sigs[:]                                         # (the weights are packed when the engine is built)
    try:
        fn(eng)
    finally:
        ops.set_backend(old)
        eng.close()
    return [s for s in rec.sigs if s[0] not in quiet]


def refine_kw(N, K, I, T, every, seed=5):
    kw = E.request_kw(N, T, every, seed)
    kw.pop("candidates")
    g = torch.Generator().manual_seed(seed)
    return dict(kw, init_mean=torch.rand(T, CD, generator=g), init_std=0.1 + torch.rand(T, CD, generator=g), candidates=N, elites=K,
                iterations=I)


def test_launch_accounting():
    """The recorded calls, by name and shapes: the trunks and the pose heads once; per iteration one random_normal (and its commit),
    one plan_sample, the launches of plan_rollout from the image heads on, one plan_select_steps, one plan_refit; one
    gather_best_steps in total; no plan_select, gather_best or assembly launch."""
    B = RC.BATCH
    for N, K, I, T, every in ((1, 1, 1, 1, True), (3, 2, 2, 2, True), (9, 3, 3, 2, False)):
        kw = refine_kw(N, K, I, T, every)
        got = recorded(lambda e: e.plan_refine(**kw))
        names = [s[0] for s in got]
        trunks = recorded(lambda e: e._run(("t",), lambda *a: e._trunks(*a), [kw["x"][0], kw["x"][1], kw["pose"]]))
        pr_kw = {k: v for k, v in kw.items() if k not in ("init_mean", "init_std", "candidates", "elites", "iterations")}
        rollout = recorded(lambda e: e.plan_rollout(candidates=torch.rand(N, T, CD), **pr_kw), quiet=("random_normal", "counter_add"))
        assert [s[0] for s in rollout[-2:]] == ["plan_select_steps", "gather_best_steps"]
        steps = list(rollout[:-2])
        for s in trunks:                                                 # what plan_rollout runs from the image heads on
            steps.remove(s)
        assert "concat_condition_tiled" in [s[0] for s in steps] and len(steps) == len(rollout) - 2 - len(trunks)
        assert got[:len(trunks)] == trunks and not any(n in ("random_normal", "plan_sample") for n in [s[0] for s in trunks])
        per = (len(got) - len(trunks) - 1) // I
        assert len(trunks) + I * per + 1 == len(got) and names[-1] == "gather_best_steps"
        for i in range(I):
            block = got[len(trunks) + i * per:len(trunks) + (i + 1) * per]
            assert [s[0] for s in block[:3]] == ["random_normal", "counter_add", "plan_sample"], block[:3]
            assert block[0][1][0] == (N, B, T, CD)
            assert [s[0] for s in block[-2:]] == ["plan_select_steps", "plan_refit"]
            assert block[3:-2] == steps, (N, I, i)
        count = lambda n: names.count(n)
        assert count("random_normal") == count("plan_sample") == count("plan_select_steps") == count("plan_refit") == I
        assert count("gather_best_steps") == 1 and count("rollout_feed") == I * T
        assert not {"plan_select", "gather_best", "complete_select"} & set(names) and not any(n.startswith("elbo_assemble") for n in names)
    # sample=True: one [B][L] draw per step and iteration behind the candidate block
    kw = refine_kw(3, 2, 2, 2, True)
    draws = [s[1][0] for s in recorded(lambda e: e.plan_refine(sample=True, **kw)) if s[0] == "random_normal"]
    assert draws == [(3, B, 2, CD), (B, E.L), (B, E.L)] * 2


def test_existing_requests_record_what_they_recorded():
    """plan, rollout, plan_rollout, forward and score on a backend without the new ops record what they record with them, and the
    golden serving trace of the earlier requests is still what tests/test_serving_trace_emu.py pins."""
    B = RC.BATCH
    kw = E.request_kw(3, 2, True)
    x, pose, goal = kw["x"], kw["pose"], kw["goal"]
    cond = kw["candidates"][0, 0].expand(B, -1).contiguous()
    calls = (lambda e: e.plan(x, pose=pose, goal=[g[0] for g in goal], candidates=kw["candidates"][:, 0], **KW),
             lambda e: e.rollout(x, pose=pose, steps=2, condition=cond, targets=goal, **KW),
             lambda e: e.plan_rollout(**kw), lambda e: e.forward(x, pose=pose, condition=cond),
             lambda e: e.score(x, pose=pose, condition=cond))
    for call in calls:
        assert recorded(call) == recorded(call, backend=EmuBackendHorizon())
    import importlib.util
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_serving_trace", os.path.join(golden, "make_serving_trace.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    with open(os.path.join(golden, "serving_trace.json")) as f:
        trace = json.load(f)
    assert M.compare(trace, M.digested(M.record())) == []


def test_argument_errors_and_graph_keys():
    """The refusals, and what the graph key carries: I, N, K, T, the goal's form, ``sample``, alpha, std_min, the pose multiplier,
    the presence of bounds and the shapes -- never values."""
    eng = MVAEInference(PC.build(False), use_graph=False)
    B, T, cd = RC.BATCH, 2, CD
    kw = refine_kw(3, 2, 2, T, True)
    bad = lambda **k: dict(kw, **k)
    for k, values in (("candidates", (0, 4097, 1.5, True, None)), ("elites", (0, 4, 1.5, True)), ("iterations", (0, -1, 2.5, True)),
                      ("steps", (0, 1.5, True, None)), ("alpha", (1.0, -0.5, nan, "a", True, 1.0 - 1e-12)), ("std_min", (-1.0, nan, None))):
        for v in values:
            with pytest.raises(ValueError, match=k):
                eng.plan_refine(**bad(**{k: v}))
    for k in ("init_mean", "init_std"):
        for t in (None, torch.zeros(T, cd + 1), torch.zeros(T + 1, cd), torch.zeros(B + 1, T, cd), torch.zeros(cd), torch.zeros(T, cd, dtype=torch.int64),
                  [[0.0] * cd] * T):
            with pytest.raises(ValueError, match=k):
                eng.plan_refine(**bad(**{k: t}))
    lo, hi = torch.zeros(cd), torch.ones(cd)
    for b in (lo, (lo,), (lo, hi, hi), (lo, torch.ones(cd + 1)), (lo, None), (lo.long(), hi.long()), (0.0, 1.0)):
        with pytest.raises(ValueError, match="bounds"):
            eng.plan_refine(**bad(bounds=b))
    v, t, p = kw["goal"]
    for g in (None, [None, None, None], [v[:, :2], None, None], v):
        with pytest.raises(ValueError, match="goal"):
            eng.plan_refine(**bad(goal=g))
    with pytest.raises(ValueError, match="mixes the two forms"):
        eng.plan_refine(**bad(goal=[v, t[0], None]))
    with pytest.raises(ValueError, match="step_weight"):
        eng.plan_refine(**bad(step_weight=torch.ones(T + 1)))
    with pytest.raises(ValueError, match="goal_available"):
        eng.plan_refine(**bad(goal_available=torch.ones(B, 3)))
    with pytest.raises(ValueError, match="modality"):
        eng.plan_refine(**bad(x=[None, None], pose=None))
    long = 32                                                           # a horizon at which the trajectory tensor reaches 2^31 below N = 4096
    most = min((2 ** 31 - 1) // (long * B * 3 * 64 * 64), (2 ** 31 - 1) // (B * 32 * 32 * 32))
    assert most < 4096
    with pytest.raises(ValueError, match=rf"largest N for B = {B} and steps = {long} is {most}\b"):
        eng.plan_refine(**bad(steps=long, candidates=most + 1, goal=[v[0], None, None], init_mean=torch.zeros(long, cd),
                              init_std=torch.ones(long, cd)))
    # a backend written before the ops: an error that names one of them, before anything is launched
    ops.set_backend(EmuBackendHorizon())
    with pytest.raises(RuntimeError, match="plan_sample"):
        eng.plan_refine(**kw)
    ops.set_backend(EmuBackendRefine())
    eng.close()
    cat = MVAEInference(PC.build(True), use_graph=False)
    with pytest.raises(ValueError, match="categorical"):
        cat.plan_refine(**kw)
    cat.close()
    import avail_cases as A
    plain = MVAEInference(setup_model("cnn-mvae", cross_modal=True, **A.PLAIN_KW).eval(), use_graph=False)
    with pytest.raises(ValueError, match="unconditional model"):
        plain.plan_refine(**kw)
    plain.close()
    eng = MVAEInference(PC.build(False), use_graph=False)
    keys = []
    eng._run = lambda key, fn, args: keys.append(key)
    w = torch.tensor([1.0, 2.0])
    calls = [kw, bad(init_mean=kw["init_mean"] + 1.0), bad(init_std=kw["init_std"].expand(B, T, cd) * 2.0), bad(kl_weight=2.0),    # values
             bad(bounds=(lo, hi)), bad(bounds=(lo - 1.0, hi + 1.0)),                                                             # ... again
             bad(step_weight=w), bad(candidates=4), bad(elites=1), bad(iterations=3), bad(sample=True), bad(alpha=0.5), bad(std_min=0.1),
             bad(pose_multiplier=10.0), bad(goal=[g[1] for g in kw["goal"]]),
             bad(steps=3, goal=RC.frames(1, 3, B), init_mean=torch.zeros(3, cd), init_std=torch.ones(3, cd))]
    for c in calls:
        eng.plan_refine(**c)
    assert keys[0] == keys[1] == keys[2] == keys[3] and keys[4] == keys[5] != keys[0]
    assert len(set(keys)) == len(calls) - 4
    assert all(k[0] == "plan_refine" for k in keys)
