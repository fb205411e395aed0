"""The horizon planner on a real MI355X: mmdyn_plan_select_steps against its rules, its fp64 restatement and mmdyn_plan_select,
mmdyn_gather_best_steps against T mmdyn_gather_best calls (bit for bit), both on dirty destinations and with every refused argument;
then ``MVAEInference.plan_rollout`` -- the checks of tests/test_horizon_emu.py on the HIP library, captured against eager on one Philox
stream with new candidates, step weights and KL weight per replay, dirty allocator memory -- and ``DynModeling.plan_rollout``.  The
reference has no such operation: nothing here comes from a golden file."""
import ctypes

import numpy as np
import pytest
import torch

import cond_cases as CC
import dirty
import horizon_cases as HC
import philox_ref as P
import plan_cases as PC
import rollout_cases as RC
import test_horizon_emu as E
from mmdyn_hip import _lib, engine, layers, ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from test_elbo_rows_gpu import RTOL_SUM          # (that file's constant, not a new one)
from test_noise_gpu import NORMAL_TOL
from test_plan_gpu import SIGMOID_ATOL, gen

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
L = HC.L


# ---- plan_select_steps --------------------------------------------------------------------------------------------------------
def test_select_rules():
    E.check_select_rules(HIP, DEV)


@pytest.mark.parametrize("B,N", [(1, 1), (5, 9), (300, 2)])
def test_one_scored_step_is_plan_select(B, N):
    E.check_one_step_is_plan_select(HIP, DEV, B, N)


def test_total_is_not_contracted():
    E.check_total_is_not_contracted(HIP, DEV)


@pytest.mark.parametrize("B,N,T", [(1, 1, 1), (5, 9, 3), (300, 2, 2)])
def test_select_against_the_restatement(B, N, T):
    E.check_select_restatement(HIP, DEV, B, N, T)


def test_select_on_dirty_destinations_and_bad_arguments():
    N, B, T = 3, 5, 2
    bce, mse, kl = HC.random_tables(B, N, T, 7)
    tab = torch.ones(T, B, 4, dtype=torch.uint8)
    tab[0, 1, 0] = tab[1, 3, 2] = 0
    args = (bce, mse, kl, tab, torch.tensor([0.5, 1.5]), gen(3, T, N * B, 2), torch.empty(N, B), torch.empty(T, N, B),
            torch.empty(B, dtype=torch.int32), torch.empty(B), torch.empty(B, T, 2), torch.empty(4, B, dtype=torch.int32), torch.empty(4, B),
            N, B, T, T, 1000.0, 0.3)
    runs = dirty.run_dirty(HIP, "plan_select_steps", args, outs=[6, 7, 8, 9, 10, 11, 12], state=[0, 1], device=DEV)
    assert bool(torch.isnan(runs[dirty.ZERO]["top_cost"][3]).all()) and runs[dirty.ZERO]["top"][3].tolist() == [-1] * B      # K = 4 > N
    for got in runs.values():           # (the one documented NaN: the list's entries past the N candidates)
        got["top_cost"] = got["top_cost"][:N]
    dirty.assert_same_bits(runs, what="plan_select_steps: ")
    lib, t = HIP.lib, torch.zeros(256, device=DEV)
    p = t.data_ptr()

    def f(kl=p, tav=None, w=None, cand=p, idx=None, cost=p, sc=p, best=p, bc=p, cond=p, bidx=None, top=None, tc=None, K=0, N=1, B=1,
          T=1, Tg=1, cd=1):
        return lib.mmdyn_plan_select_steps(None, None, kl, tav, w, cand, idx, cd, cost, sc, best, bc, cond, bidx, top, tc, K, N, B, T, Tg,
                                           1.0, 1.0, None, None)
    assert f(kl=None) == -2 and f(cost=None) == -2 and f(sc=None) == -2 and f(best=None) == -2 and f(bc=None) == -2
    assert f(cand=None, cond=None) == -2 and f(idx=p, bidx=p) == -2 and f(cond=None) == -2 and f(cand=None, cond=None, idx=p) == -2
    assert f(top=p, K=1) == -2 and f(tc=p, K=1) == -2
    assert f(N=0) == -1 and f(B=0) == -1 and f(T=0) == -1 and f(Tg=0) == -1 and f(cd=0) == -1 and f(tav=p + 1) == -1
    assert f(T=3, Tg=2) == -1 and f(T=1, Tg=3) == -1
    assert f(top=p, tc=p, K=0) == -1 and f(top=p, tc=p, K=9) == -1
    assert f(N=65536, B=32768) == -3 and f(T=2, Tg=2, N=32768, B=32768) == -3
    torch.cuda.synchronize()


# ---- gather_best_steps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_lens,B,N,T,shift", [((48, 48, 7), 5, 3, 3, 0), ((12288, 12288, 7), 2, 2, 2, 0), ((12, 12), 3, 3, 2, 1)])
def test_gather_steps_is_gather_best_per_step(row_lens, B, N, T, shift):
    E.check_gather_steps(HIP, DEV, row_lens, B, N, T, shift)


@pytest.mark.parametrize("row_lens,B,N,T,shift", [((48, 48, 7), 5, 3, 3, 0), ((12, 12), 3, 3, 2, 1)])
def test_gather_steps_is_complete_select_on_the_picked_rows(row_lens, B, N, T, shift):
    """The independent form of the check above (one kernel serves both gather entries, so that one compares it with itself): every
    step of every group against mmdyn_complete_select(x = null) on the rows a torch index picks from src[t] -- the same bits in
    every taken row; a row with best = -1 or best = N is all NaN in every step."""
    best = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(7 + B)).to(torch.int32)
    best[1], best[B - 1] = -1, N
    best = best.to(DEV)
    taken = (best >= 0) & (best < N)
    rows = torch.where(taken, best.long(), torch.zeros_like(best).long()) * B + torch.arange(B, device=DEV)
    groups = [dict(src=(3.0 * gen(970 + g, T, N * B, n)).to(DEV), out=E.shifted(DEV, (T, B, n), shift), logits=g == 1)
              for g, n in enumerate(row_lens)]
    HIP.gather_best_steps(groups, best, N, B, T)
    assert int(taken.sum()) >= 1
    for g in groups:
        for t in range(T):
            want = torch.empty(B, g["src"].shape[2], device=DEV)
            HIP.complete_select(None, g["src"][t][rows], None, 0, want, g["logits"])
            diff = dirty.first_diff(g["out"][t][taken], want[taken])
            assert diff is None, (t, diff)
            assert bool(torch.isfinite(g["out"][t][taken]).all()) and bool(torch.isnan(g["out"][t][~taken]).all())


def test_gather_steps_on_dirty_destinations_and_bad_arguments():
    B, N, T, row_lens = 5, 3, 3, (48, 48, 7)
    best = torch.tensor([2, 0, 1, 0, 2], dtype=torch.int32)

    def gather(backend, s0, s1, s2, d0, d1, d2, bst):
        backend.gather_best_steps([dict(src=s, out=d, logits=g == 1) for g, (s, d) in enumerate(zip((s0, s1, s2), (d0, d1, d2)))], bst,
                                  N, B, T)
    args = tuple(gen(960 + g, T, N * B, n) for g, n in enumerate(row_lens)) + tuple(torch.empty(T, B, n) for n in row_lens) + (best,)
    dirty.assert_same_bits(dirty.run_dirty(HIP, gather, args, outs=[3, 4, 5], device=DEV), what="gather_best_steps: ")
    lib, t = HIP.lib, torch.zeros(2048, device=DEV)
    p, ip = t.data_ptr(), torch.zeros(8, dtype=torch.int32, device=DEV).data_ptr()

    def call(G=1, N=2, Bk=1, T=2, best=ip, **over):
        """src [T = 2][N = 2][4] = 64 bytes at p, out [T = 2][1][4] = 32 bytes at p + 4096 unless overridden."""
        a = _lib.GatherGroups()
        for g in range(4):
            a.src[g], a.out[g], a.row_len[g], a.logits[g] = p, p + 4096, 4, 0
        for k, (g, v) in over.items():
            getattr(a, k)[g] = v
        return lib.mmdyn_gather_best_steps(ctypes.addressof(a), G, best, N, Bk, T, None)
    assert lib.mmdyn_gather_best_steps(None, 1, ip, 1, 1, 1, None) == -2 and call(best=None) == -2
    assert call(src=(0, None)) == -2 and call(G=2, out=(1, None)) == -2
    assert call(G=0) == -1 and call(G=5) == -1 and call(Bk=0) == -1 and call(N=0) == -1 and call(T=0) == -1 and call(row_len=(0, 0)) == -1
    assert call() == 0
    # out inside the T * N * B source rows -- the second step's rows included -- or over the indices
    assert call(out=(0, p)) == -1 and call(out=(0, p + 32)) == -1 and call(out=(0, p + 60)) == -1 and call(out=(0, p + 64)) == 0
    assert call(out=(0, ip)) == -1
    # two groups: an out may touch neither the other group's source rows nor its out (all T steps of either)
    assert call(G=2, src=(1, p + 512), out=(1, p + 6144)) == 0
    assert call(G=2, src=(1, p + 512), out=(1, p + 16)) == -1 and call(G=2, src=(1, p + 6144 - 16), out=(1, p + 6144)) == -1
    assert call(G=2, src=(1, p + 512)) == -1 and call(G=2, src=(1, p + 512), out=(1, p + 4096 + 16)) == -1
    assert call(G=2, src=(1, p + 4096 - 16), out=(1, p + 6144)) == -1
    assert call(N=32768, T=2, row_len=(0, 32768)) == -3
    assert call(src=(1, None)) == 0                                             # groups past G are not looked at
    torch.cuda.synchronize()


# ---- the engine ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    """What stands behind the decoders inherits their fp32 summation order: the bound this suite puts on such sums."""
    return torch.allclose(a.double(), b.double(), rtol=RTOL_SUM, atol=0.0)


@pytest.mark.parametrize("name,sample", [("steps", True), ("final", False), ("classes", False), ("nine", False)])
def test_one_step_consistency(name, sample):
    E.check_one_step_consistency(DEV, name, sample, sigmoid_atol=SIGMOID_ATOL)


@pytest.mark.parametrize("name", list(HC.CASES))
def test_choice_against_the_chained_oracle(name):
    E.check_choice(DEV, name)


@pytest.mark.parametrize("sample", [False, True])
def test_one_step_is_plan(sample):
    E.check_one_step_is_plan(DEV, sample)


def test_one_candidate_is_rollout():
    E.check_one_candidate_is_rollout(DEV)


def test_permuted_candidates():
    E.check_permutation(DEV)


def test_mixed_request_and_absent_goal_terms():
    E.check_mixed_request(DEV)


def test_problem_layer(tmp_path):
    E.check_problem_layer(DEV, tmp_path)


def test_captured_equals_eager_on_one_philox_stream():
    """14. use_graph=True against an eager engine with the same seed: three calls with new inputs, new candidate VALUES, new step
    weights and, at the third, a new KL weight -- all static inputs of ONE graph, whose key carries N, T, the kind and the goal's
    form.  Draw accounting: sample=True takes one [B, L] block per step, n = counters_of(B L) counters each; the capture's eager
    warm-up takes the first T blocks, so replay c is compared with eager call c + 1.  means / log_var of step 0 stand in front of
    every decoder: equal bit for bit; everything later stands behind the decoders: OUT_TOL for the posteriors and states, RTOL_SUM
    for the tables; ``best`` equal under the gap condition.  The draws are tied to tests/philox_ref.py through ``means``: means[1]
    is a function of step 0's draw, so a request with the reference's numbers INJECTED at the accounted counters gives the engine's
    means within OUT_TOL, the numbers of the next call's blocks give means further away than 100 x the tolerance."""
    name, seed = "steps", 5
    B, N, T, categorical = HC.CASES[name][:4]
    n = P.counters_of(B * L)
    assert NORMAL_TOL < 1e-4
    model = PC.build(categorical, DEV)
    from mmdyn_hip.utils.seeded_init import seeded_batch
    xs = [E.dev_list(seeded_batch(B, 1600 + c, with_pose=True)[0], DEV) for c in range(3)]
    goals = [E.dev_list(RC.frames(1610 + c, T, B), DEV) for c in range(3)]
    cands = [torch.rand(N, T, CC.REAL_DIM, generator=torch.Generator().manual_seed(1620 + c)).to(DEV) for c in range(3)]
    steps_w = [torch.tensor(w) for w in ((1.0, 1.0), (0.5, 1.0), (1.0, 0.25))]
    weights = (0.3, 0.3, 2.0)
    call = lambda eng, c, **k: E.keep(eng.plan_rollout(xs[c][:2], pose=xs[c][2], steps=T, goal=goals[c], candidates=cands[c], top=2,
                                                       step_weight=steps_w[c], sample=True, kl_weight=weights[c],
                                                       pose_multiplier=HC.POSE_MULTIPLIER, **k))
    eager = MVAEInference(model, seed=seed, use_graph=False)
    e = [call(eager, c) for c in (0, 0, 1, 2)]
    graph = MVAEInference(model, seed=seed)
    assert graph.use_graph
    g = [call(graph, c) for c in range(3)]
    assert len(graph._graphs) == 1
    key = next(iter(graph._graphs))
    assert key[0] == "plan_rollout" and ("candidates", N, False) in key and "real" in key and key[1:3] == (T, T)
    tol = E.OUT_TOL
    for c in range(3):
        a, b = g[c], e[c + 1]
        assert torch.equal(a["means"][0], b["means"][0]) and torch.equal(a["log_var"][0], b["log_var"][0]), c
        print("replay", c, "bit-equal to eager:", {k: bool(torch.equal(a[k], b[k])) for k in ("cost", "best", "kl", "bce_visual", "means", "visual")})
        for k in ("means", "log_var") + E.STATES:
            np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), **tol, err_msg=f"{k} {c}")
        for k in E.TERMS + ("cost", "step_cost", "best_cost", "top_cost"):
            assert same(a[k], b[k]), (c, k)
        low = b["cost"].double().min(0).values.abs().cpu()
        assert bool((PC.gap(b["cost"].double().cpu()) >= E.GAP * low).all())    # (the choice is pinned: the gap condition)
        assert torch.equal(a["best"], b["best"]) and torch.equal(a["best_condition"], b["best_condition"]) and torch.equal(a["top"], b["top"]), c
        win = a["best"].long()
        assert torch.equal(a["best_condition"], cands[c][win])                  # the replay saw the new candidates
        E.check_own_tables(E.cpu(a), steps_w[c], top=2, klw=float(np.float32(weights[c])))   # ... the new step and KL weights
        for m in range(3):
            np.testing.assert_allclose(a["trajectory"][m].cpu().numpy(), b["trajectory"][m].cpu().numpy(), **tol)
    assert float((g[2]["cost"] - g[1]["cost"]).abs().min()) > 0
    # new step weights and a new KL weight alone, same inputs and candidates: the same graph, another total from the same tables
    again = call(graph, 2)
    assert len(graph._graphs) == 1
    inj = MVAEInference(model, use_graph=False)
    draws = lambda first: [torch.from_numpy(P.normal_ref(B * L, seed, (first + t) * n)[0].astype(np.float32)).reshape(B, L) for t in range(T)]
    for who, res, first, inputs in (("eager", e, 0, (0, 0, 1, 2)), ("graph", g + [again], 1, (0, 1, 2, 2))):
        for c, r in enumerate(res):
            for block, near in (((c + first) * T, True), ((c + first + 1) * T, False)):
                inj.noise = InjectedNoise(draws(block), [])
                m = call(inj, inputs[c])["means"][1]
                d = (m - r["means"][1]).abs()
                print(who, "call", c, "draws from block", block, "largest / median |means[1] - injected|", float(d.max()), float(d.median()))
                if near:
                    np.testing.assert_allclose(m.cpu().numpy(), r["means"][1].cpu().numpy(), **tol, err_msg=f"{who} {c}")
                else:
                    assert float(d.median()) > 100 * tol["atol"], (who, c)
    graph.close(), eager.close(), inj.close()


def test_replay_follows_weights_alone():
    """14. (posterior means, so two calls differ only in what is asked): a replay under a new KL weight and new step weights equals
    a fresh eager call with them -- the posteriors bit for bit, the totals from the replay's own tables exactly."""
    name = "steps"
    model = PC.build(False, DEV)
    graph, eager = MVAEInference(model), MVAEInference(model, use_graph=False)
    first = E.ask(graph, name, DEV, step_weight=torch.ones(2))                  # (a weight tensor's PRESENCE is in the key)
    for w, klw in ((torch.tensor([0.25, 2.0]), 1.5), (torch.tensor([float("inf"), 1.0]), 0.3)):
        a, b = E.ask(graph, name, DEV, step_weight=w, kl_weight=klw), E.ask(eager, name, DEV, step_weight=w, kl_weight=klw)
        assert len(graph._graphs) == 1
        assert torch.equal(a["means"][0], b["means"][0]) and torch.equal(a["means"], first["means"])
        for k in E.TERMS + ("step_cost",):
            assert same(a[k], b[k]), k
        assert same(torch.nan_to_num(a["cost"]), torch.nan_to_num(b["cost"])) and torch.equal(a["best"], b["best"])
        if bool(torch.isfinite(w).all()):
            E.check_own_tables(E.cpu(a), w, klw=float(np.float32(klw)))
    graph.close(), eager.close()


def test_plan_rollout_on_dirty_allocator_memory(monkeypatch):
    """15. Eager, the mixed request with absent goal terms: every torch.empty of ops / layers / engine pre-filled with zeros, NaNs or
    junk (tests/dirty.py), and the real torch.empty: the same bits; the fp64 tables and what is formed from them come from atomics
    (rtol 1e-12)."""
    B, N, T = RC.BATCH, 3, 2
    inputs, av = RC.start()
    goal, gav = RC.frames(1402, T, B), RC.mixed_table(8, T, B)
    cand = torch.rand(N, T, CC.REAL_DIM, generator=torch.Generator().manual_seed(15))
    eps = RC.draws(37, T, B)
    got = {}
    for fill in (None,) + dirty.FILLS:
        for mod in (ops, layers, engine):
            monkeypatch.setattr(mod, "torch", torch if fill is None else dirty.PoisonTorch(fill))
        eng = MVAEInference(PC.build(False, DEV), use_graph=False)
        try:
            eng.noise = InjectedNoise([x.clone() for x in eps], [])
            r = eng.plan_rollout(E.dev_list(inputs[:2], DEV), pose=inputs[2].to(DEV), steps=T, goal=E.dev_list(goal, DEV), top=3,
                                 candidates=cand.to(DEV), available=av, goal_available=gav, sample=True, **E.KW)
            torch.cuda.synchronize()
            flat = {}
            for k, v in r.items():
                for i, t in enumerate(v if isinstance(v, list) else [v]):
                    flat[f"{k}{i}" if isinstance(v, list) else k] = t.detach().cpu().clone()
            got["real torch.empty" if fill is None else fill] = flat
        finally:
            eng.close()
    dirty.assert_same_bits(got, approx=E.TERMS + ("cost", "step_cost", "best_cost", "top_cost"), what="plan_rollout: ")
