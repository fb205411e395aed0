"""Iterative plan refinement on a real MI355X: mmdyn_plan_sample / mmdyn_plan_refit against the restatements of tests/refine_cases.py
(``cand`` and ``mean_out`` bit for bit, ``std_out`` within one fp32 ulp), on dirty destinations and with every refused argument; the
model-free loop; then ``MVAEInference.plan_refine`` -- the checks of tests/test_refine_emu.py on the HIP library, the Philox counters,
captured against eager on one stream, dirty allocator memory -- and ``DynModeling.plan_refine``.  The reference has no such
operation: nothing here comes from a golden file."""
import numpy as np
import pytest
import torch

import dirty
import philox_ref as P
import plan_cases as PC
import refine_cases as RF
import rollout_cases as RC
import test_refine_emu as E
from mmdyn_hip import engine, layers, ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise
from test_noise_gpu import NORMAL_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
CD = RF.CD
L = PC.L


@pytest.fixture(autouse=True)
def hip_backend():
    old = ops.set_backend(HIP)
    yield
    ops.set_backend(old)


# ---- plan_sample ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,T,cd,shift", E.SAMPLE_SHAPES)
def test_sample_exact(B, N, T, cd, shift):
    E.check_sample_exact(HIP, DEV, B, N, T, cd, shift)


def test_sample_on_dirty_destinations_and_bad_arguments():
    E.check_sample_dirty(HIP, DEV)
    lib, t = HIP.lib, torch.zeros(4096, device=DEV)
    p = t.data_ptr()
    q = p + 8192                                                         # cand: past every input of the calls below

    def f(mean=p, std=p, eps=p, keep=None, lo=None, hi=None, cand=q, N=2, B=2, T=2, cd=2):
        return lib.mmdyn_plan_sample(mean, std, eps, keep, lo, hi, cand, N, B, T, cd, None)
    assert f() == 0 and f(keep=p, lo=p, hi=p) == 0
    assert f(mean=None) == -2 and f(std=None) == -2 and f(eps=None) == -2 and f(cand=None) == -2 and f(lo=p) == -2 and f(hi=p) == -2
    assert f(N=0) == -1 and f(B=0) == -1 and f(T=0) == -1 and f(cd=0) == -1
    assert f(cand=p) == -1 and f(cand=p + 60) == -1 and f(keep=q) == -1 and f(lo=q + 4, hi=p) == -1      # cand over an input
    assert f(N=65536, B=32768) == -3 and f(N=4096, B=4096, T=64, cd=2) == -3
    torch.cuda.synchronize()


# ---- plan_refit ----------------------------------------------------------------------------------------------------------------
def test_refit_rules():
    E.check_refit_rules(HIP, DEV)


@pytest.mark.parametrize("B,N,K,T,cd", E.REFIT_SHAPES)
def test_refit_against_the_restatement(B, N, K, T, cd):
    E.check_refit_restatement(HIP, DEV, B, N, K, T, cd)


@pytest.mark.parametrize("B,N,K", [(5, 9, 3), (3, 40, 8), (1, 2, 1)])
def test_refit_elites_are_the_top_list(B, N, K):
    E.check_refit_is_top(HIP, DEV, B, N, K)


def test_refit_on_dirty_destinations_and_bad_arguments():
    E.check_refit_dirty(HIP, DEV)
    lib, t = HIP.lib, torch.zeros(65536, device=DEV)
    p = t.data_ptr()
    # N = 2, B = 2, T = 2, cd = 2: cost 16 bytes, cand 64, mean / std 32 each, elite 4, count 8 -- 32 KB apart unless overridden
    cost, cand, mi, si, mo, so, el, ct = (p + 32768 * k for k in range(8))

    def f(cost=cost, cand=cand, mi=mi, si=si, mo=mo, so=so, el=el, ct=ct, K=1, N=2, B=2, T=2, cd=2, alpha=0.5, std_min=0.0):
        return lib.mmdyn_plan_refit(cost, cand, mi, si, mo, so, el, ct, K, N, B, T, cd, alpha, std_min, None)
    assert f() == 0 and f(el=None, ct=None) == 0 and f(mo=mi, so=si) == 0 and f(K=2) == 0
    assert f(cost=None) == -2 and f(cand=None) == -2 and f(mi=None) == -2 and f(si=None) == -2 and f(mo=None) == -2 and f(so=None) == -2
    assert f(K=0) == -1 and f(K=3) == -1 and f(N=0) == -1 and f(B=0) == -1 and f(T=0) == -1 and f(cd=0) == -1
    assert f(N=4097, K=1) == -1 and f(N=4096, K=4096, B=1, T=1, cd=1) == 0
    assert f(alpha=1.0) == -1 and f(alpha=-0.25) == -1 and f(alpha=float("nan")) == -1
    assert f(std_min=-1.0) == -1 and f(std_min=float("nan")) == -1
    # an output may be exactly its own input and nothing else
    assert f(mo=mi + 4) == -1 and f(mo=si) == -1 and f(so=mi) == -1 and f(mo=so) == -1 and f(mo=cand + 32) == -1 and f(so=cost) == -1
    assert f(el=cost) == -1 and f(ct=mo) == -1 and f(el=ct) == -1 and f(ct=cand) == -1
    assert f(N=4096, K=1, B=65536, T=4, cd=2) == -3
    torch.cuda.synchronize()


def test_loop_without_the_model():
    E.check_loop(HIP, DEV)


# ---- the engine ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RF.CASES))
def test_equal_to_the_chain_of_existing_requests(name):
    E.check_chain(DEV, name)


@pytest.mark.parametrize("name", ["steps", "one"])
def test_incumbent(name):
    E.check_incumbent(DEV, name)


@pytest.mark.parametrize("name", list(RF.CASES))
def test_history_does_not_rise(name):
    E.check_history(DEV, name)


def test_mixed_request_and_absent_goal_terms():
    E.check_mixed_request(DEV)


def test_problem_layer(tmp_path):
    E.check_problem_layer(DEV, tmp_path)


@pytest.mark.parametrize("sample", [False, True])
def test_philox_counters(sample):
    """With the engine's own NoiseSource, iteration 0's candidates of two consecutive eager calls are mean + std * eps of the
    reference draws at the stated counters, within NORMAL_TOL * std; the two calls draw disjoint counters."""
    name, seed = "steps", 7
    B, N, K, T, I = RF.CASES[name][:5]
    eng = MVAEInference(PC.build(False, DEV), seed=seed, use_graph=False)
    _, _, mean, std, _, _ = RF.request(name)
    seen = []
    for call in range(2):
        # iterations = 1: the returned candidates are iteration 0's; the counters advance by I = 1 iteration per call
        r = E.keep(eng.plan_refine(**E.call_kw(name, DEV, iterations=1, sample=sample)))
        n_c, n_l = P.counters_of(N * B * T * CD), P.counters_of(B * L)
        per = n_c + (T * n_l if sample else 0)
        z = torch.from_numpy(P.normal_ref(N * B * T * CD, seed, call * per)[0].astype(np.float32)).reshape(N, B, T, CD)
        want = RF.sample_ref(mean.expand(B, T, CD).contiguous(), std.expand(B, T, CD).contiguous(), z).view(T, N, B, CD)
        got = r["candidates"].cpu()
        err = ((got - want).abs() / std.reshape(T, 1, 1, CD)).max()
        print("call", call, "sample", sample, "largest |candidates - reference| / std", float(err), "allowed", NORMAL_TOL)
        assert float(err) <= NORMAL_TOL
        assert dirty.first_diff(got[:, 0], mean.reshape(T, 1, CD).expand(T, B, CD).contiguous()) is None
        seen.append(got[:, 1:])
    assert float((seen[1] - seen[0]).abs().median()) > 100 * NORMAL_TOL * float(std.min())   # the second call drew another block
    eng.close()


def test_captured_equals_eager_on_one_philox_stream():
    """use_graph=True against an eager engine with the same seed: three replays with new inputs, goals, init_mean / init_std, bounds,
    step weights and KL weight -- all static inputs of ONE graph.  The capture's eager warm-up takes the draws of the first call, so
    replay c is compared with eager call c + 1: the same bits."""
    name, seed = "nine", 5
    B, N, K, T, I = RF.CASES[name][:5]
    model = PC.build(False, DEV)
    from mmdyn_hip.utils.seeded_init import seeded_batch
    g = torch.Generator().manual_seed(77)
    xs = [E.dev_list(seeded_batch(B, 1800 + c, with_pose=True)[0], DEV) for c in range(3)]
    goals = [E.dev_list([t[0] for t in RC.frames(1810 + c, 1, B)], DEV) for c in range(3)]
    means = [0.25 + 0.5 * torch.rand(T, CD, generator=g) for _ in range(3)]
    stds = [0.05 + 0.2 * torch.rand(B, T, CD, generator=g) for _ in range(3)]
    bounds = [(torch.full((CD,), 0.1 * c), torch.full((CD,), 1.0 - 0.1 * c)) for c in range(3)]
    steps_w = [torch.tensor([w]) for w in (1.0, 0.5, 2.0)]
    weights = (0.3, 0.3, 2.0)
    call = lambda eng, c: E.keep(eng.plan_refine(xs[c][:2], pose=xs[c][2], steps=T, goal=goals[c], init_mean=means[c], init_std=stds[c],
                                                 candidates=N, elites=K, iterations=I, alpha=0.25, std_min=0.01, bounds=bounds[c],
                                                 step_weight=steps_w[c], sample=True, kl_weight=weights[c], pose_multiplier=1000.0))
    eager = MVAEInference(model, seed=seed, use_graph=False)
    e = [call(eager, c) for c in (0, 0, 1, 2)]
    graph = MVAEInference(model, seed=seed)
    assert graph.use_graph
    gr = [call(graph, c) for c in range(3)]
    assert len(graph._graphs) == 1
    key = next(iter(graph._graphs))
    assert key[:6] == ("plan_refine", I, N, K, T, 1) and key[6] is True
    for c in range(3):
        a, b = gr[c], e[c + 1]
        same = {k: dirty.first_diff(a[k], b[k]) is None for k in ("candidates", "mean", "std", "cost", "best", "history", "best_condition",
                                                                  "elite_count", "means", "kl")}
        print("replay", c, "bit-equal to eager:", same)
        assert all(same.values()), (c, same)
        for m in range(3):
            assert dirty.first_diff(a["trajectory"][m], b["trajectory"][m]) is None, (c, m)
        lo, hi = bounds[c]
        cand = a["candidates"].cpu()
        assert bool((cand >= lo).all()) and bool((cand <= hi).all())     # the replay saw the new bounds
    assert float((gr[2]["mean"] - gr[1]["mean"]).abs().max()) > 0
    # another I, N or K is another graph; new values are not
    call(graph, 1)
    assert len(graph._graphs) == 1
    E.keep(graph.plan_refine(xs[0][:2], pose=xs[0][2], steps=T, goal=goals[0], init_mean=means[0], init_std=stds[0], candidates=N, elites=K - 1,
                             iterations=I, alpha=0.25, std_min=0.01, bounds=bounds[0], step_weight=steps_w[0], sample=True, **E.KW))
    assert len(graph._graphs) == 2
    graph.close(), eager.close()


def test_plan_refine_on_dirty_allocator_memory(monkeypatch):
    """Eager, the mixed request: every torch.empty of ops / layers / engine pre-filled with zeros, NaNs or junk (tests/dirty.py), and
    the real torch.empty: the same bits; the fp64 tables and what is formed from them come from atomics (rtol 1e-12)."""
    B, N, K, T, I = RC.BATCH, 3, 2, 2, 2
    inputs, av = RC.start()
    goal, gav = RC.frames(1402, T, B), RC.mixed_table(8, T, B)
    g = torch.Generator().manual_seed(17)
    mean, std = torch.rand(T, CD, generator=g), 0.1 + 0.1 * torch.rand(T, CD, generator=g)
    draws = [torch.randn(N, B, T, CD, generator=g) for _ in range(I)]
    got = {}
    for fill in (None,) + dirty.FILLS:
        for mod in (ops, layers, engine):
            monkeypatch.setattr(mod, "torch", torch if fill is None else dirty.PoisonTorch(fill))
        eng = MVAEInference(PC.build(False, DEV), use_graph=False)
        try:
            eng.noise = InjectedNoise([x.clone() for x in draws], [])
            r = eng.plan_refine(E.dev_list(inputs[:2], DEV), pose=inputs[2].to(DEV), steps=T, goal=E.dev_list(goal, DEV), init_mean=mean,
                                init_std=std, candidates=N, elites=K, iterations=I, available=av, goal_available=gav, **E.KW)
            torch.cuda.synchronize()
            flat = {}
            for k, v in r.items():
                for i, t in enumerate(v if isinstance(v, list) else [v]):
                    flat[f"{k}{i}" if isinstance(v, list) else k] = t.detach().cpu().clone()
            got["real torch.empty" if fill is None else fill] = flat
        finally:
            eng.close()
    dirty.assert_same_bits(got, approx=E.E.TERMS + ("cost", "step_cost", "best_cost", "history"), what="plan_refine: ")
