"""MPPI weights and the receding-horizon warm start on a real MI355X: mmdyn_plan_refit_weighted / mmdyn_plan_shift against the
restatements of tests/mppi_cases.py -- the weights within MC.EXP_ULPS fp64 ulps of torch's exp on the CPU (exactly 0 and 1 where the
header fixes them), ``mean_out`` bit for bit from the device's own weights, ``std_out`` within one fp32 ulp --, on dirty destinations
and with every refused argument through the C ABI; then ``MVAEInference.plan_refine(temperature=..., warm_start=...)`` -- the checks
of tests/test_mppi_emu.py on the HIP library, captured against eager, dirty allocator memory -- and ``DynModeling.plan_refine``."""
import pytest
import torch

import dirty
import mppi_cases as MC
import plan_cases as PC
import refine_cases as RF
import rollout_cases as RC
import test_mppi_emu as E
import test_refine_emu as R
from mmdyn_hip import engine, layers, ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import InjectedNoise

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
CD = RF.CD


@pytest.fixture(autouse=True)
def hip_backend():
    old = ops.set_backend(HIP)
    yield
    ops.set_backend(old)


# ---- plan_refit_weighted -------------------------------------------------------------------------------------------------------
def test_weight_rules():
    E.check_weight_rules(HIP, DEV, exact=False)


@pytest.mark.parametrize("B,N,K,T,cd", E.WEIGHTED_SHAPES)
def test_refit_weighted_against_the_restatement(B, N, K, T, cd):
    E.check_refit_weighted(HIP, DEV, B, N, K, T, cd, exact=False)


@pytest.mark.parametrize("B,N,K,T,cd", E.TIE_SHAPES)
def test_equal_elite_costs_give_plan_refit(B, N, K, T, cd):
    E.check_tie_identity(HIP, DEV, B, N, K, T, cd)


def test_refit_weighted_on_dirty_destinations_and_bad_arguments():
    E.check_weighted_dirty(HIP, DEV)
    lib, t = HIP.lib, torch.zeros(10 * 8192, device=DEV)
    p = t.data_ptr()
    # N = 2, B = 2, T = 2, cd = 2: cost 16 bytes, cand 64, mean / std 32 each, elite 4, count 8, weight 32, ess 8 -- 32 KB apart
    cost, cand, mi, si, mo, so, el, ct, wt, es = (p + 32768 * k for k in range(10))

    def f(cost=cost, cand=cand, mi=mi, si=si, mo=mo, so=so, el=el, ct=ct, wt=wt, es=es, K=1, N=2, B=2, T=2, cd=2, temp=1.0, alpha=0.5,
          std_min=0.0):
        return lib.mmdyn_plan_refit_weighted(cost, cand, mi, si, mo, so, el, ct, wt, es, K, N, B, T, cd, temp, alpha, std_min, None)
    assert f() == 0 and f(el=None, ct=None, wt=None, es=None) == 0 and f(mo=mi, so=si) == 0 and f(K=2) == 0
    assert f(cost=None) == -2 and f(cand=None) == -2 and f(mi=None) == -2 and f(si=None) == -2 and f(mo=None) == -2 and f(so=None) == -2
    assert f(K=0) == -1 and f(K=3) == -1 and f(N=0) == -1 and f(B=0) == -1 and f(T=0) == -1 and f(cd=0) == -1
    assert f(N=4097, K=1) == -1 and f(N=4096, K=4096, B=1, T=1, cd=1) == 0
    assert f(alpha=1.0) == -1 and f(alpha=float("nan")) == -1 and f(std_min=-1.0) == -1 and f(wt=wt + 4) == -1
    assert f(temp=0.0) == -3 and f(temp=-1.0) == -3 and f(temp=float("nan")) == -3 and f(temp=float("inf")) == -3
    # an output may be exactly its own input and nothing else; weight and ess overlap nothing
    assert f(mo=mi + 4) == -1 and f(mo=si) == -1 and f(so=mi) == -1 and f(mo=so) == -1 and f(el=cost) == -1 and f(ct=mo) == -1
    assert f(wt=cost) == -1 and f(wt=cand + 32) == -1 and f(wt=mi) == -1 and f(wt=mo) == -1 and f(wt=el) == -1 and f(wt=es - 24) == -1
    assert f(es=cost) == -1 and f(es=si) == -1 and f(es=so + 16) == -1 and f(es=ct) == -1 and f(es=wt + 24) == -1
    assert f(N=4096, K=1, B=65536, T=4, cd=2) == -3
    torch.cuda.synchronize()


# ---- plan_shift ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,cd,offset", E.SHIFT_SHAPES)
def test_shift_exact(B, T, cd, offset):
    E.check_shift_exact(HIP, DEV, B, T, cd, offset)


def test_shift_on_dirty_destinations_and_bad_arguments():
    E.check_shift_dirty(HIP, DEV)
    E.check_shift_overlaps(HIP, DEV)
    lib, t = HIP.lib, torch.zeros(8 * 8192, device=DEV)
    p = t.data_ptr()
    # B = 2, T = 2, cd = 2: 32 bytes each, 32 KB apart
    pm, ps, pk, im, is_, mo, so, ko = (p + 32768 * k for k in range(8))

    def f(pm=pm, ps=ps, pk=pk, im=im, is_=is_, mo=mo, so=so, ko=ko, B=2, T=2, cd=2, shift=1, widen=0.0):
        return lib.mmdyn_plan_shift(pm, ps, pk, im, is_, mo, so, ko, B, T, cd, shift, widen, None)
    assert f() == 0 and f(pk=None, ko=None) == 0 and f(shift=0) == 0 and f(shift=2, widen=3.0) == 0 and f(ps=pm, pk=pm, im=pm, is_=pm) == 0
    assert f(pm=None) == -2 and f(ps=None) == -2 and f(im=None) == -2 and f(is_=None) == -2 and f(mo=None) == -2 and f(so=None) == -2
    assert f(pk=None) == -2 and f(ko=None) == -2
    assert f(B=0) == -1 and f(T=0) == -1 and f(cd=0) == -1 and f(shift=-1) == -1 and f(shift=3) == -1
    assert f(widen=-0.5) == -1 and f(widen=float("nan")) == -1 and f(widen=float("inf")) == -1
    assert f(mo=pm) == -1 and f(mo=ps + 28) == -1 and f(so=is_) == -1 and f(ko=im) == -1 and f(ko=pk + 4) == -1
    assert f(mo=so) == -1 and f(so=ko - 4) == -1 and f(mo=ko) == -1
    assert f(B=65536, T=4096, cd=8) == -3
    torch.cuda.synchronize()


# ---- the engine ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["steps", "nine"])
def test_mppi_equal_to_the_chain_of_existing_requests(name):
    E.check_mppi_chain(DEV, name, exact=False)


def test_large_temperature_is_cem():
    E.check_large_temperature_is_cem(DEV, "steps")


def test_warm_start():
    E.check_warm_start(DEV)


def test_problem_layer(tmp_path):
    E.check_problem_layer(DEV, tmp_path)


def test_captured_equals_eager():
    """use_graph=True against an eager engine with the same seed, MPPI with a warm start: three replays with new inputs, goals,
    init_mean / init_std and previous plans -- all static inputs of ONE graph.  The capture's eager warm-up takes the draws of the
    first call, so replay c is compared with eager call c + 1: the same bits.  Replay 2 is warm-started from the dict replay 1
    returned -- the graph's own output buffers."""
    name, seed = "steps", 5
    B, N, K, T, I = RF.CASES[name][:5]
    model = PC.build(False, DEV)
    from mmdyn_hip.utils.seeded_init import seeded_batch
    g = torch.Generator().manual_seed(78)
    xs = [R.dev_list(seeded_batch(B, 1900 + c, with_pose=True)[0], DEV) for c in range(3)]
    goals = [R.dev_list(RC.frames(1910 + c, T, B), DEV) for c in range(3)]
    means = [0.25 + 0.5 * torch.rand(T, CD, generator=g) for _ in range(3)]
    stds = [0.05 + 0.2 * torch.rand(B, T, CD, generator=g) for _ in range(3)]
    prevs = [{k: torch.rand(B, T, CD, generator=g).to(DEV) for k in ("mean", "std", "best_condition")} for _ in range(3)]
    raw = lambda eng, c, prev: eng.plan_refine(xs[c][:2], pose=xs[c][2], steps=T, goal=goals[c], init_mean=means[c], init_std=stds[c],
                                               candidates=N, elites=N, iterations=I, alpha=0.25, std_min=0.01, sample=True,
                                               temperature=E.TEMPERATURE, warm_start=prev, shift=1, widen=0.5, **R.KW)
    call = lambda eng, c, prev: R.keep(raw(eng, c, prev))
    eager = MVAEInference(model, seed=seed, use_graph=False)
    e = [call(eager, 0, prevs[0]), call(eager, 0, prevs[0]), call(eager, 1, prevs[1])]
    e.append(call(eager, 2, e[2]))
    graph = MVAEInference(model, seed=seed)
    assert graph.use_graph
    gr = [call(graph, 0, prevs[0])]
    live = raw(graph, 1, prevs[1])                                       # the graph's static outputs, not copied
    gr.append(R.keep(live))
    gr.append(call(graph, 2, live))
    assert len(graph._graphs) == 1
    key = next(iter(graph._graphs))
    assert key[:6] == ("plan_refine", I, N, N, T, T) and key[-2:] == (("mppi", E.TEMPERATURE), ("warm", 1, 0.5))
    for c in range(3):
        a, b = gr[c], e[c + 1]
        same = {k: dirty.first_diff(a[k], b[k]) is None for k in ("candidates", "mean", "std", "cost", "best", "history", "best_condition",
                                                                  "elite_count", "ess", "weight")}
        print("replay", c, "bit-equal to eager:", same, "ess", a["ess"].tolist())
        assert all(same.values()), (c, same)
    graph.close(), eager.close()


def test_plan_refine_on_dirty_allocator_memory(monkeypatch):
    """Eager, one round of MPPI with a warm start: every torch.empty of ops / layers / engine pre-filled with zeros, NaNs or junk
    (tests/dirty.py), and the real torch.empty: the same bits; the fp64 tables and what is formed from them come from atomics (rtol
    1e-12).  The weights are formed from those costs: a cost of a few 1e4 that moves by 1e-12 of itself moves q = d / 100 by a few
    1e-10 and so the weight and ess by that fraction (rtol 1e-8); mean and std may then round to the neighbouring fp32 (rtol 1e-6)."""
    name = "steps"
    B, N, K, T, I = RF.CASES[name][:5]
    prev = {k: 0.25 + 0.5 * torch.rand(B, T, CD, generator=torch.Generator().manual_seed(18)).to(DEV) for k in ("mean", "std", "best_condition")}
    got = {}
    for fill in (None,) + dirty.FILLS:
        for mod in (ops, layers, engine):
            monkeypatch.setattr(mod, "torch", torch if fill is None else dirty.PoisonTorch(fill))
        eng = MVAEInference(PC.build(False, DEV), use_graph=False)
        try:
            r = R.ask(eng, name, DEV, iterations=1, temperature=E.TEMPERATURE, warm_start=prev, shift=1, widen=0.5)
            torch.cuda.synchronize()
            flat = {}
            for k, v in r.items():
                for i, t in enumerate(v if isinstance(v, list) else [v]):
                    if t is not None:
                        flat[f"{k}{i}" if isinstance(v, list) else k] = t.detach().cpu().clone()
            got["real torch.empty" if fill is None else fill] = flat
        finally:
            eng.close()
    part = lambda keys: {fill: {k: v for k, v in flat.items() if (k in keys)} for fill, flat in got.items()}
    from_weights = ("weight", "ess", "mean", "std")
    what = "plan_refine(temperature, warm_start): "
    dirty.assert_same_bits(part(set(got[dirty.ZERO]) - set(from_weights)), approx=R.E.TERMS + ("cost", "step_cost", "best_cost", "history"), what=what)
    dirty.assert_same_bits(part(("weight", "ess")), approx=("weight", "ess"), rtol=1e-8, what=what)
    dirty.assert_same_bits(part(("mean", "std")), approx=("mean", "std"), rtol=1e-6, what=what)
