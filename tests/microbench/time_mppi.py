"""MPPI weights and the warm start beside what they stand next to (docs/LAB_NOTES.md AC), on one MI355X, by the method of
tests/microbench/time_refine.py: one process, the two sides in alternation, three rounds, one pair of device events around CALLS
calls after WARM warm-up calls, the time per call = elapsed / CALLS; the median of the rounds is reported and the spread of the first
side between its rounds is the yardstick for the difference.
  kernels: mmdyn_plan_refit beside mmdyn_plan_refit_weighted through ops.HipBackend, T * cd = 8 * 3 = 24, at (B, N, K) = (32, 8, 8),
           (4, 64, 64) and (32, 4096, 4096) -- K = N: plan_refit ranks, plan_refit_weighted does not.  Back-to-back launches, so a
           figure is the larger of the launch interval and the kernel; run ``kernels`` alone under a kernel trace for the kernels' own
           durations.
  step:    one control step at T = 8, I = 4, (B, N) = (32, 8), 64 x 64, L = 256, fp32x3:
           cold = one replayed ``plan_refine`` started at the torch-shifted mean / std of the previous call, plus the torch shift of
                  ``mean`` / ``std`` / ``best_condition`` between the replays (the previous winner cannot be handed back);
           warm = one replayed ``plan_refine(warm_start=previous result, shift=1)``;
           and the same warm step with ``temperature`` (MPPI, K = N).

    python tests/microbench/time_mppi.py [out.json] [kernels|step|all] [calls] [warm]
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-dynamics_amd")]
import torch
from mmdyn_hip import ops

dev, CD, T, I = "cuda", 3, 8, 4
WHAT = sys.argv[2] if len(sys.argv) > 2 else "all"
CALLS = int(sys.argv[3]) if len(sys.argv) > 3 else 200
WARM = int(sys.argv[4]) if len(sys.argv) > 4 else 20


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) * 1e3 / CALLS, 1)


def rounds(res, tag, call):
    names = list(call)
    for rnd in range(3):
        for k in names:
            res.setdefault(f"{tag}/{k}", []).append(timed(call[k]))
    us = {k: res[f"{tag}/{k}"] for k in names}
    res[f"{tag}/summary"] = dict({f"{k}_median_us": statistics.median(us[k]) for k in names},
                                 **{f"{names[0]}_round_spread_us": round(max(us[names[0]]) - min(us[names[0]]), 1)})
    print(tag, us, res[f"{tag}/summary"], "(us per call: one figure per round)", flush=True)


res = {"calls": CALLS, "warm": WARM}
if WHAT in ("kernels", "all"):
    hip = ops.B
    for B, N, K in ((32, 8, 8), (4, 64, 64), (32, 4096, 4096)):
        g = torch.Generator().manual_seed(N)
        cost = (3.0 + 50.0 * torch.rand(N, B, generator=g)).to(dev)
        cand = torch.randn(T, N * B, CD, generator=g).to(dev)
        mean_in, std_in = torch.zeros(B, T, CD, device=dev), torch.ones(B, T, CD, device=dev)
        mean, std = torch.empty_like(mean_in), torch.empty_like(std_in)
        count, weight, ess = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(N, B, dtype=torch.float64, device=dev), torch.empty(B, device=dev)
        rounds(res, f"kernels/B{B}_N{N}_K{K}",
               {"refit": lambda: hip.plan_refit(cost, cand, mean_in, std_in, mean, std, None, count, K, N, B, T, 0.0, 0.0),
                "refit_weighted": lambda: hip.plan_refit_weighted(cost, cand, mean_in, std_in, mean, std, None, count, weight, ess, K, N, B, T,
                                                                  10.0, 0.0, 0.0)})
if WHAT in ("step", "all"):
    from mmdyn_hip.engine import MVAEInference
    from mmdyn_hip.models import setup_model
    from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats
    m = setup_model("cnn-mvae", cross_modal=True, input_dim=4096, architecture="cnn", latent_size=256, use_pose=True, conditional=True,
                    categorical_conditions=False, condition_dim=CD)
    m.load_state_dict(seeded_running_stats(seeded_state_dict(m.state_dict(), 0)))
    eng = MVAEInference(m.to(dev).eval(), seed=1)
    KW = dict(kl_weight=0.3, pose_multiplier=1000.0)
    B, N, K = 32, 8, 8
    g = torch.Generator().manual_seed(B)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    v, t, p = r(B, 3, 64, 64), r(B, 3, 64, 64), r(B, 7)
    goal = [r(T, B, 3, 64, 64), r(T, B, 3, 64, 64), r(T, B, 7)]
    mean0, std0 = torch.full((B, T, CD), 0.5, device=dev), torch.full((B, T, CD), 0.25, device=dev)
    req = dict(x=[v, t], pose=p, steps=T, goal=goal, candidates=N, elites=K, iterations=I, **KW)
    state = {"cold": eng.plan_refine(init_mean=mean0, init_std=std0, **req)}
    state["cold"] = {k: state["cold"][k].clone() for k in ("mean", "std", "best_condition")}
    state["warm"] = dict(state["cold"])
    state["mppi"] = dict(state["cold"])
    moved = lambda prev, init: torch.cat((prev[:, 1:], init[:, -1:]), 1)

    def cold():
        s = state["cold"]
        mean, std, kept = moved(s["mean"], mean0), moved(s["std"], std0), moved(s["best_condition"], mean0)   # (kept: no way back in)
        out = eng.plan_refine(init_mean=mean, init_std=std, **req)
        state["cold"] = {k: out[k] for k in ("mean", "std", "best_condition")}
        return kept

    def warm(key="warm", **extra):
        state[key] = eng.plan_refine(init_mean=mean0, init_std=std0, warm_start=state[key], shift=1, **extra, **req)

    rounds(res, f"step/B{B}_N{N}_T{T}_I{I}", {"cold": cold, "warm": warm, "warm_mppi": lambda: warm("mppi", temperature=100.0)})
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
