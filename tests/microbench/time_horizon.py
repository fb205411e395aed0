"""N candidate condition sequences per row rolled out over T = 8 steps, scored against a goal per step and the best trajectory
served, two ways (docs/LAB_NOTES.md W), on one MI355X, 64 x 64, fp32x3, a real-valued conditional model, posterior-mean latents, at
(B, N, T) = (32, 8, 8) and (4, 64, 8):
  (a) chain:   what today's API allows without ``plan_rollout`` -- N replayed ``rollout(steps=T, condition=sequence n, targets=goal)``
               calls, each one's ``rows`` [T, B] table copied to the host, a host weighted sum over the steps and a host argmin, and the
               winner's trajectory indexed out of the N kept ones;
  (b) horizon: ONE replayed ``plan_rollout(candidates=[N, T, cd], goal=[T, B, ...], step_weight=[T])``.
One process, the two in alternation, three rounds; in each round one pair of device events around CALLS = 200 calls after WARM = 20
warm-up calls (the chain's host copies, sum and argmin lie between the events), the time per call = elapsed / CALLS; the median of the
rounds is reported, and the spread of (a) between its rounds is the yardstick for (b) - (a).

    python tests/microbench/time_horizon.py [out.json] [calls] [warm]
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-dynamics_amd")]
import torch
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import setup_model
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats

dev, CD, T = "cuda", 3, 8
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 20
m = setup_model("cnn-mvae", cross_modal=True, input_dim=4096, architecture="cnn", latent_size=256, use_pose=True, conditional=True,
                categorical_conditions=False, condition_dim=CD)
m.load_state_dict(seeded_running_stats(seeded_state_dict(m.state_dict(), 0)))
eng = MVAEInference(m.to(dev).eval(), seed=1)
KW = dict(kl_weight=0.3, pose_multiplier=1000.0)


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


res = {"calls": CALLS, "warm": WARM}
for B, N in ((32, 8), (4, 64)):
    g = torch.Generator().manual_seed(B)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    v, t, p = r(B, 3, 64, 64), r(B, 3, 64, 64), r(B, 7)
    goal = [r(T, B, 3, 64, 64), r(T, B, 3, 64, 64), r(T, B, 7)]
    cand = r(N, T, CD)
    weight = torch.linspace(0.5, 1.0, T)
    weight_dev = weight.to(dev)

    def chain():
        kept, total = [], torch.empty(N, B, dtype=torch.float64)
        for n in range(N):
            out = eng.rollout([v, t], pose=p, steps=T, condition=cand[n].unsqueeze(1).expand(T, B, CD), targets=goal, **KW)
            total[n] = (weight.double().unsqueeze(1) * out["rows"].cpu().double()).sum(0)      # the table visits the host
            kept.append([out[k].clone() for k in ("visual", "tactile", "pose")])               # (the outputs are the graph's static tensors)
        best = total.argmin(0).to(dev)                                                          # the choice is made on the host
        rows = torch.arange(B, device=dev)
        return [torch.stack([k[m_] for k in kept])[best, :, rows].transpose(0, 1) for m_ in range(3)]

    call = {"chain": chain,
            "horizon": lambda: eng.plan_rollout([v, t], pose=p, steps=T, goal=goal, candidates=cand, step_weight=weight_dev, **KW)}
    # the two pick the same sequences (every row: the totals differ by rounding only where the chain's fp32 rows are summed)
    a, b = call["chain"](), call["horizon"]()
    torch.cuda.synchronize()
    agree = float((a[2] - b["trajectory"][2]).abs().max())
    for rnd in range(3):
        for k in ("chain", "horizon"):
            res.setdefault(f"B{B}_N{N}/{k}", []).append(timed(call[k]))
    us = {k: res[f"B{B}_N{N}/{k}"] for k in ("chain", "horizon")}
    res[f"B{B}_N{N}/summary"] = {"chain_median_us": statistics.median(us["chain"]), "horizon_median_us": statistics.median(us["horizon"]),
                                 "chain_round_spread_us": round(max(us["chain"]) - min(us["chain"]), 1),
                                 "largest_pose_difference_of_the_two_winners": agree}
    print(B, N, T, us, res[f"B{B}_N{N}/summary"], "(us per request: one figure per round)", flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
