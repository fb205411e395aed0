"""I = 4 iterations of the cross-entropy method over a horizon of T = 8 steps (N candidate shock sequences per row, the K = 8 best
refit mean and std), two ways (docs/LAB_NOTES.md X), on one MI355X, 64 x 64, L = 256, fp32x3, a real-valued conditional model,
posterior-mean latents, at (B, N) = (32, 8) and (4, 64):
  (a) loop:   what the API allows without ``plan_refine`` -- per iteration torch ``randn`` candidates on the device, one replayed
              ``plan_rollout(top=8)``, the elites indexed out through ``top`` with torch, a torch mean / std; nothing synchronises;
  (b) refine: ONE replayed ``plan_refine(candidates=N, elites=8, iterations=4)``.
One process, the two in alternation, three rounds; in each round one pair of device events around CALLS = 200 calls after WARM = 20
warm-up calls, the time per call = elapsed / CALLS; the median of the rounds is reported, and the spread of (a) between its rounds is
the yardstick for (b) - (a).  The two draw different numbers (torch's generator against the engine's Philox stream), so their
results are not compared here: tests/test_refine_gpu.py holds ``plan_refine`` to the same loop on the same draws, bit for bit.

    python tests/microbench/time_refine.py [out.json] [calls] [warm]
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-dynamics_amd")]
import torch
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import setup_model
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats

dev, CD, T, I, K = "cuda", 3, 8, 4, 8
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


res = {"calls": CALLS, "warm": WARM, "iterations": I, "elites": K}
for B, N in ((32, 8), (4, 64)):
    g = torch.Generator().manual_seed(B)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    v, t, p = r(B, 3, 64, 64), r(B, 3, 64, 64), r(B, 7)
    goal = [r(T, B, 3, 64, 64), r(T, B, 3, 64, 64), r(T, B, 7)]
    mean0, std0 = torch.full((B, T, CD), 0.5, device=dev), torch.full((B, T, CD), 0.25, device=dev)
    rows = torch.arange(B, device=dev)

    def loop():
        mean, std = mean0, std0
        for _ in range(I):
            cand = mean.unsqueeze(1) + std.unsqueeze(1) * torch.randn(B, N, T, CD, device=dev)
            out = eng.plan_rollout([v, t], pose=p, steps=T, goal=goal, candidates=cand, top=K, **KW)
            elite = cand[rows, out["top"].long()]                                              # [K][B][T][cd], through the device list
            mean, std = elite.mean(0), elite.std(0, unbiased=False)
        return mean, std

    call = {"loop": loop,
            "refine": lambda: eng.plan_refine([v, t], pose=p, steps=T, goal=goal, init_mean=mean0, init_std=std0, candidates=N, elites=K,
                                              iterations=I, **KW)}
    for rnd in range(3):
        for k in ("loop", "refine"):
            res.setdefault(f"B{B}_N{N}/{k}", []).append(timed(call[k]))
    us = {k: res[f"B{B}_N{N}/{k}"] for k in ("loop", "refine")}
    res[f"B{B}_N{N}/summary"] = {"loop_median_us": statistics.median(us["loop"]), "refine_median_us": statistics.median(us["refine"]),
                                 "loop_round_spread_us": round(max(us["loop"]) - min(us["loop"]), 1)}
    print(B, N, T, us, res[f"B{B}_N{N}/summary"], "(us per request: one figure per round)", flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
