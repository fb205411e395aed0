"""N = 16 candidate conditions per row, scored against a goal and the best one served, two ways (docs/LAB_NOTES.md R), on one
MI355X, batch 32 and 256, 64 x 64, fp32x3, a real-valued conditional model, sampled latents:
  (a) chain: what a caller wrote before ``MVAEInference.plan`` -- N replayed ``score(condition=c_n)`` calls, the N x B costs copied
             to the host, a host argmin, and one more replayed ``forward()`` with each row's winner;
  (b) plan:  ONE replayed ``plan(candidates=[N, cd])``.
Device events around each call (the chain's host copy and argmin lie between them), 10 warm-up calls, median and spread (min ..
max) of 50 calls, three rounds in alternation; the spread of (a) between its rounds is the yardstick for (b) - (a).

    python tests/microbench/time_plan.py [out.json]
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-dynamics_amd")]
import torch
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import setup_model
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats

dev, N, CD = "cuda", 16, 3
m = setup_model("cnn-mvae", cross_modal=True, input_dim=4096, architecture="cnn", latent_size=256, use_pose=True, conditional=True,
                categorical_conditions=False, condition_dim=CD)
m.load_state_dict(seeded_running_stats(seeded_state_dict(m.state_dict(), 0)))
eng = MVAEInference(m.to(dev).eval(), seed=1)
KW = dict(kl_weight=0.3, pose_multiplier=1000.0)


def timed(fn, n=50, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) * 1e3)
    return [round(statistics.median(ms), 1), round(min(ms), 1), round(max(ms), 1)]


res = {}
for B in (32, 256):
    g = torch.Generator().manual_seed(B)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    v, t, p = r(B, 3, 64, 64), r(B, 3, 64, 64), r(B, 7)
    goal = [r(B, 3, 64, 64), r(B, 3, 64, 64), r(B, 7)]
    cand = r(N, CD)

    def chain():
        costs = torch.empty(N, B, device=dev)
        for n in range(N):
            costs[n] = eng.score([v, t], pose=p, targets=goal, condition=cand[n].expand(B, CD), **KW)["rows"]
        best = torch.from_numpy(costs.cpu().numpy().argmin(0)).to(dev)            # the choice is made on the host
        return eng.forward([v, t], pose=p, condition=cand[best])

    # (score() and forward() draw their latents, so the plan draws too: one [B, L] block per request)
    call = {"chain": chain, "plan": lambda: eng.plan([v, t], pose=p, goal=goal, candidates=cand, sample=True, **KW)}
    for rnd in range(3):
        for k in ("chain", "plan"):
            res.setdefault(f"B{B}/{k}", []).append(timed(call[k]))
    print(B, {k: v_ for k, v_ in res.items() if k.startswith(f"B{B}/")}, "(us per request of N = 16 candidates: median, min, max per round)",
          flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
