"""A T-step trajectory of the one-step dynamics model, served two ways (docs/LAB_NOTES.md O), on one MI355X, T = 16 at batch 32 and
256, 64 x 64, fp32x3, a fresh draw per step:
  (a) chain:   what a caller wrote before ``MVAEInference.rollout`` -- per step one replayed ``forward()`` (its inputs copied into
               the graph's static buffers), then three ``complete_select`` launches back to image space;
  (b) rollout: ONE replayed ``rollout(steps=T, sample=True)``.
Device events around each call, 20 warm-up calls, median and spread (min .. max) of 200 calls, three rounds in alternation; the
spread of (a) between its rounds is the yardstick for (b) - (a).

    python tests/microbench/time_rollout.py [out.json]
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-dynamics_amd")]
import torch
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import setup_model
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats

dev, T = "cuda", 16
m = setup_model("cnn-mvae", cross_modal=True, input_dim=4096, architecture="cnn", latent_size=256, use_pose=True, conditional=False,
                categorical_conditions=False, condition_dim=0)
m.load_state_dict(seeded_running_stats(seeded_state_dict(m.state_dict(), 0)))
eng = MVAEInference(m.to(dev).eval(), seed=1)


def timed(fn, n=200, warm=20):
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
    v, t, p = (torch.rand(B, 3, 64, 64, generator=g).to(dev), torch.rand(B, 3, 64, 64, generator=g).to(dev),
               torch.rand(B, 7, generator=g).to(dev))
    traj = [torch.empty(T, B, 3, 64, 64, device=dev), torch.empty(T, B, 3, 64, 64, device=dev), torch.empty(T, B, 7, device=dev)]

    def chain():
        s = [v, t, p]
        for i in range(T):
            lv, lt, pr = eng.forward([s[0], s[1]], pose=s[2])[:3]
            ops.B.complete_select(None, lv, None, 0, traj[0][i], True)
            ops.B.complete_select(None, lt, None, 1, traj[1][i], True)
            ops.B.complete_select(None, pr, None, 2, traj[2][i], False)
            s = [traj[0][i], traj[1][i], traj[2][i]]
        return traj

    call = {"chain": chain, "rollout": lambda: eng.rollout([v, t], pose=p, steps=T, sample=True)}
    for rnd in range(3):
        for k in ("chain", "rollout"):
            res.setdefault(f"B{B}/{k}", []).append(timed(call[k]))
    print(B, {k: v_ for k, v_ in res.items() if k.startswith(f"B{B}/")}, "(us per T = 16 trajectory: median, min, max per round)",
          flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
