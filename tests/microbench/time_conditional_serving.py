"""Replayed request time of MVAEInference.forward, categorical-conditional (condition_dim 5) beside unconditional, at batch
1 / 64 / 4096 (docs/LAB_NOTES.md J): both engines in one process, five rounds in alternation, microseconds per request.

    python tests/microbench/time_conditional_serving.py [out.json]
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-dynamics_amd")]
import torch
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import setup_model
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats

dev = "cuda"
def engine(cond):
    kw = dict(input_dim=4096, architecture="cnn", latent_size=256, use_pose=True, conditional=cond, categorical_conditions=cond,
              condition_dim=5 if cond else 0)
    m = setup_model("cnn-mvae", cross_modal=True, **kw)
    m.load_state_dict(seeded_running_stats(seeded_state_dict(m.state_dict(), 0)))
    return MVAEInference(m.to(dev).eval(), seed=1)

engs = {"uncond": engine(False), "cond": engine(True)}
res = {}
for B in (1, 64, 4096):
    g = torch.Generator().manual_seed(B)
    v, t, p = torch.rand(B, 3, 64, 64, generator=g).to(dev), torch.rand(B, 3, 64, 64, generator=g).to(dev), torch.rand(B, 7, generator=g).to(dev)
    c = torch.randint(0, 5, (B,), generator=g).to(dev)
    n = 300 if B < 4096 else 20
    call = {"uncond": lambda: engs["uncond"].forward([v, t], pose=p), "cond": lambda: engs["cond"].forward([v, t], pose=p, condition=c)}
    for k in call:
        for _ in range(10):
            call[k]()
    torch.cuda.synchronize()
    for rnd in range(5):
        for k in ("uncond", "cond"):
            t0 = time.perf_counter()
            for _ in range(n):
                call[k]()
            torch.cuda.synchronize()
            res.setdefault(f"B{B}/{k}", []).append((time.perf_counter() - t0) / n * 1e6)
    print(B, {k: [round(x, 1) for x in v_] for k, v_ in res.items() if k.startswith(f"B{B}/")}, flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
