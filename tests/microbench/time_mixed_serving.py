"""A batch whose rows hold different modality subsets, served three ways (docs/LAB_NOTES.md K), on one MI355X at batch 7 / 64 / 256
with the seven subsets of {visual, tactile, pose} in equal shares:
  (a) split:  what the engine offered before per-row availability -- gather the rows of each subset into a sub-batch, one
              replayed ``forward`` per subset (seven captured graphs), scatter the rows of means / log_var / reconstructions back;
  (b) mixed:  ONE replayed ``forward(available=)`` on the whole batch;
  (c) joint:  one replayed ``forward`` of the whole batch with every modality -- the floor for (b).
Device events around each request, 10 warm-up requests, median and spread (min .. max) of 60 replays, three rounds in alternation.

    python tests/microbench/time_mixed_serving.py [out.json]
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-dynamics_amd")]
import torch
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import setup_model
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats

dev = "cuda"
SUBSETS = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]
m = setup_model("cnn-mvae", cross_modal=True, input_dim=4096, architecture="cnn", latent_size=256, use_pose=True, conditional=False,
                categorical_conditions=False, condition_dim=0)
m.load_state_dict(seeded_running_stats(seeded_state_dict(m.state_dict(), 0)))
eng = MVAEInference(m.to(dev).eval(), seed=1)


def timed(fn, n=60, warm=10):
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
for B in (7, 64, 256):
    g = torch.Generator().manual_seed(B)
    v, t, p = (torch.rand(B, 3, 64, 64, generator=g).to(dev), torch.rand(B, 3, 64, 64, generator=g).to(dev),
               torch.rand(B, 7, generator=g).to(dev))
    rows = [torch.arange(i, B, 7, device=dev) for i in range(7)]                  # subset i holds the rows i, i + 7, ...
    avail = torch.zeros(B, 3, device=dev)
    for i, s in enumerate(SUBSETS):
        avail[rows[i]] = torch.tensor(s, dtype=torch.float32, device=dev)
    outs = [torch.empty(B, 3, 64, 64, device=dev), torch.empty(B, 3, 64, 64, device=dev), torch.empty(B, 7, device=dev),
            torch.empty(B, 256, device=dev), torch.empty(B, 256, device=dev)]

    def split():
        for i, s in enumerate(SUBSETS):
            r = rows[i]
            if not len(r):
                continue
            got = eng.forward([v[r] if s[0] else None, t[r] if s[1] else None], pose=p[r] if s[2] else None)
            for dst, src in zip(outs, got):
                dst[r] = src
        return outs

    call = {"split": split, "mixed": lambda: eng.forward([v, t], pose=p, available=avail),
            "joint": lambda: eng.forward([v, t], pose=p)}
    for rnd in range(3):
        for k in ("split", "mixed", "joint"):
            res.setdefault(f"B{B}/{k}", []).append(timed(call[k]))
    print(B, {k: v_ for k, v_ in res.items() if k.startswith(f"B{B}/")}, "(us: median, min, max per round)", flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
