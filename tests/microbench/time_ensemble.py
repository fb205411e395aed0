"""N sampled T-step trajectories per request row and their per-element mean / variance, served two ways (docs/LAB_NOTES.md S), on one
MI355X, T = 16, 64 x 64, fp32x3, touch observed under a mixed table, (B, N) = (32, 8) and (4, 64):
  (a) repeat:   what a caller wrote before ``rollout(samples=)`` -- ONE replayed ``rollout(sample=True)`` of the request repeated N
                times (observations and table repeated N times), then torch ``mean`` / ``var(unbiased=False)`` over the N axis of
                the three trajectory tensors on the device;
  (b) ensemble: ONE replayed ``rollout(sample=True, samples=N)``.
Device events around each call, 20 warm-up calls, median and spread (min .. max) of 200 calls, three rounds in alternation; the
spread of (a) between its rounds is the yardstick for (b) - (a).  Then the feed kernel alone on the operands of one step: device
events around 200 back-to-back launches, against the bytes it must move -- per group (2 N + 2) B row_len 4 (recon read, out
written, mean and var written) plus the observation rows it takes.

    python tests/microbench/time_ensemble.py [out.json]
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-dynamics_amd")]
import torch
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import setup_model
from mmdyn_hip.models.functional import availability_table
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
for B, N in ((32, 8), (4, 64)):
    g = torch.Generator().manual_seed(B)
    v, t, p = (torch.rand(B, 3, 64, 64, generator=g).to(dev), torch.rand(B, 3, 64, 64, generator=g).to(dev),
               torch.rand(B, 7, generator=g).to(dev))
    touch = torch.rand(T, B, 3, 64, 64, generator=g).to(dev)
    seen = (torch.rand(T, B, 3, generator=g) < 0.5).float()
    rep = lambda x, d=0: x.repeat((1,) * d + (N,) + (1,) * (x.dim() - d - 1))
    vN, tN, pN, touchN, seenN = rep(v), rep(t), rep(p), rep(touch, 1), rep(seen, 1)

    def repeat():
        r = eng.rollout([vN, tN], pose=pN, steps=T, sample=True, observed=[None, touchN, None], observed_available=seenN)
        out = []
        for k in ("visual", "tactile", "pose"):
            x = r[k].view((T, N, B) + tuple(r[k].shape[2:]))
            out += [x.mean(1), x.var(1, unbiased=False)]
        return out

    call = {"repeat": repeat,
            "ensemble": lambda: eng.rollout([v, t], pose=p, steps=T, sample=True, samples=N, observed=[None, touch, None],
                                            observed_available=seen)}
    for rnd in range(3):
        for k in ("repeat", "ensemble"):
            res.setdefault(f"B{B}N{N}/{k}", []).append(timed(call[k]))
    # the feed kernel alone, on one step's operands
    table = availability_table(seen[0], B, dev)
    groups, moved = [], 0
    for col, row in enumerate(((3, 64, 64), (3, 64, 64), (7,))):
        groups.append(dict(recon=torch.randn((N * B,) + row, device=dev), obs=touch[0] if col == 1 else None,
                           out=torch.empty((N * B,) + row, device=dev), mean=torch.empty((B,) + row, device=dev),
                           var=torch.empty((B,) + row, device=dev), spread=torch.zeros(B, dtype=torch.float64, device=dev),
                           logits=col < 2, column=col))
        n = groups[-1]["mean"][0].numel()
        moved += (2 * N + 2) * B * n * 4 + (int(seen[0, :, 1].sum()) * n * 4 if col == 1 else 0)
    feed = lambda: ops.B.ensemble_feed(groups, table, N, B)
    for _ in range(20):
        feed()
    rates = []
    for rnd in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(200):
            feed()
        b.record()
        b.synchronize()
        us = a.elapsed_time(b) * 1e3 / 200
        rates.append([round(us, 2), round(moved / us / 1e6, 3)])
    res[f"B{B}N{N}/feed"] = {"bytes": moved, "us_and_TB_per_s": rates}
    print(B, N, {k: v_ for k, v_ in res.items() if k.startswith(f"B{B}N{N}/")},
          "(us per T = 16 call: median, min, max per round; feed: us per launch and TB/s over the bytes it must move)", flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
