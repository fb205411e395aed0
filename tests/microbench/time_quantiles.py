"""Per-element quantiles of N sampled T-step trajectories per request row, served two ways (docs/LAB_NOTES.md AB), on one MI355X,
T = 16, 64 x 64, fp32x3, Q = 3 quantiles (0.05, 0.5, 0.95), touch observed under a mixed table, (B, N) = (32, 8) and (4, 64):
  (a) sort:      what a caller can do without ``rollout(quantiles=)`` -- ONE replayed ``rollout(sample=True, samples=N)``, then
                 ``torch.sort`` over the N axis of the three kept trajectory tensors and the same interpolation in torch
                 (``torch.quantile`` refuses tensors of this size).  Under observations these are the quantiles of the STATE, not
                 of the prediction: the baseline cannot produce the latter;
  (b) quantiles: ONE replayed ``rollout(sample=True, samples=N, quantiles=...)``;
  (c) ensemble:  the replayed ``rollout(sample=True, samples=N)`` alone, for what the T extra launches of (b) cost.
Device events around each call, 10 warm-up calls, median and spread (min .. max) of 100 calls, three rounds in alternation; the
spread of (a) between its rounds is the yardstick for (b) - (a).  Then the quantile kernel alone on the operands of one step: device
events around 200 back-to-back launches, against the bytes it must move -- per group (N + Q) B row_len 4 (src read, out written).

    python tests/microbench/time_quantiles.py [out.json]
"""
import json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-dynamics_amd")]
import torch
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import setup_model
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats

dev, T, QS = "cuda", 16, (0.05, 0.5, 0.95)
m = setup_model("cnn-mvae", cross_modal=True, input_dim=4096, architecture="cnn", latent_size=256, use_pose=True, conditional=False,
                categorical_conditions=False, condition_dim=0)
m.load_state_dict(seeded_running_stats(seeded_state_dict(m.state_dict(), 0)))
eng = MVAEInference(m.to(dev).eval(), seed=1)


def timed(fn, n=100, warm=10):
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
    h = [q * (N - 1) for q in QS]
    lo = [min(int(math.floor(x)), N - 1) for x in h]
    frac = [x - l for x, l in zip(h, lo)]
    kw = dict(pose=p, steps=T, sample=True, samples=N, observed=[None, touch, None], observed_available=seen)

    def sort():
        r = eng.rollout([v, t], **kw)
        out = []
        for k in ("visual", "tactile", "pose"):
            s = torch.sort(r[k], dim=1).values
            qs = []
            for l, f in zip(lo, frac):
                a = s[:, l]
                if f != 0.0:
                    a64 = a.double()
                    a = (a64 + f * (s[:, min(l + 1, N - 1)].double() - a64)).float()
                qs.append(a)
            out.append(torch.stack(qs, 1))
        return out

    call = {"sort": sort, "quantiles": lambda: eng.rollout([v, t], quantiles=QS, **kw), "ensemble": lambda: eng.rollout([v, t], **kw)}
    for rnd in range(3):
        for k in ("sort", "quantiles", "ensemble"):
            res.setdefault(f"B{B}N{N}/{k}", []).append(timed(call[k]))
    # the quantile kernel alone, on one step's operands
    groups, moved, Q = [], 0, len(QS)
    for row in ((3, 64, 64), (3, 64, 64), (7,)):
        groups.append(dict(src=torch.randn((N * B,) + row, device=dev), out=torch.empty((Q, B) + row, device=dev),
                           logits=len(row) == 3))
        moved += (N + Q) * B * groups[-1]["out"][0, 0].numel() * 4
    quant = lambda: ops.B.ensemble_quantiles(groups, lo, frac, N, B)
    for _ in range(20):
        quant()
    rates = []
    for rnd in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(200):
            quant()
        b.record()
        b.synchronize()
        us = a.elapsed_time(b) * 1e3 / 200
        rates.append([round(us, 2), round(moved / us / 1e6, 3)])
    res[f"B{B}N{N}/kernel"] = {"bytes": moved, "us_and_TB_per_s": rates}
    print(B, N, {k: v_ for k, v_ in res.items() if k.startswith(f"B{B}N{N}/")},
          "(us per T = 16 call: median, min, max per round; kernel: us per launch and TB/s over the bytes it must move)", flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
