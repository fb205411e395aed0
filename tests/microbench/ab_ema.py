#!/usr/bin/env python3
"""What the exponential moving average of the parameters costs on one GPU.  (1) The replayed bs-256 step with ema_decay=None
against ema_decay=0.999, in the default arithmetic and in the precisions given as arguments (fp16: the guarded mode).  Every
measurement is a fresh child process holding ONE engine, the two settings alternating (as in ab_gradclip.py: two engines in one
process share the hardware queues).  (2) The launches alone on a buffer of the engine's size: mmdyn_adam_step (tick + Adam), the
fused mmdyn_adam_step_ema (tick + EMA tick + Adam with the average), and the separate form mmdyn_adam_step + mmdyn_ema_tick +
mmdyn_ema_update, each with the bytes it moves over the time."""
import os
import statistics
import subprocess
import sys
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-dynamics_amd"))
from mmdyn_hip import ops  # noqa: E402
from mmdyn_hip.engine import MVAEStep  # noqa: E402
from mmdyn_hip.models import setup_model, NoiseSource  # noqa: E402
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_state_dict  # noqa: E402

HBM_TBS = 8.0          # MI355X peak HBM3E rate, TB/s
DEV = "cuda"
DECAY = 0.999


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def show(name, t, extra=""):
    print(f"  {name:58s} {statistics.median(t) * 1e3:9.2f} us  ({min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f}) {extra}", flush=True)


def warm_clocks():
    x = torch.randn(8192, 8192, device=DEV)
    for _ in range(40):                      # ~0.3 s of matrix work: clocks up before anything is timed
        x @ x
    torch.cuda.synchronize()


def engine(precision, ema_decay):
    m = setup_model("cnn-mvae", cross_modal=True, condition_dim=0, input_dim=4096, architecture="cnn", conditional=False,
                    categorical_conditions=False, latent_size=256, use_pose=True)
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    return MVAEStep(m.to(DEV).train(), noise=NoiseSource(1234), precision=precision, ema_decay=ema_decay)


def step_child(precision, decay, B=256, rounds=7, reps=20):
    """One engine, one process: prints the per-step times of `rounds` windows of `reps` replays (ms) and the buffer size."""
    warm_clocks()
    inputs, targets = ([x.to(DEV) for x in xs] for xs in seeded_batch(B, 1234))
    e = engine(precision, None if decay == "None" else float(decay))
    for _ in range(3):                       # warm-up step + capture, then replays
        e.train_step_graphed(inputs, targets, 0.02)
    torch.cuda.synchronize()
    t = [event_ms(lambda: e.train_step_graphed(inputs, targets, 0.02), reps) for _ in range(rounds)]
    print("TIMES", e.params.total, e.skipped_steps, e.ema_updates, *t, flush=True)
    e.close()


def steps(precision, processes=3):
    times, n = {"None": [], str(DECAY): []}, 0
    for _ in range(processes):
        for decay in times:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", precision, decay], capture_output=True,
                                 text=True, timeout=200, check=True).stdout
            f = [l for l in out.splitlines() if l.startswith("TIMES")][0].split()
            n, skipped, updates = int(f[1]), int(f[2]), int(f[3])
            assert skipped == 0 and (updates > 0) == (decay != "None")
            times[decay] += [float(x) for x in f[4:]]
    print(f"replayed step, bs 256, {precision} ({processes} processes per setting, alternating):")
    for decay in times:
        show(f"ema_decay={decay}", times[decay])
    d = statistics.median(times[str(DECAY)]) - statistics.median(times["None"])
    print(f"  difference of the medians {d * 1e3:.2f} us; two more streams of {4 * n / 1e6:.1f} MB at {HBM_TBS} TB/s = "
          f"{2 * 4 * n / (HBM_TBS * 1e12) * 1e6:.2f} us", flush=True)
    return n


def launches(n, rounds=7, reps=50):
    H = ops.B
    g = torch.randn(n, device=DEV) * 0.01
    p, m, v = torch.randn(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    e = p.clone()
    state, es = torch.zeros(6, dtype=torch.float64, device=DEV), ops.new_ema_state(DECAY, False, DEV)
    adam = (1e-3, 0.9, 0.999, 1e-8, 1.0)

    def separate():
        H.adam_step(p, g, m, v, state, *adam)
        H.ema_tick(es)
        H.ema_update(e, p, es)

    # streams of n fp32 values each launch set moves: Adam reads p g m v and writes p m v; the average adds a read and a write
    variants = [("adam_step (tick + Adam)", lambda: H.adam_step(p, g, m, v, state, *adam), 7),
                ("adam_step_ema (tick + EMA tick + fused Adam)", lambda: H.adam_step_ema(p, g, m, v, e, state, None, es, *adam), 9),
                ("adam_step + ema_tick + ema_update (separate)", separate, 10),
                ("ema_tick", lambda: H.ema_tick(es), 0),
                ("ema_update", lambda: H.ema_update(e, p, es), 3)]
    times = {k: [] for k, _, _ in variants}
    for k, fn, _ in variants:
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn, _ in variants:
            times[k].append(event_ms(fn, reps))
    print(f"launches alone, n = {n} ({4 * n / 1e6:.1f} MB per stream); one stream at {HBM_TBS} TB/s = "
          f"{4 * n / (HBM_TBS * 1e12) * 1e6:.2f} us:")
    for k, _, streams in variants:
        t = statistics.median(times[k])
        show(k, times[k], f"{streams} streams, {streams * 4 * n / (t * 1e-3) / 1e12:.2f} TB/s" if streams else "")


def main():
    if sys.argv[1:2] == ["--step"]:
        return step_child(sys.argv[2], sys.argv[3])
    n = 0
    for precision in ["fp32x3"] + sys.argv[1:]:          # (children first: this process opens the GPU only afterwards)
        n = steps(precision)
    print(torch.cuda.get_device_name(0))
    warm_clocks()
    launches(n)


if __name__ == "__main__":
    main()
