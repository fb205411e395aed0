#!/usr/bin/env python3
"""What clipping by the global norm costs on one GPU.  (1) The replayed bs-256 step with max_grad_norm=None against max_grad_norm=inf
(the norm is taken and reported, nothing is clipped: the same update), in the default arithmetic and in the precisions given as
arguments (fp16 / fp16s: the guarded modes).  Every measurement is a fresh child process holding ONE engine, the two settings
alternating: two engines in one process share the hardware queues, and the one created second measured 0.5 ms slower per step
whatever its setting.  (2) The new launches alone on
the engine's gradient buffer: the two launches of grad_sumsq, grad_clip_coef, and their sum against bytes over the HBM rate.
(3) The guard of the fp16 modes: grad_nonfinite + tick + Adam (mmdyn_adam_step_guarded) after a grad_sumsq + grad_clip_coef --
two reads of the gradient for the two decisions -- against the one-read form (grad_sumsq + grad_clip_coef + mmdyn_adam_step_clipped
guarded)."""
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


def engine(precision, max_grad_norm, B):
    m = setup_model("cnn-mvae", cross_modal=True, condition_dim=0, input_dim=4096, architecture="cnn", conditional=False,
                    categorical_conditions=False, latent_size=256, use_pose=True)
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    return MVAEStep(m.to(DEV).train(), noise=NoiseSource(1234), precision=precision, max_grad_norm=max_grad_norm)


def step_child(precision, norm, B=256, rounds=7, reps=20):
    """One engine, one process: prints the per-step times of `rounds` windows of `reps` replays (ms) and the buffer size."""
    warm_clocks()
    inputs, targets = ([x.to(DEV) for x in xs] for xs in seeded_batch(B, 1234))
    e = engine(precision, None if norm == "None" else float(norm), B)
    for _ in range(3):                       # warm-up step + capture, then replays
        e.train_step_graphed(inputs, targets, 0.02)
    torch.cuda.synchronize()
    t = [event_ms(lambda: e.train_step_graphed(inputs, targets, 0.02), reps) for _ in range(rounds)]
    print("TIMES", e.params.total, e.skipped_steps, *t, flush=True)
    e.close()


def steps(precision, processes=3):
    times, n = {"None": [], "inf": []}, 0
    for _ in range(processes):
        for norm in times:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", precision, norm], capture_output=True,
                                 text=True, timeout=200, check=True).stdout
            f = [l for l in out.splitlines() if l.startswith("TIMES")][0].split()
            n, skipped = int(f[1]), int(f[2])
            assert skipped == 0
            times[norm] += [float(x) for x in f[3:]]
    print(f"replayed step, bs 256, {precision} ({processes} processes per setting, alternating):")
    for norm in times:
        show(f"max_grad_norm={norm}", times[norm])
    d = statistics.median(times["inf"]) - statistics.median(times["None"])
    print(f"  difference of the medians {d * 1e3:.2f} us; one more read of {4 * n / 1e6:.1f} MB at {HBM_TBS} TB/s = "
          f"{4 * n / (HBM_TBS * 1e12) * 1e6:.2f} us", flush=True)
    return n


def launches(n, rounds=7, reps=50):
    H = ops.B
    g = torch.randn(n, device=DEV) * 0.01
    p, m, v = torch.randn(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ws = torch.empty(H.grad_sumsq_blocks(n), dtype=torch.float64, device=DEV)
    clip, state = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
    inf = float("inf")

    def two_reads():
        H.grad_sumsq(g, ws, clip)
        H.grad_clip_coef(clip, 1.0, inf)
        H.adam_step(p, g, m, v, state, 1e-3, 0.9, 0.999, 1e-8, 1.0, guarded=True)

    def one_read():
        H.grad_sumsq(g, ws, clip)
        H.grad_clip_coef(clip, 1.0, inf)
        H.adam_step_clipped(p, g, m, v, state, clip, 1e-3, 0.9, 0.999, 1e-8, 1.0, guarded=True)

    variants = [("grad_sumsq (two launches)", lambda: H.grad_sumsq(g, ws, clip)),
                ("grad_clip_coef", lambda: H.grad_clip_coef(clip, 1.0, inf)),
                ("grad_sumsq + grad_clip_coef", lambda: (H.grad_sumsq(g, ws, clip), H.grad_clip_coef(clip, 1.0, inf))),
                ("adam_step (tick + Adam)", lambda: H.adam_step(p, g, m, v, state, 1e-3, 0.9, 0.999, 1e-8, 1.0)),
                ("adam_step_clipped (tick + Adam)", lambda: H.adam_step_clipped(p, g, m, v, state, clip, 1e-3, 0.9, 0.999, 1e-8, 1.0)),
                ("guard: sumsq + coef + adam_step_guarded (two reads)", two_reads),
                ("guard: sumsq + coef + adam_step_clipped guarded (one read)", one_read)]
    times = {k: [] for k, _ in variants}
    for k, fn in variants:
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in variants:
            times[k].append(event_ms(fn, reps))
    print(f"launches alone, n = {n} ({4 * n / 1e6:.1f} MB, {H.grad_sumsq_blocks(n)} partial sums); reading it once at {HBM_TBS} TB/s = "
          f"{4 * n / (HBM_TBS * 1e12) * 1e6:.2f} us:")
    for k, _ in variants:
        t = statistics.median(times[k])
        show(k, times[k], f"{4 * n / (t * 1e-3) / 1e12:.2f} TB/s of gradient" if "sumsq" in k and "guard" not in k else "")


def warm_clocks():
    x = torch.randn(8192, 8192, device=DEV)
    for _ in range(40):                      # ~0.3 s of matrix work: clocks up before anything is timed
        x @ x
    torch.cuda.synchronize()


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
