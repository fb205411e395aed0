#!/usr/bin/env python3
"""bench.py -- cnn-mvae visuotactile+pose training throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one optimiser step of the cnn-mvae seq_modeling problem on one synthetic batch that is already
resident in HBM: the 7 modality-subset ELBO passes, backward and Adam (problems.py:148-156, 473-546), fp32,
64x64 visual + tactile + 7-DoF pose, 256 samples per GPU (weak scaling: pure data parallel, gradients
all-reduced over RCCL).  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, higher_is_better, dtype,
ms_per_step, config).  --full adds what takes runs of its own: the per-kernel HIP-event profile and the `roofline` object, the
other fp32 arithmetic timed beside the line (`native_fp32` / `alt_arithmetic`) and the CPU baseline (`cpu_baseline`):
    python bench.py --full
--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (seeded inputs: two builds compare file by file).

Other BASELINE configs (same JSON contract, the workload named in config.workload):
    configs[2]  python bench.py --dtype bf16s --batch 128
    configs[3]  python bench.py --image-size 128 --problem dyn_modeling --batch 128
    configs[4]  python bench.py --image-size 256 --dtype fp16 --batch 256
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "multimodal-dynamics_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_BF16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense bf16 (v_mfma_f32_32x32x16_bf16), no sparsity
PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense, = fp32 vector peak
PEAK_F16_MFMA_TFLOPS = 2500.0      # same rate as bf16 (MI355X_MICROARCH.md, matrix cores table)
KL_WEIGHT = 1.0 / 50               # epoch 0 of the reference's annealing schedule (problems.py:212-216)


def algo_gflop_per_sample(size=64, use_pose=True):
    """Algorithmic FLOPs of one train step per sample, counted as SURVEY.md section 8(d) does: every mathematically
    distinct contraction once (encoder trunks once per modality, image heads per pass, the 4 live passes of each image
    decoder, the pose encoder once, 4 live pose-decoder passes), forward + input gradient + weight gradient, no input
    gradient for a network's first layer.  size = 64 gives the survey's 1 012 188 160 MAC = 2.024 GFLOP; 128 / 256 apply
    the same count to the extended stacks of models/shapes.py."""
    from mmdyn_hip.models.shapes import extra_stages, encoder_channels, decoder_channels, FEAT, HID
    e = extra_stages(size)
    L = 256
    enc, H = [], size // 2
    first = H * H * 32 * 3 * 16
    for j, (cin, cout) in enumerate(encoder_channels(e)):
        last = j == 2 + e
        Ho = H - 3 if last else H // 2
        enc.append(Ho * Ho * cout * cin * 16)
        H = Ho
    fc = FEAT * HID
    trunk = first + sum(enc) + fc
    heads = HID * 2 * L
    enc_mod = trunk * 2 + (trunk - first) + 4 * 3 * heads            # fwd + wgrad + dgrad (not for conv1); heads x 4 passes
    dec, H = [], 5
    for j, (cin, cout) in enumerate(decoder_channels(e)):
        Ho = H + 3 if j == 0 else 2 * H
        dec.append(H * H * cin * cout * 16)          # transposed: every INPUT pixel meets all 16 taps
        H = Ho
    dec_pass = L * FEAT + sum(dec) + (2 * H) * (2 * H) * 3 * 32 * 4   # last layer: each output pixel sees 4 of the 16 taps
    macs = 2 * enc_mod + 2 * 4 * 3 * dec_pass
    if use_pose:
        macs += (7 * HID + HID * HID) * 2 + HID * HID + 3 * heads + 4 * 3 * (L * HID + HID * HID + HID * 7)
    return 2.0 * macs / 1e9


ALGO_GFLOP_PER_SAMPLE = 2.024      # SURVEY.md section 8(d), 64 x 64 (== algo_gflop_per_sample(64), asserted in main)


def _sha256(path):
    import hashlib
    try:
        return hashlib.sha256(open(path, "rb").read()).hexdigest()
    except OSError:
        return None


PEAK_HBM_BYTES_PER_S = 8.0e12       # MI355X_MICROARCH.md: HBM3E peak (spec); ~6.3 TB/s achievable


def sources_sha256():
    """sha-256 over the kernel sources (csrc/*.hip, *.h): the provenance key of the committed PMC profiles."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "multimodal-dynamics_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()


def pmc_traffic(workload_key):
    """HBM-side bytes of one step of this workload from the committed rocprofv3 PMC passes (profiles/r5/traffic_<key>.json, else r4's / r3's:
    FETCH_SIZE doubled per the gfx950 correction + WRITE_SIZE; profiles/collect_r5.sh traffic).  PMC counters cannot be
    read from inside this process, so the values are the last profiled ones -- WITH their provenance: the profile records
    the sha-256 of the kernel sources it was taken on, and the values are reported as None (plus the reason) when the
    sources have changed since.  Returns (dict | None, note)."""
    d = None
    for rnd in ("r6", "r5", "r4", "r3"):          # the latest round's collection first
        rel = ("profiles", rnd, f"traffic_{workload_key}.json")
        try:
            d = json.load(open(os.path.join(ROOT, *rel)))
            break
        except (OSError, ValueError):
            continue
    if d is None:
        return None, {"stale": f"no PMC profile committed for this workload (profiles/r6|r5|r4|r3/traffic_{workload_key}.json)"}
    note = {"profile": "/".join(rel), "collected": d.get("collected"), "sources_sha256": d.get("sources_sha256")}
    if d.get("sources_sha256") and d["sources_sha256"] == sources_sha256():
        return d, note
    note["stale"] = "kernel sources changed since the profile was collected"
    return None, note


def host_cpu_share():
    """CPU threads this process may really use: the cgroup quota if there is one, else the affinity mask."""
    n = len(os.sched_getaffinity(0))
    found = False
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n, found = min(n, max(1, int(float(quota) / float(period) + 0.5))), True
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            n, found = min(n, max(1, int(q / per + 0.5))), True
    except (OSError, ValueError):
        pass
    if not found:
        n = min(n, 16)          # a one-GPU box's documented CPU share
    return max(1, n)


def host_cpu_all():
    """os.cpu_count() as SURVEY.md section 8(d) specifies for the CPU baseline, bounded by the affinity mask and by a
    cgroup quota when one is visible (more runnable threads than the quota allows only thrash)."""
    n = min(os.cpu_count() or 1, len(os.sched_getaffinity(0)))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_baseline(batch, threads, size=64, budget_s=30.0):
    """The CPU oracle (a port of the reference path executing the reference's own schedule: 8 encoder + 14
    decoder forwards, autograd backward, Adam) timed on this box's host cores.  Bounded: a probe step at bs=32
    decides whether the full bs=256 step fits the budget; otherwise a bs=64 sample is timed."""
    from oracle import mvae_oracle as O
    from mmdyn_hip.models.shapes import state_dict_shapes
    from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_batch, seeded_noise
    torch.set_num_threads(threads)

    def run(bs, steps):
        prm, buf = O.split_state(seeded_state_dict(state_dict_shapes("cnn-mvae", use_pose=True, size=size), 0))
        inputs, targets = seeded_batch(bs, 1234, size=size)
        eps, masks = seeded_noise(bs, 256, 7, 8, 4321)
        opt = O.Adam([prm[k] for k in prm], lr=1e-3)
        times, loss = [], None
        for s in range(steps):
            t0 = time.perf_counter()
            opt.zero_grad()
            _, loss, _ = O.evaluate_mvae(prm, inputs, targets, eps, masks, KL_WEIGHT, 1000.0, True, buf)
            loss.backward()
            opt.step()
            times.append(time.perf_counter() - t0)
            print(f"[cpu_baseline] bs={bs} step {s}: {times[-1]:.2f} s ({threads} threads)", file=sys.stderr, flush=True)
        return times, float(loss.detach())

    pb = 32 if size == 64 else 8
    probe, _ = run(pb, 2)
    est_full = probe[-1] * (batch / float(pb))
    bs = batch if est_full * 3 <= 1.5 * budget_s else max(pb, min(batch, 64 if size == 64 else 16))
    n_timed = 6 if est_full * 7 <= budget_s else 2             # ~10-30 s of CPU work in total
    times, loss = run(bs, 1 + n_timed)
    best, med = min(times[1:]), sorted(times[1:])[len(times[1:]) // 2]
    cpu = "unknown CPU"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"value": bs / best, "unit": "samples/s", "cores": threads, "kind": "port",
            "sample": f"{n_timed} timed steps (+1 warm-up) of the cnn-mvae+pose {size}x{size} train step at bs={bs}; "
                      f"min {best:.2f} s/step (value), median {med:.2f} s/step; {cpu}, os.cpu_count()={os.cpu_count()}",
            "loss": loss}


_RESULT_FD = None


def _claim_stdout():
    """The contract is ONE JSON line on stdout.  Libraries write there too (RCCL prints a five-line version banner when
    its communicator is created), so the real stdout is set aside for the result and everything else -- C libraries
    included, they share file descriptor 1 -- goes to stderr."""
    global _RESULT_FD
    sys.stdout.flush()
    _RESULT_FD = os.dup(1)
    os.dup2(2, 1)


def _emit(obj):
    sys.stdout.flush()
    os.write(_RESULT_FD if _RESULT_FD is not None else 1, (json.dumps(obj) + "\n").encode())


DUMP_BYTES = 63 * 10 ** 6          # the .npy payloads of --dump-outputs (64 MB in all with their headers)


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each (name, tensor) as out_dir/<name>.npy, float64 kept, every other dtype as float32.  When the arrays
    exceed DUMP_BYTES together, every array above 1 MB is replaced by a sample of its flattened elements, in index order, the
    indices drawn from a fixed seed: the same elements in every run of the same arguments."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrs = [(name, (t.double() if t.dtype == torch.float64 else t.float()).detach().cpu().numpy()) for name, t in arrays]
    total = sum(a.nbytes for _, a in arrs)
    small = sum(a.nbytes for _, a in arrs if a.nbytes <= 2 ** 20)
    for name, a in arrs:
        if total > DUMP_BYTES and a.nbytes > 2 ** 20:
            n = a.size
            keep = int(n * (DUMP_BYTES - small) / (total - small))
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(n, keep, replace=False))]
            print(f"[bench] {name}: a seeded sample of {keep} of its {n} elements", file=sys.stderr)
        np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"[bench] outputs written to {out_dir}: {', '.join(n for n, _ in arrs)}", file=sys.stderr)


def _self_launch(n):
    """``python bench.py --gpus N`` without a launcher: start the N ranks ourselves, the way the driver does for N > 1
    (``python -m torch.distributed.run --nproc-per-node N``), as a CHILD process -- this process has not touched the GPU
    and never will; it relays rank 0's single JSON line and exits with the child's return code.  (The reference has no
    counterpart: it is a single process, problems.py:52, 388.)"""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    print(f"[bench] --gpus {n} without WORLD_SIZE: launching {n} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=sys.stderr, text=True)
    lines = [ln for ln in proc.stdout.read().splitlines() if ln.startswith("{")]
    rc = proc.wait()
    for ln in lines[-1:]:
        _emit(json.loads(ln))
    if rc != 0 or not lines:
        raise SystemExit(rc or 1)


def main():
    _claim_stdout()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256, help="samples per GPU")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the per-kernel profile and roofline, the other fp32 "
                         "arithmetic beside the line and the CPU baseline (off: set up, warm up, time the steps, print the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (loss, partial ELBOs, updated parameters and "
                         "BatchNorm buffers; --infer: the forward's outputs) as DIR/<name>.npy, float32 / float64, at most 64 MB in all "
                         "(a fixed seeded sample of an array beyond that)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-graph", action="store_true", help="do not replay the step from a HIP graph")
    ap.add_argument("--breakdown", action="store_true", help="print the per-kernel table to stderr")
    ap.add_argument("--image-size", type=int, choices=(64, 128, 256), default=64,
                    help="64: the reference's only input size (BASELINE configs[1], default).  128 / 256: the extended stacks of "
                         "models/shapes.py (configs[3] / configs[4]; no reference architecture exists for them)")
    ap.add_argument("--problem", choices=("seq_modeling", "dyn_modeling"), default="seq_modeling",
                    help="dyn_modeling (configs[3]): the batch is --seq-length frames per sequence, targets are the next frames "
                         "(DynModeling.parse_input, problems.py:765-803); the step itself is the same computation")
    ap.add_argument("--seq-length", type=int, default=4)
    ap.add_argument("--dtype", choices=("f32", "f32x3", "bf16", "bf16s", "fp16", "fp16s"), default="f32x3",
                    help="f32x3 (default): BASELINE configs[1] with the fp32 GEMMs on the bf16 matrix cores through the exact "
                         "three-term split of their fp32 operands (fp32 storage, results and tolerances; with --full the native fp32 run is "
                         "timed by the same process and reported beside it as native_fp32).  f32: the native fp32 matrix cores.  bf16s: bf16 activation storage + bf16 matrix "
                         "cores, fp32 accumulate / master weights = the per-GPU share of configs[2] (use --batch 128).  "
                         "bf16: bf16 matrix-core operands only (fp32 storage).  fp16: fp16 matrix-core operands, fp32 "
                         "accumulate / storage / master weights (configs[4]).  fp16s: fp16 + fp16 activation storage")
    ap.add_argument("--defer-wgrad", choices=("auto", "on", "off"), default="auto",
                    help="decoder weight-gradient GEMMs on two extra streams next to the encoder backward (auto: the engine's rule, "
                         "on in fp32 on one GPU)")
    ap.add_argument("--sync-bn", action="store_true",
                    help="BatchNorm statistics over the global batch (N > 1; one small all-reduce per BatchNorm layer and "
                         "direction, captured into the lanes' HIP graphs, each lane on its own RCCL communicator).  Default: "
                         "local statistics")
    ap.add_argument("--no-alt", action="store_true",
                    help="(--full) skip the extra timed run in the other fp32 arithmetic (native fp32 beside the default f32x3 line, f32x3 "
                         "beside --dtype f32) that a one-GPU run reports next to its value")
    ap.add_argument("--infer", action="store_true",
                    help="time forward-only inference instead (model.eval(): joint visual+tactile+pose pass through the "
                         "module API, running-estimate BatchNorm); prints its own JSON line, not the BASELINE metric")
    ap.add_argument("--no-grouped-heads", action="store_true",
                    help="A/B switch: launch the heads of the three encoders one by one instead of as grouped launches")
    ap.add_argument("--no-planes", action="store_true",
                    help="A/B switch (f32x3): every GEMM splits its fp32 operands inside the kernel (the round-4 structure) instead of "
                         "taking them already split where the plane-ring kernel serves the launch")
    ap.add_argument("--no-patch-planes", action="store_true",
                    help="A/B switch (f32x3): the 32-channel up-sampling layers (tconv_patch_kernel) keep fp32 operands")
    ap.add_argument("--inkernel-finish", action="store_true",
                    help="A/B switch (LAB library only: MMDYN_HIP_LIB=.../libmmdyn_hip_lab.so): the persistent stream-K kernels finish "
                         "split tiles inside the launch instead of parking the pieces for a fix-up launch (measured slower: LAB_NOTES H.a)")
    ap.add_argument("--ab-off", default="", help="A/B switches (comma list): fused_bce, copy_many -- turn a round-6 change off")
    ap.add_argument("--ticket-max-work", type=int, default=None,
                    help="A/B switch: BatchNorm finalize launches with at most this many (group, tile) partial-sum rows take the "
                         "single-launch last-block-finishes form (ops.HipBackend.ticket_max_work)")
    ap.add_argument("--fc-planes", action="store_true",
                    help="A/B switch (f32x3): the decoder's Linear forward and the encoder FC layer's input gradient on the DENSE mode of "
                         "the plane-ring kernel (measured 0.6 %% slower on the two-lane step: layers.FC_PLANES)")
    ap.add_argument("--single-lane", action="store_true",
                    help="no visual/tactile stream overlap: per-kernel durations in a rocprofv3 trace then match "
                         "the roofline object's live HIP-event measurement")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return _self_launch(args.gpus)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # MMDYN_BENCH_DRYRUN=emu (tests only): rehearse the multi-rank control flow of this script -- rendezvous, sharding,
    # barriers, max-over-ranks timing, the JSON line -- on CPU with gloo and the kernels replaced by the test suite's
    # emulation.  The numbers are meaningless and the line says so; the product path below never takes this branch.
    dry = os.environ.get("MMDYN_BENCH_DRYRUN") == "emu"
    rehearse = False
    if dry:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from emu_backend import EmuBackend
        from mmdyn_hip import ops as _ops
        _ops.set_backend(EmuBackend())
        torch.set_num_threads(2)
        dev = torch.device("cpu")
        args.no_graph, args.no_cpu_baseline = True, True
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a ROCm GPU (the HIP path has no CPU fallback)")
        # MMDYN_BENCH_REHEARSE_ONE_GPU=1 (rehearsal on a one-GPU box): every rank on cuda:0, collectives over gloo -- the real
        # kernels, HIP graphs and the data-parallel schedule (buckets between the graph rows), without RCCL.  The line says so.
        rehearse = os.environ.get("MMDYN_BENCH_REHEARSE_ONE_GPU") == "1"
        if rehearse:
            local_rank = 0
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    sync = (lambda: None) if dry else torch.cuda.synchronize
    pg = None
    if world > 1 or os.environ.get("MMDYN_BENCH_FORCE_PG") == "1":      # (the flag: 1-rank rehearsal of the RCCL path)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if dry or rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        pg = dist.group.WORLD
    if args.gpus != world and rank == 0:
        print(f"[bench] --gpus {args.gpus} but WORLD_SIZE={world}: one process per GPU is launched by torch.distributed.run "
              f"--nproc-per-node N; reporting n_gpus={world}", file=sys.stderr)

    from mmdyn_hip.engine import MVAEStep
    from mmdyn_hip.models import setup_model, NoiseSource
    from mmdyn_hip.profiling import profile_step
    for sw in [x for x in args.ab_off.split(",") if x]:
        from mmdyn_hip import layers as _lay, engine as _eng
        if sw == "fused_bce":
            _eng.FUSED_BCE = False
        elif sw == "copy_many":
            _eng.COPY_MANY = False
        else:
            raise SystemExit(f"--ab-off: unknown switch {sw}")
    if args.ticket_max_work is not None:
        from mmdyn_hip import ops as _ops3
        _ops3.B.ticket_max_work = args.ticket_max_work
    if args.fc_planes:
        from mmdyn_hip import layers as _lay2
        _lay2.FC_PLANES = True
    if args.inkernel_finish:
        from mmdyn_hip import ops as _ops2
        _ops2.B.use_flags = True
    if args.no_planes:
        from mmdyn_hip import layers as _layers
        _layers.PLANES = False
    if args.no_patch_planes:
        from mmdyn_hip import layers as _layers
        _layers.PATCH_PLANES = False
    from mmdyn_hip.utils.seeded_init import seeded_batch

    S = args.image_size
    PRECS = {"f32": "fp32", "f32x3": "fp32x3", "bf16": "bf16", "bf16s": "bf16s", "fp16": "fp16", "fp16s": "fp16s"}
    assert abs(algo_gflop_per_sample(64) - ALGO_GFLOP_PER_SAMPLE) < 1e-3
    gflop_per_sample = algo_gflop_per_sample(S)

    def new_model():
        torch.manual_seed(0)
        return setup_model("cnn-mvae", cross_modal=True, condition_dim=0, input_dim=S * S, architecture="cnn",
                           conditional=False, categorical_conditions=False, latent_size=256, use_pose=True).to(dev).train()

    if args.infer:
        model = new_model()
        inputs, _ = seeded_batch(args.batch, 1234 + rank, size=S)
        v, t, p = [z.to(dev) for z in inputs]
        from mmdyn_hip.engine import MVAEInference
        model.eval()
        eng = MVAEInference(model, precision=PRECS[args.dtype],
                            use_graph=not args.no_graph,
                            seed=1234 + rank)
        for _ in range(args.warmup):
            eng([v, t], pose=p)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = eng([v, t], pose=p)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, [(name, x) for name, x in zip(
                ("visual_recon", "tactile_recon", "pose_recon", "means", "log_var"), out) if x is not None])
        _emit({"metric": "visuotactile samples/sec (inference, joint v+t+p forward, eval mode)",
                          "value": args.batch * args.steps / dt, "unit": "samples/s", "n_gpus": 1, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
                          "dtype": args.dtype, "data": "synthetic",
                          "config": {"workload": f"cnn-mvae joint inference forward, bs={args.batch}, engine.MVAEInference "
                                                 f"(prepacked weights, two streams, {'eager' if args.no_graph else 'HIP graph'})",
                                     "algorithmic_gflop_per_sample": 0.274,
                                     "tflops": args.batch * args.steps / dt * 0.274e9 / 1e12}})
        return

    inputs, targets = seeded_batch(args.batch, 1234 + rank, size=S)
    inputs, targets = [x.to(dev) for x in inputs], [x.to(dev) for x in targets]
    if args.problem == "dyn_modeling":
        # the frames of --seq-length-long sequences are the samples; the target of a frame is the next frame of its
        # sequence, the last frame's target is the sequence's final target (DynModeling.parse_input, problems.py:765-803:
        # roll by -1 and patch the sequence ends; the pose target is rolled without the patch, as the reference does)
        Lq = args.seq_length
        if args.batch % Lq:
            raise SystemExit("--batch must be a multiple of --seq-length for dyn_modeling")
        final = targets
        targets = [torch.roll(x, -1, dims=0) for x in inputs]
        for k in (0, 1):
            targets[k][Lq - 1::Lq] = final[k][Lq - 1::Lq]

    def measure(dtype, with_pg, profile, dump_dir=None):
        """W warm-up + K timed steps of the workload in one arithmetic (between barrier + synchronize, max over ranks), then
        (dump_dir) what the last timed step computed, then (profile) the per-kernel HIP-event profile of one more (untimed,
        single-lane, eager) step.  Same seeds for every arithmetic."""
        model = new_model()
        step = MVAEStep(model, lr=1e-3, pose_multiplier=1000.0, noise=NoiseSource(1234 + rank), process_group=pg if with_pg else None,
                        world_size=world if with_pg else 1, two_lanes=not args.single_lane,
                        precision=PRECS[dtype], defer_wgrad={"auto": None, "on": True, "off": False}[args.defer_wgrad],
                        sync_bn=args.sync_bn and pg is not None and with_pg, group_heads=not args.no_grouped_heads)

        def eager_step():
            return step.train_step(inputs, targets, KL_WEIGHT)

        def one_step():
            if args.no_graph:
                return step.train_step(inputs, targets, KL_WEIGHT)
            return step.train_step_graphed(inputs, targets, KL_WEIGHT)

        for _ in range(args.warmup):
            one_step()
        sync()
        if pg is not None and with_pg:
            dist.barrier()
            sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = one_step()
        host_enqueue = time.perf_counter() - t0      # host side done enqueueing; the GPU is still running if it is ahead
        sync()
        if pg is not None and with_pg:
            dist.barrier()
            sync()
        elapsed = time.perf_counter() - t0
        if pg is not None and with_pg:
            t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t)
        res = {"dtype": dtype, "elapsed": elapsed, "host_enqueue": host_enqueue, "final_loss": float(loss)}
        if dump_dir and rank == 0:
            # what a caller of the step holds after it: the loss and the partial ELBO of each modality subset of the last
            # timed step, the parameters its Adam update wrote and the BatchNorm running buffers, in module order
            dump_outputs(dump_dir, [("loss", step.loss), ("partials", step.partials[:step.P]),
                                    ("params", torch.cat([p.detach().reshape(-1).float() for p in model.parameters()])),
                                    ("buffers", torch.cat([b.detach().reshape(-1).double() for b in model.buffers()]))])
        # per-kernel timing of one extra (untimed) step, HIP events on the launch stream (one lane, eager launches: per-kernel
        # durations are then not inflated by the other lane's kernels).  The step is profiled TWICE and the second pass is
        # kept: the first eager step after the graph replays draws its scratch tensors (stream-K slabs, partial-sum tables)
        # from the default memory pool for the first time, and that allocation sits between the two events of the launch that
        # asked for it (the k4 s1 p0 layer read 282 us by events against 204 us in the rocprofv3 trace of the same run:
        # VERDICT r4, profiles/r5/event_vs_trace_s1p0.txt)
        kern, by_shape = {}, {}
        if profile and not dry:
            lanes_on, step.lanes.on = step.lanes.on, False
            profile_step(eager_step)
            kern = profile_step(eager_step)
            by_shape = dict(profile_step.by_shape)
            step.lanes.on = lanes_on
        res["kern"], res["by_shape"] = kern, by_shape
        step.close()
        del step, model
        if not dry:
            torch.cuda.empty_cache()
        return res

    def roofline_of(res, sps):
        """The `roofline` object of one measured arithmetic: the dominant MFMA kernel family by live HIP events against the
        dense peak of the matrix pipe it runs on, the committed PMC traffic of the same workload beside it."""
        dtype, kern = res["dtype"], res["kern"]
        ig = kern.get("igemm_nt", {"ms": 0.0, "flops": 0.0, "calls": 0, "bytes": 0.0})
        wg = kern.get("wgrad_tn", {"ms": 0.0, "flops": 0.0, "calls": 0, "bytes": 0.0})
        dom = ig if ig["ms"] >= wg["ms"] else wg
        achieved = dom["flops"] / (dom["ms"] * 1e-3) / 1e12 if dom["ms"] > 0 else 0.0
        total_ms = sum(d["ms"] for d in kern.values())
        peak = PEAK_FP32_MFMA_TFLOPS if dtype == "f32" else (PEAK_F16_MFMA_TFLOPS if dtype in ("fp16", "fp16s") else PEAK_BF16_MFMA_TFLOPS)
        if dtype == "f32x3":
            # fp32 products as SIX bf16 products of the exact three-term operand split: an algorithmic (fp32) flop costs six flops
            # of the bf16 matrix pipe, so the ceiling for algorithmic flops is the dense bf16 peak / 6 (2.65 x the native fp32 peak)
            peak = PEAK_BF16_MFMA_TFLOPS / 6.0
        # byte side: the committed PMC passes of THIS workload (whole step + the implicit-GEMM launches)
        wkey = f"s{S}_{dtype}_b{args.batch}_{args.problem}"
        prof, traffic_note = pmc_traffic(wkey)
        traffic = prof["hbm_bytes_per_launch"] if (prof and dom is ig) else None
        step_bytes = (prof["whole_step"]["fetch_bytes"] + prof["whole_step"]["write_bytes"]) if prof else None
        step_s = res["elapsed"] / args.steps
        step_hbm_frac = step_bytes / step_s / PEAK_HBM_BYTES_PER_S if step_bytes else None
        step_mfma_frac = sps / world * gflop_per_sample * 1e9 / 1e12 / peak
        kern_hbm_frac = (traffic / (dom["ms"] / max(dom["calls"], 1) * 1e-3) / PEAK_HBM_BYTES_PER_S) if traffic and dom["ms"] > 0 else None
        kern_mfma_frac = achieved / peak

        def bound_of(mfma, hbm):
            # the resource with the larger share of its peak; "launch" when neither reaches a fifth of its peak: the time then
            # goes to the chain of dependent launches, not to a roofline resource
            if hbm is None:           # no byte-side evidence (no committed PMC profile of these sources): claim the MFMA bound only
                return "mfma" if mfma >= 0.2 else "unknown"      # where the matrix side alone supports it
            if max(mfma, hbm) < 0.2:
                return "launch"
            return "hbm" if hbm > mfma else "mfma"
        if dom is ig:
            dom_name = ("implicit-GEMM family: every mmdyn_igemm_nt* entry-point call of the step (" + kernel_mix(res["by_shape"], dtype) + ")")
        else:
            dom_name = "weight-gradient family: every mmdyn_wgrad_tn* entry-point call of the step"
        rl = {"bound": bound_of(kern_mfma_frac, kern_hbm_frac), "kernel": dom_name,
              "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
              "traffic": traffic, "traffic_provenance": traffic_note, "hbm_frac": kern_hbm_frac,
              "algorithmic_flops_per_launch": dom["flops"] / max(dom["calls"], 1),
              "operand_bytes_per_launch": dom["bytes"] / max(dom["calls"], 1),
              "launches_per_step": dom["calls"], "avg_launch_ms": dom["ms"] / max(dom["calls"], 1),
              "kernel_share_of_step": dom["ms"] / total_ms if total_ms else None,
              "algorithmic_gflop_per_sample": gflop_per_sample,
              "step_algorithmic_tflops": sps / world * gflop_per_sample * 1e9 / 1e12,
              "step_frac_of_peak": step_mfma_frac,
              "step_hbm_bytes": step_bytes, "step_hbm_frac_of_8TBps": step_hbm_frac,
              "step_launches": prof["whole_step"]["launches"] if prof else None,
              "step_bound": bound_of(step_mfma_frac, step_hbm_frac)}
        # what the measured arithmetic adds around the family and is booked under its own name: stand-alone operand splits
        rl["split_planes_ms_per_step"] = kern.get("split_planes", {"ms": 0.0})["ms"]
        rl["bound_note"] = ("label only: `traffic` / `step_hbm_bytes` are the COMMITTED rocprofv3 PMC profile of these kernel sources "
                            "(traffic_provenance; possibly another box), divided by THIS run's event times -- boxes differ by up to 6 %")
        if dtype == "f32x3":
            rl["peak_note"] = ("dense bf16 MFMA peak / 6: every fp32 product is six bf16 products of the exact three-term split "
                               "(MI355X_MICROARCH.md: ~2.5 PF dense at the 2.4 GHz the chip does not hold on random data -- bf16 loops "
                               "measure ~1.25 PF there); launches the split does not serve run on the fp32 matrix cores (peak %.1f)"
                               % PEAK_FP32_MFMA_TFLOPS)
            rl["frac_of_native_fp32_mfma_peak"] = achieved / PEAK_FP32_MFMA_TFLOPS
            rl["step_frac_of_native_fp32_mfma_peak"] = sps / world * gflop_per_sample * 1e9 / 1e12 / PEAK_FP32_MFMA_TFLOPS
        return rl, total_ms

    def kernel_mix(by_shape, dtype):
        """Which kernels served the implicit-GEMM entry-point calls, asked of the library's own launch rules (host-side shape
        queries): a launch the plane-ring kernel serves takes its operands already split (igemm_wsp3_kernel); one with stream-K
        slabs runs the persistent fp32-operand kernel (igemm_wsp_kernel)."""
        from mmdyn_hip import ops as _ops
        lib = getattr(_ops.B, "lib", None)
        n_all = n_p3 = n_wsp = n_patch = 0
        fl_all = fl_p3 = 0.0
        for k, d in by_shape.items():
            if k[0] != "igemm_nt":
                continue
            n_all += d["calls"]
            fl_all += d["flops"]
            ints = [x for x in k[1:] if isinstance(x, int)]
            try:
                mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N = ints[:9]
                if lib is None or ints[13] != 1:
                    continue
                planes_on = dtype == "f32x3" and not args.no_planes and not (N == 32 and args.no_patch_planes)
                if planes_on and lib.mmdyn_igemm_planes_served(mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N) == 1:
                    if N == 32:          # the patch-resident kernel of the 32-channel up-sampling layers, plane form
                        n_patch += d["calls"]
                    else:
                        n_p3 += d["calls"]
                    fl_p3 += d["flops"]
                elif lib.mmdyn_igemm_slab_floats_mx(mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, 128 if dtype == "f32x3" else 0) > 0:
                    n_wsp += d["calls"]
            except Exception:
                pass
        if dtype == "f32x3":
            return (f"{n_all} calls, {n_p3 + n_patch} of them ({100.0 * fl_p3 / max(fl_all, 1.0):.0f} % of the family's flops) convolution-level "
                    f"launches on operands that arrive split, on the persistent plane-ring kernel igemm_wsp3_kernel + its stream-K fix-up "
                    f"launch; {n_wsp} on the persistent fp32-operand kernel igemm_wsp_kernel (split in the MFMA waves); the rest -- FC-level "
                    f"GEMMs -- on igemm_ws_kernel / igemm_nt_kernel.  Booked apart, as in rounds 3-4: the 3-channel layers (conv3.hip) and "
                    f"the 32-channel up-sampling layers (tconv_patch_kernel, in its plane form)")
        return (f"{n_all} calls: {n_wsp} on the persistent stream-K ring kernel igemm_wsp_kernel + its fix-up launch, the rest on "
                f"the one-tile ring kernel igemm_ws_kernel / the register-staged igemm_nt_kernel")

    if pg is not None:
        import torch.distributed as dist
    primary = measure(args.dtype, True, args.full or args.breakdown, args.dump_outputs)
    if pg is not None:
        dist.barrier()
    if rank != 0:
        if pg is not None:
            dist.destroy_process_group()
        return

    elapsed, final_loss = primary["elapsed"], primary["final_loss"]
    global_batch = args.batch * world
    sps = global_batch * args.steps / elapsed
    arith = {"f32": "fp32 (native fp32 matrix cores)",
             "f32x3": "fp32 storage and results, GEMMs in the fp32x3 arithmetic (exact three-term bf16 split of the fp32 operands, "
                      "six of nine products on the bf16 matrix cores, fp32 accumulate; error vs fp64 <= native fp32 MFMA)",
             "bf16": "bf16 matrix-core operands (fp32 accumulate, storage and master weights)",
             "bf16s": "bf16 activation storage + bf16 matrix-core operands (fp32 accumulate and master weights)",
             "fp16": "fp16 matrix-core operands (fp32 accumulate, storage and master weights)",
             "fp16s": "fp16 activation storage + fp16 matrix-core operands (fp32 accumulate and master weights, loss scale 4B)"
             }[args.dtype]
    which = ("BASELINE configs[1]" if (S == 64 and args.dtype in ("f32", "f32x3") and args.problem == "seq_modeling") else
             "per-GPU share of BASELINE configs[2]" if (S == 64 and args.dtype in ("bf16", "bf16s")) else
             "per-GPU share of BASELINE configs[3] (extension: no reference architecture at this size)" if S == 128 else
             "per-GPU share of BASELINE configs[4] (extension: no reference architecture at this size)" if S == 256 else
             "variant")
    workload = (f"cnn-mvae visuotactile+pose {S}x{S}, bs={args.batch} per GPU, {arith}, {args.problem} train step "
                f"(7 subset ELBOs + backward + Adam), {which}")
    out = {
        "metric": "visuotactile samples/sec (train) + ELBO vs CPU ref, cnn-mvae 64x64 bs256 @1/2/4/8 GPU",
        "value": sps, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        # the arithmetic `value` was measured in, at the top level: BENCH_r01..r04 are native-fp32 lines and compare
        # with `native_fp32.value` of this line, BENCH_r05 onwards (f32x3) with `value`
        "arithmetic": arith,
        "compare_with": {"BENCH_r01..r04 (dtype f32)": "native_fp32.value", "BENCH_r05.. (dtype f32x3)": "value"},
        "config": {"workload": workload,
                   "global_batch": global_batch, "parallelism": f"dp{world}", "bn": "sync" if (args.sync_bn and pg is not None) else "local",
                   "launch": "eager" if (args.no_graph or (args.sync_bn and pg is not None and dry)) else "hip_graph",
                   "final_loss": final_loss, "host_enqueue_ms_per_step": 1e3 * primary["host_enqueue"] / args.steps},
    }
    if args.full:
        out["roofline"], _ = roofline_of(primary, sps)
    if rehearse:
        out["rehearsal"] = "all ranks on ONE GPU, collectives over gloo (MMDYN_BENCH_REHEARSE_ONE_GPU=1): schedule check, not a scaling number"
    if dry:
        out["dry_run"] = "CPU rehearsal with emulated kernels (MMDYN_BENCH_DRYRUN=emu): control flow only, numbers meaningless"

    def print_breakdown(res, title):
        k2, tot = res["kern"], sum(d["ms"] for d in res["kern"].values())
        print(f"---- {title} ----", file=sys.stderr)
        for k, d in sorted(k2.items(), key=lambda kv: -kv[1]["ms"]):
            tf = d["flops"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 and d["flops"] else 0.0
            gb = d["bytes"] / (d["ms"] * 1e-3) / 1e9 if d["ms"] > 0 else 0.0
            print(f"{k:24s} calls {d['calls']:4d}  {d['ms']:8.3f} ms  {tf:7.2f} TFLOP/s  {gb:8.1f} GB/s(args)", file=sys.stderr)
        print(f"sum of kernel time {tot:.3f} ms vs step {1e3 * res['elapsed'] / args.steps:.3f} ms", file=sys.stderr)
        print("per-shape MFMA launches: name, (mode,G,Bg,Hi,Wi,Cin,Ho,Wo,N,ldc,stride,offset,act,splitk) | "
              "(mode,Bt,Hr,Wr,Cd,Hi,Wi,Cg,stride,offset,chunks)", file=sys.stderr)
        for k, d in sorted(res["by_shape"].items(), key=lambda kv: -kv[1]["ms"]):
            tf = d["flops"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 else 0.0
            print(f"  {k[0]:9s} {str(k[1:]):70s} x{d['calls']:2d} {d['ms']:7.3f} ms {tf:6.1f} TF/s", file=sys.stderr)

    if args.breakdown:
        print_breakdown(primary, f"{args.dtype} (the measured arithmetic)")
    if args.full and world == 1 and args.dtype in ("f32", "f32x3") and not args.no_alt and not dry and not args.no_graph:
        # The same workload, same seeds, in the OTHER fp32 arithmetic, timed the same way by the same process on the same box and
        # reported NEXT to `value` with its own roofline: native fp32 matrix cores beside the default fp32x3 line (VERDICT r4
        # item 2), or fp32x3 beside an explicit --dtype f32 run.
        other = "f32" if args.dtype == "f32x3" else "f32x3"
        sec = measure(other, False, True)
        sps2 = args.batch * args.steps / sec["elapsed"]
        roof2, _ = roofline_of(sec, sps2)
        obj = {"dtype": other, "value": sps2, "unit": "samples/s", "ms_per_step": 1e3 * sec["elapsed"] / args.steps,
               "final_loss": sec["final_loss"], "roofline": roof2}
        if other == "f32":
            obj["what"] = ("the same workload on the native fp32 matrix cores (v_mfma_f32_16x16x4_f32 / 32x32x2_f32, peak 157.3 TFLOP/s): "
                           "python bench.py --dtype f32 makes it the measured arithmetic")
            out["native_fp32"] = obj
            out["speedup_over_native_fp32"] = sps / sps2
        else:
            obj["name"] = "fp32x3"
            obj["what"] = ("fp32 operands split exactly into three bf16 terms (round-to-nearest), six of the nine cross products on "
                           "the bf16 matrix cores, fp32 accumulate; the default arithmetic of bench.py")
            out["alt_arithmetic"] = obj
        if args.breakdown:
            print_breakdown(sec, other)
    if args.full and world == 1 and not args.no_cpu_baseline:
        # torch.set_num_threads(os.cpu_count()).  On a box whose CPU share is smaller than the
        # machine (the one-GPU box: 16 of 256 hardware threads, no visible quota) the figure at the documented share is
        # reported next to it; `value` / `cores` are the faster of the two, i.e. the strongest CPU baseline measured.
        share, allc = host_cpu_share(), host_cpu_all()
        base = cpu_baseline(args.batch, share, S, 20.0)
        if allc != share:
            full = cpu_baseline(args.batch, allc, S, 12.0)
            best, other = (full, base) if full["value"] > base["value"] else (base, full)
            base = dict(best)
            base["other_thread_count"] = {k: other[k] for k in ("value", "cores", "sample")}
        out["cpu_baseline"] = base
    _emit(out)
    if pg is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
