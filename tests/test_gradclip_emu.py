"""Clipping by the global L2 norm, host side (no GPU): the C ABI's argument checks and host query, FusedAdam / FusedSGD with
``max_norm`` against torch.nn.utils.clip_grad_norm_ + torch.optim, MVAEStep(max_grad_norm) on the emulation, the --grad-clip flag
and its two log entries, and the data-parallel step on gloo.  The kernels are emulated by tests/emu_backend_gradclip.py."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mmdyn_hip import _lib, ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.problems.problems import FusedAdam, FusedSGD, SeqModeling, SyntheticVisuoTactile
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise
from emu_backend_gradclip import EmuBackendGradClip, clip_factor
import test_model_emu as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(autouse=True)
def emu():
    old = ops.set_backend(EmuBackendGradClip())
    yield
    ops.set_backend(old)


def rnd(n, seed):
    g = torch.Generator().manual_seed(seed + n)
    return torch.rand(n, generator=g) * 2 - 1


# ---- C ABI --------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_argument_errors_and_block_query():
    lib = _lib.load()
    for name in ("mmdyn_grad_sumsq_blocks", "mmdyn_grad_sumsq", "mmdyn_grad_clip_coef", "mmdyn_adam_step_clipped",
                 "mmdyn_sgd_step_clipped"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES
    assert lib.mmdyn_abi_version() == 6
    one = 64                # (any non-null address: the checks below return before a launch)
    assert lib.mmdyn_grad_sumsq(None, 4, one, one, 0, None) == -2
    assert lib.mmdyn_grad_sumsq(one, 4, None, one, 0, None) == -2
    assert lib.mmdyn_grad_sumsq(one, 4, one, None, 0, None) == -2
    assert lib.mmdyn_grad_clip_coef(None, 1.0, 1.0, None) == -2
    assert lib.mmdyn_adam_step_clipped(one, one, one, one, one, None, 4, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0, None) == -2
    assert lib.mmdyn_adam_step_clipped(None, one, one, one, one, one, 4, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0, None) == -2
    assert lib.mmdyn_sgd_step_clipped(one, one, one, None, 4, 1e-3, 0.9, 5e-4, 1.0, 1, None) == -2
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        assert lib.mmdyn_grad_clip_coef(one, 1.0, bad, None) == -1, bad
    sizes = (0, 1, 4, 100003, 2 ** 21 + 5)
    blocks = [lib.mmdyn_grad_sumsq_blocks(n) for n in sizes]
    assert all(b >= 1 for b in blocks) and blocks == sorted(blocks), blocks
    assert blocks[-1] > blocks[0]                                       # (more than one block at the large sizes)


def test_wrappers_reject_bad_arguments_before_any_launch():
    """HipBackend's own checks (no library call is reached: the tensors are CPU tensors and the first thing a launch would do with
    them is refuse them)."""
    hip = ops.HipBackend()
    g, ws = torch.zeros(8), torch.zeros(1, dtype=torch.float64)
    for clip in (torch.zeros(3, dtype=torch.float64), torch.zeros(4), torch.zeros(5, dtype=torch.float64), None):
        with pytest.raises(ValueError):
            hip.grad_sumsq(g, ws, clip)
        with pytest.raises(ValueError):
            hip.grad_clip_coef(clip, 1.0, 1.0)
        with pytest.raises(ValueError):
            hip.adam_step_clipped(g, g, g, g, torch.zeros(3, dtype=torch.float64), clip, 1e-3, 0.9, 0.999, 1e-8, 1.0)
        with pytest.raises(ValueError):
            hip.sgd_step_clipped(g, g, g, clip, 1e-3, 0.9, 5e-4, 1.0, True)
    clip = torch.zeros(4, dtype=torch.float64)
    for bad in (0, 0.0, -1.0, float("nan"), None, "1", True, 1j):
        with pytest.raises(ValueError):
            hip.grad_clip_coef(clip, 1.0, bad)
    with pytest.raises(ValueError):                                     # a guarded step with a three-double state
        hip.adam_step_clipped(g, g, g, g, torch.zeros(3, dtype=torch.float64), clip, 1e-3, 0.9, 0.999, 1e-8, 1.0, guarded=True)
    with pytest.raises(ValueError):                                     # a workspace smaller than the host query asks for
        hip.grad_sumsq(torch.zeros(100003), torch.zeros(3, dtype=torch.float64), clip)


# ---- module-path optimisers ------------------------------------------------------------------------------------------------------
SIZES = (1, 7, 100003)


def _grads(step):
    return [rnd(n, 50 + i) * 0.01 * (step + 1) for i, n in enumerate(SIZES)]


def _norm64(gs):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))


@pytest.mark.parametrize("which", ["adam", "sgd"])
@pytest.mark.parametrize("clips", [True, False])
def test_fused_optimisers_clip_like_torch(which, clips):
    """Three tensors of 1, 7 and 100003 elements, three steps, against clip_grad_norm_ + torch.optim on the CPU.  max_norm comes
    from the data: half the smallest step norm (every step clips) or twice the largest (none does)."""
    norms = [_norm64(_grads(s)) for s in range(3)]
    max_norm = float(np.float32(0.5 * min(norms) if clips else 2.0 * max(norms)))
    for nm in norms:                                                    # the reference itself clips / does not clip
        coef = max_norm / (nm + 1e-6)
        assert coef < 1.0 if clips else min(1.0, coef) == 1.0
    p0 = [rnd(n, 60 + i) for i, n in enumerate(SIZES)]
    ours = [torch.nn.Parameter(p.clone()) for p in p0]
    ref = [torch.nn.Parameter(p.clone()) for p in p0]
    if which == "adam":
        opt, ropt = FusedAdam(ours, lr=1e-3, max_norm=max_norm), torch.optim.Adam(ref, lr=1e-3)
    else:
        opt = FusedSGD(ours, lr=1e-3, momentum=0.9, weight_decay=5e-4, max_norm=max_norm)
        ropt = torch.optim.SGD(ref, lr=1e-3, momentum=0.9, weight_decay=5e-4)
    assert opt.grad_norm is None and opt.clipped_steps == 0
    for s in range(3):
        for p, r, g in zip(ours, ref, _grads(s)):
            p.grad, r.grad = g.clone(), g.clone()
        opt.step()
        torch.nn.utils.clip_grad_norm_(ref, max_norm)
        ropt.step()
        assert opt.grad_norm == pytest.approx(norms[s], rel=1e-12)
        assert opt.clipped_steps == (s + 1 if clips else 0)
    for p, r in zip(ours, ref):
        torch.testing.assert_close(p.detach(), r.detach(), rtol=1e-6, atol=1e-7)


def test_fused_optimisers_without_max_norm_are_the_unclipped_path():
    """max_norm=None never touches the clipping ops (a backend without them serves it); a bad max_norm is a ValueError."""
    from emu_backend import EmuBackend
    old = ops.set_backend(EmuBackend())
    try:
        for cls in (FusedAdam, FusedSGD):
            p = torch.nn.Parameter(rnd(7, 1))
            opt = cls([p], lr=1e-3)
            p.grad = rnd(7, 2)
            opt.step()
            assert opt.max_norm is None and opt.grad_norm is None and opt.clipped_steps == 0
    finally:
        ops.set_backend(old)
    for cls in (FusedAdam, FusedSGD):
        for bad in (0.0, -2.0, float("nan"), "x"):
            with pytest.raises(ValueError):
                cls([torch.nn.Parameter(rnd(7, 1))], max_norm=bad)


# ---- fused engine ----------------------------------------------------------------------------------------------------------------
def _engine(use_pose, B, **kw):
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass, n_mask, 4321)
    return MVAEStep(T.build("cnn-mvae", True, use_pose, "cpu"), noise=InjectedNoise(eps, masks), precision="fp32", **kw)


@pytest.mark.parametrize("use_pose", [True, False])
def test_engine_reports_and_clips_the_global_norm(use_pose):
    """B = 4 (the golden batch of the engine tests).  inf: the norm is reported and the step is max_grad_norm=None's bit for bit.
    Half the norm: the step equals the unclipped adam_step given grad_scale = f, with f built from the reported coefficient."""
    B = 4
    inputs, targets = seeded_batch(B, 1234, with_pose=use_pose)
    plain, report = _engine(use_pose, B), _engine(use_pose, B, max_grad_norm=float("inf"))
    assert plain.max_grad_norm is None and plain.grad_norm is None and plain.clipped_steps == 0
    for e in (plain, report):
        e.forward(inputs, targets, 0.02, train=True)
        e.optimizer_step(e.backward())
    assert torch.equal(plain.params.grad, report.params.grad)
    want = math.sqrt(float((report.params.grad.double() ** 2).sum())) / (report.world * report.loss_scale)
    assert report.grad_norm == pytest.approx(want, rel=1e-12) and want > 0
    assert report.clipped_steps == 0 and float(report.clip[2]) == 1.0
    for a, b in ((plain.params.flat, report.params.flat), (plain.adam_m, report.adam_m), (plain.adam_v, report.adam_v),
                 (plain.adam_state, report.adam_state)):
        assert torch.equal(a, b)

    clipped = _engine(use_pose, B, max_grad_norm=0.5 * want)
    clipped.forward(inputs, targets, 0.02, train=True)
    handles = clipped.backward()
    assert torch.equal(clipped.params.grad, report.params.grad)
    twin = [t.clone() for t in (clipped.params.flat, clipped.adam_m, clipped.adam_v, clipped.adam_state)]
    clipped.optimizer_step(handles)
    assert clipped.grad_norm == pytest.approx(want, rel=1e-12) and clipped.clipped_steps == 1
    coef = float(clipped.clip[2])
    assert coef == pytest.approx(float(np.float32(0.5 * want)) / (want + 1e-6), rel=1e-12) and coef < 1.0
    f = clip_factor(1.0 / (clipped.world * clipped.loss_scale), coef)
    ops.B.adam_step(twin[0], clipped.params.grad, twin[1], twin[2], twin[3], clipped.lr, clipped.betas[0], clipped.betas[1],
                    clipped.eps, f)
    for a, b in zip(twin, (clipped.params.flat, clipped.adam_m, clipped.adam_v, clipped.adam_state)):
        assert torch.equal(a, b)
    assert not torch.equal(clipped.params.flat, plain.params.flat)


def test_engine_rejects_bad_max_grad_norm():
    m = T.build("cnn-mvae", True, True, "cpu")
    for bad in (0, 0.0, -1.0, float("nan"), "0.5", True):
        with pytest.raises(ValueError):
            MVAEStep(m, max_grad_norm=bad)


# ---- problem layer and command line --------------------------------------------------------------------------------------------
def test_grad_clip_flag_reaches_the_fused_step_and_the_optimiser(tmp_path):
    from mmdyn_hip.main import build_parser, main
    base = ["--problem-type", "seq_modeling", "--model-name", "cnn-mvae", "--input-type", "visuotactile", "--use-pose", "--no-cuda"]
    assert build_parser().parse_args(base + ["--grad-clip", "0.5"]).grad_clip == 0.5
    assert build_parser().parse_args(base + ["--grad-clip", "inf"]).grad_clip == float("inf")
    assert build_parser().parse_args(base).grad_clip == 0
    prob = SeqModeling(T.args(no_cuda=True, grad_clip=0.5), log_dir=str(tmp_path))
    assert prob._step is not None and prob._step.max_grad_norm == 0.5 and prob._optimizer.max_norm == 0.5
    for over in (dict(), dict(grad_clip=0.0)):
        prob = SeqModeling(T.args(no_cuda=True, **over), log_dir=str(tmp_path))
        assert prob._step.max_grad_norm is None and prob._optimizer.max_norm is None and prob._step.clip is None
    prob = SeqModeling(T.args(no_cuda=True, grad_clip=0.5, optimizer="SGD", model_name="cnn-vae", input_type="visual"),
                       log_dir=str(tmp_path))
    assert isinstance(prob._optimizer, FusedSGD) and prob._optimizer.max_norm == 0.5
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="--grad-clip"):
            SeqModeling(T.args(no_cuda=True, grad_clip=bad), log_dir=str(tmp_path))
    for bad in ("-1", "nan"):
        with pytest.raises(SystemExit):
            main(base + ["--grad-clip", bad, "--synthetic-batches", "1"])


@pytest.mark.parametrize("fused", [True, False])
def test_grad_clip_log_entries_after_one_synthetic_epoch(tmp_path, fused):
    """One epoch of two steps, fused engine and module path.  1e-3 is far below the norm of this loss's gradient (12 288 BCE terms
    per image, the pose term times 1000): both steps clip."""
    over = {} if fused else dict(model_name="cnn-vae", input_type="visual")
    prob = SeqModeling(T.args(no_cuda=True, grad_clip=1e-3, batchsize=2, **over), log_dir=str(tmp_path), fused=True,
                       train_loader=SyntheticVisuoTactile(2, 2))
    assert (prob._step is not None) == fused
    prob._anneal_KL(0)
    prob._train_epoch(0)
    norms, clipped = prob._logger_dict["Grad_norm/train_epoch"], prob._logger_dict["Grad_clipped/train_epoch"]
    assert len(norms) == 1 and math.isfinite(norms[0]) and norms[0] > 1e-3
    assert clipped == [2]
    prob._train_epoch(1)                                                # the count is per epoch, not cumulative
    assert prob._logger_dict["Grad_clipped/train_epoch"] == [2, 2]
    plain = SeqModeling(T.args(no_cuda=True, batchsize=2, **over), log_dir=str(tmp_path), train_loader=SyntheticVisuoTactile(1, 2))
    plain._anneal_KL(0)
    plain._train_epoch(0)
    assert "Grad_norm/train_epoch" not in plain._logger_dict and "Grad_clipped/train_epoch" not in plain._logger_dict


# ---- data parallel (gloo, world size 2, emulation) -----------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, max_grad_norm):
    for p in (ROOT, os.path.join(ROOT, "multimodal-dynamics_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ops.set_backend(EmuBackendGradClip())
    B = 2
    inputs, targets = seeded_batch(B * world, 1234)
    sl = slice(rank * B, (rank + 1) * B)
    eps, masks = seeded_noise(B, 256, 7, 8, 100 + rank)
    step = MVAEStep(T.build("cnn-mvae", True, True, "cpu"), noise=InjectedNoise(eps, masks), process_group=dist.group.WORLD,
                    world_size=world, precision="fp32", max_grad_norm=max_grad_norm)
    step.train_step([x[sl] for x in inputs], [x[sl] for x in targets], 0.02)
    torch.save({"flat": step.params.flat.clone(), "offsets": step.params.offsets, "clip": step.clip.clone(),
                "grad": step.params.grad.clone()}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_clipped_step_matches_averaged_clipped_gradients(tmp_path):
    """Both ranks report the same norm bits and end with equal parameters, which are those of "average the shard gradients, clip
    by the global norm, one Adam step" (the oracle's gradients, torch's clip_grad_norm_, the oracle's Adam) to the tolerance of
    tests/test_ddp_gloo.py.  max_grad_norm is half the norm of the oracle's averaged gradient."""
    from oracle import mvae_oracle as O
    from mmdyn_hip.models.shapes import state_dict_shapes
    from mmdyn_hip.utils.seeded_init import seeded_state_dict
    world = 2
    sd = seeded_state_dict(state_dict_shapes("cnn-mvae", use_pose=True), 0)
    inputs, targets = seeded_batch(4, 1234)
    grads = []
    for rank in range(world):
        prm, buf = O.split_state(sd)
        sl = slice(rank * 2, (rank + 1) * 2)
        eps, masks = seeded_noise(2, 256, 7, 8, 100 + rank)
        _, loss, _ = O.evaluate_mvae(prm, [x[sl] for x in inputs], [x[sl] for x in targets], eps, masks, 0.02, 1000.0, True, buf)
        loss.backward()
        grads.append({k: v.grad for k, v in prm.items()})
    prm, _ = O.split_state(sd)
    names = list(prm)
    for k in names:
        prm[k].grad = 0.5 * (grads[0][k] + grads[1][k])
    norm = _norm64([prm[k].grad for k in names])
    max_norm = float(np.float32(0.5 * norm))
    assert max_norm / (norm + 1e-6) < 1.0

    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path), max_norm), nprocs=world, join=True, start_method="spawn")
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=False)
    assert torch.equal(r0["clip"].view(torch.int64), r1["clip"].view(torch.int64))      # the same norm BITS on both ranks
    torch.testing.assert_close(r0["flat"], r1["flat"], rtol=0, atol=0)
    # the reported norm is that of the AVERAGED gradient (the buffer holds the sum over ranks)
    assert float(r0["clip"][1]) == pytest.approx(0.5 * math.sqrt(float((r0["grad"].double() ** 2).sum())), rel=1e-12)
    assert float(r0["clip"][1]) == pytest.approx(norm, rel=1e-3) and float(r0["clip"][3]) == 1.0

    torch.nn.utils.clip_grad_norm_([prm[k] for k in names], max_norm)
    O.Adam([prm[k] for k in names], lr=1e-3).step()
    for k in names:
        o = r0["offsets"][k]
        got = r0["flat"][o:o + prm[k].numel()].view_as(prm[k])
        err = (got - prm[k].detach()).abs()
        assert float((err > 1e-5).float().mean()) < 0.02, (k, float(err.max()))
        assert float(err.max()) <= 2.1e-3, k
