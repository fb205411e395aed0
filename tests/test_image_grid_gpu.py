"""mmdyn_image_grid_u8 on the device: every case of tests/grid_cases.py through the C ABI against the numpy oracle, with guard bytes
around the output range; the workload's shape on a non-default stream; and --log-images through main() on the fused, graph-replayed
step, the written files against clones of the engine's reconstructions taken when each step ended -- with the epoch's last training
step an eager one, the capturing call, and a real replay."""
import os

import numpy as np
import pytest
import torch

from mmdyn_hip import ops
import grid_cases as G
from test_image_grid_emu import read_png

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(name, logits):
    c = G.case(name)
    srcs = [torch.from_numpy(s).to(DEV) for s in G.sources(name, logits)]
    lo, hi = G.expected(name, logits)

    def launch(out):
        got = ops.B.image_grid(srcs if len(srcs) > 1 else srcs[0], c["take"], c["nrow"], logits, c["padding"], out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.current_stream().synchronize()

    got = G.run_guarded(launch, lo.shape, DEV)
    G.assert_within(got, lo, hi, f"{name} logits={logits}")
    G.check_specials(name, got)
    return srcs, lo, hi


@pytest.mark.parametrize("name,logits", G.RUNS)
def test_kernel_meets_the_oracle(name, logits):
    assert ops.B.name == "hip"
    srcs, lo, hi = _run(name, logits)
    # ... and the allocating form of the wrapper gives the same grid
    c = G.case(name)
    out = ops.B.image_grid(srcs, c["take"], c["nrow"], logits, c["padding"])
    assert out.dtype == torch.uint8 and out.device.type == "cuda" and tuple(out.shape) == lo.shape
    G.assert_within(out.cpu().numpy(), lo, hi, name)


def test_workload_shape_on_a_side_stream():
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run("workload_shape", 1)
    torch.cuda.current_stream().wait_stream(side)


KEYS = ["Input_img/train", "Output_img/train", "Target_img/train", "Input_img/validation", "Output_img/validation",
        "Target_img/validation", "Samples/latent_space"]


def _png(prob, key, epoch=0):
    return read_png(os.path.join(prob.plot_dir, "%s_epoch_%d.png" % (key.replace("/", "_"), epoch)))


# how the epoch's LAST training step runs: the eager exact-last-step path (the issue's command line); the call of
# train_step_graphed that captures (its work is done by an eager warm-up step); a real replay of the captured graphs
@pytest.mark.parametrize("last_step,extra", [("eager", ["--synthetic-batches", "2"]),
                                             ("capture", ["--synthetic-batches", "1", "--exact-running-stats"]),
                                             ("replay", ["--synthetic-batches", "3", "--exact-running-stats"])])
def test_main_writes_the_image_log_of_the_fused_step(tmp_path, monkeypatch, last_step, extra):
    """cnn-mvae with pose on visuotactile input, batches of 4, one epoch, logged, through the CLI on the fused step.  The model's
    recon_x is taken INDEPENDENTLY of the image log: a clone of the engine's `last['recon_x']` right after every training call and
    every validation call, the last of each kept.  The written reconstructions must meet the sigmoid criterion against those clones;
    inputs and targets are exact against the regenerated loader batches."""
    from mmdyn_hip.main import main
    from mmdyn_hip.engine import MVAEStep
    from mmdyn_hip.problems.problems import SyntheticVisuoTactile
    seen = {"replays": 0}

    def cloning(name, split):
        real = getattr(MVAEStep, name)

        def wrapped(self, *a, **k):
            before = seen["replays"]
            out = real(self, *a, **k)
            now = [t.detach().clone() for t in self.last["recon_x"][:2]]
            if name == "train_step_graphed" and seen["replays"] == before:
                # the capturing call: its work was the eager warm-up train_step inside it, whose clone is already kept -- the
                # truth for this step; the engine's `last` must hold the same values now, in the buffers the replays will write
                assert all(torch.equal(a_, b_) for a_, b_ in zip(now, seen[split])), "last after a capturing call"
            else:
                seen[split] = now
            seen[split + "_how"] = (name, seen["replays"] - before)
            return out
        monkeypatch.setattr(MVAEStep, name, wrapped)

    real_replay = MVAEStep._replay
    monkeypatch.setattr(MVAEStep, "_replay", lambda self, c: (seen.__setitem__("replays", seen["replays"] + 1), real_replay(self, c))[1])
    cloning("train_step", "train")
    cloning("train_step_graphed", "train")
    cloning("eval_step", "validation")
    monkeypatch.chdir(tmp_path)
    prob = main(["--problem-type", "seq_modeling", "--model-name", "cnn-mvae", "--input-type", "visuotactile", "--use-pose",
                 "--batchsize", "4", "--num-epochs", "1", "--log-images", "1", "--save-name", "grid"] + extra)
    assert prob._step is not None and prob._step._graph is not None
    assert seen["train_how"] == {"eager": ("train_step", 0), "capture": ("train_step_graphed", 0),
                                 "replay": ("train_step_graphed", 1)}[last_step]
    assert sorted(os.listdir(prob.plot_dir)) == sorted("%s_epoch_0.png" % k.replace("/", "_") for k in KEYS)
    grids = prob.image_grids()
    for key in KEYS:
        assert np.array_equal(_png(prob, key), grids[key].numpy()), key
    take, nrow = 4, 2
    for split in ("train", "validation"):
        recon = [t.cpu().numpy() for t in seen[split]]
        assert all(r.dtype == np.float32 and r.shape == (4, 3, 64, 64) and np.isfinite(r).all() for r in recon)
        lo, hi = G.bounds(recon, take, nrow, 2, 1)
        G.assert_within(_png(prob, "Output_img/" + split), lo, hi, "Output_img/" + split)
    assert not np.array_equal(_png(prob, "Output_img/train"), _png(prob, "Output_img/validation"))
    # after training the engine's `last` names the validation step's tensors: the same check against them, read now
    lo, hi = G.bounds([t.detach().cpu().numpy() for t in prob._step.last["recon_x"][:2]], take, nrow, 2, 1)
    G.assert_within(_png(prob, "Output_img/validation"), lo, hi, "Output_img/validation against last")
    # inputs and targets: the loaders are seeded, a second walk yields their last batches again
    n_train = int(extra[1])
    for split, loader in (("train", SyntheticVisuoTactile(n_train, 4, 1, seed=1234)),
                          ("validation", SyntheticVisuoTactile(max(1, n_train // 4), 4, 1, seed=4321))):
        data, target = list(loader)[-1]
        assert np.array_equal(_png(prob, "Input_img/" + split), G.bounds([data[0].numpy(), data[1].numpy()], take, nrow, 2, 0)[0])
        assert np.array_equal(_png(prob, "Target_img/" + split), G.bounds([target[0].numpy(), target[1].numpy()], take, nrow, 2, 0)[0])
