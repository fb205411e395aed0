"""The epoch image log, host side (no GPU): the C ABI's argument checks through the real library, the wrapper's checks, the grid
arithmetic, and --log-images through the problems on the emulation -- the files written, their contents against the oracle of
tests/grid_cases.py, the reference's nrow / take rule, the epochs that are logged, and that nothing happens with the flag off."""
import math
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from mmdyn_hip import _lib, ops
from mmdyn_hip.problems.problems import Reconstruction, Regression, SeqModeling, DynModeling, SyntheticVisuoTactile
from emu_backend_grid import EmuBackendGrid
import grid_cases as G
import test_model_emu as T


@pytest.fixture(autouse=True)
def emu():
    backend = EmuBackendGrid()
    old = ops.set_backend(backend)
    yield backend
    ops.set_backend(old)


def read_png(path):
    """The uint8 [H][W][3] pixels of an 8-bit RGB, non-interlaced PNG whose scanlines all use filter type 0 (zlib + struct)."""
    b = open(path, "rb").read()
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr, tags = 8, b"", None, []
    while pos < len(b):
        n, tag = struct.unpack(">I4s", b[pos:pos + 8])
        data = b[pos + 8:pos + 8 + n]
        assert zlib.crc32(tag + data) & 0xFFFFFFFF == struct.unpack(">I", b[pos + 8 + n:pos + 12 + n])[0], tag
        tags.append(tag)
        hdr = struct.unpack(">IIBBBBB", data) if tag == b"IHDR" else hdr
        idat += data if tag == b"IDAT" else b""
        pos += 12 + n
    assert tags[0] == b"IHDR" and tags[-1] == b"IEND" and hdr[2:] == (8, 2, 0, 0, 0), (tags, hdr)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(hdr[1], 1 + 3 * hdr[0])
    assert not raw[:, 0].any(), "a scanline with a filter type other than 0"
    return raw[:, 1:].reshape(hdr[1], hdr[0], 3)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_symbol_and_argument_errors():
    lib = _lib.load()
    assert hasattr(lib, "mmdyn_image_grid_u8") and "mmdyn_image_grid_u8" in _lib._SIGNATURES and "mmdyn_image_grid_u8" in _lib.EXPORTS
    assert lib.mmdyn_abi_version() == 6
    a, b, o = 4096, 8192, 12288    # (any non-null, aligned addresses: every check below returns before a launch)
    NULL, SHAPE, RANGE = -2, -1, -3
    #           n0 n1 take C  H  W nrow padding logits
    good = dict(n0=4, n1=0, take=4, C=3, H=8, W=8, nrow=2, padding=2, logits=0)

    def call(src0=a, src1=None, out=o, **over):
        k = dict(good, **over)
        return lib.mmdyn_image_grid_u8(src0, src1, out, k["n0"], k["n1"], k["take"], k["C"], k["H"], k["W"], k["nrow"], k["padding"],
                                       k["logits"], None)

    assert call(src0=None) == NULL and call(out=None) == NULL
    assert call(src1=b, n1=0) == SHAPE and call(src1=b, n1=-1) == SHAPE and call(src1=None, n1=2) == SHAPE
    for over in (dict(C=2), dict(C=0), dict(C=4), dict(H=0), dict(W=0), dict(take=0), dict(nrow=0), dict(padding=-1), dict(n0=0),
                 dict(H=-3), dict(n0=-1)):
        assert call(**over) == SHAPE, over
    assert call(out=o + 2) == SHAPE and call(src0=a + 1) == SHAPE and call(src1=b + 2, n1=2) == SHAPE
    # the output: 2^15 x 2^15 x 3 = 3 * 2^30 bytes; one below in each direction is inside the range (the check alone: no such call
    # is made here -- it would launch)
    assert call(n0=1, take=1, H=1 << 15, W=1 << 15) == RANGE                       # (N = 1: Hg * Wg * 3 = 3 * 2^30; src 3 * 2^30 too)
    assert call(n0=1 << 20, take=1 << 20, nrow=1 << 20, H=30, W=30, C=1) == RANGE  # (src 2^20 * 900 < 2^31; Hg * Wg * 3 = 32 * 2^20 * 32 * 3 + ...)
    assert call(n0=1 << 20, take=1, H=64, W=64) == RANGE                           # (src0: 2^20 * 12288 elements; the grid is one image)
    assert call(src1=b, n1=1 << 20, take=1, H=64, W=64) == RANGE                   # (src1 likewise)
    assert call(H=(1 << 31) - 1, W=(1 << 31) - 1, n0=(1 << 31) - 1, take=(1 << 31) - 1, padding=(1 << 31) - 1) == RANGE    # (no overflow on the way)


# ---- wrapper ---------------------------------------------------------------------------------------------------------------------------
def test_wrapper_rejects_bad_arguments_before_any_launch():
    hip = ops.HipBackend()           # (CPU tensors: a call that got past the checks would raise RuntimeError at the first pointer)
    x = torch.zeros(4, 3, 8, 8)
    bad_sources = [x.double(), x.half(), x[:, :, ::2], x[0], x.reshape(4, 3, 64), torch.zeros(4, 2, 8, 8), torch.zeros(0, 3, 8, 8),
                   [x, torch.zeros(4, 1, 8, 8)], [x, torch.zeros(4, 3, 8, 9)], [x, x, x], [], None, "x", [x, None]]
    for srcs in bad_sources:
        with pytest.raises(ValueError, match="mmdyn_image_grid_u8"):
            hip.image_grid(srcs, 4, 2, False)
    for kw in (dict(take=0), dict(take=-1), dict(nrow=0), dict(padding=-1), dict(take=1.5), dict(nrow=True)):
        k = dict(dict(take=4, nrow=2, padding=2), **kw)
        with pytest.raises(ValueError, match="mmdyn_image_grid_u8"):
            hip.image_grid(x, k["take"], k["nrow"], False, padding=k["padding"])
    for out in (torch.zeros(22, 22, 3), torch.zeros(22, 22, 3, dtype=torch.uint8)[:, ::2], torch.zeros(22, 21, 3, dtype=torch.uint8),
                torch.zeros(3, 22, 22, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out must be"):
            hip.image_grid(x, 4, 2, False, out=out)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # well-formed arguments do reach the pointer checks
        hip.image_grid(x, 4, 2, False)


def test_grid_shape_agrees_with_the_oracle():
    for c in G.CASES:
        N = min(c["n0"], c["take"]) + min(c["n1"], c["take"])
        want = G.grid_shape(N, c["H"], c["W"], c["nrow"], c["padding"])
        assert ops.grid_shape(N, c["H"], c["W"], c["nrow"], c["padding"]) == want, c["name"]
        for lg in c["logits"]:
            assert G.expected(c["name"], lg)[0].shape == want + (3,)
    assert ops.grid_shape(240, 64, 64, 16) == (15 * 66 + 2, 16 * 66 + 2) and ops.grid_shape(1, 7, 9, 4) == (7, 9)
    assert ops.grid_shape(5, 3, 5, 2) == (17, 16) and ops.grid_shape(3, 3, 3, 3, padding=1) == (5, 13)
    for bad in ((0, 4, 4, 2, 2), (4, 0, 4, 2, 2), (4, 4, 4, 0, 2), (4, 4, 4, 2, -1)):
        with pytest.raises(ValueError):
            ops.grid_shape(*bad)


@pytest.mark.parametrize("name,logits", G.RUNS)
def test_emulation_meets_the_oracle(emu, name, logits):
    """The numpy restatement the problem-level tests below run on is held to the same cases, guard bytes included."""
    c = G.case(name)
    srcs = [torch.from_numpy(s) for s in G.sources(name, logits)]
    lo, hi = G.expected(name, logits)
    got = G.run_guarded(lambda out: emu.image_grid(srcs, c["take"], c["nrow"], logits, c["padding"], out=out), lo.shape, "cpu")
    G.assert_within(got, lo, hi, name)
    G.check_specials(name, got)


# ---- problems ------------------------------------------------------------------------------------------------------------------------
SEQ_KEYS = ["Input_img/train", "Output_img/train", "Target_img/train", "Input_img/validation", "Output_img/validation",
            "Target_img/validation", "Samples/latent_space"]


def _files(keys, epochs):
    return sorted("%s_epoch_%d.png" % (k.replace("/", "_"), e) for k in keys for e in epochs)


def _last_batch(loader):
    """The loader is seeded: a second walk yields the same batches."""
    return list(SyntheticVisuoTactile(loader.n_batches, loader.batchsize, loader.seq_length, seed=loader.seed, size=loader.size))[-1]


@pytest.mark.parametrize("use_pose", [True, False])
@pytest.mark.parametrize("seq_length", [1, 2])
def test_seq_modeling_writes_the_reference_image_log(tmp_path, emu, seq_length, use_pose):
    bs, l = 4, seq_length
    train, test = SyntheticVisuoTactile(2, bs, l), SyntheticVisuoTactile(1, bs, l, seed=7)
    prob = SeqModeling(T.args(no_cuda=True, batchsize=bs, num_epochs=2, log_images=1, use_pose=use_pose), log_dir=str(tmp_path),
                       seq_length=l, train_loader=train, test_loader=test)
    assert prob._step is not None and prob.plot_dir == str(tmp_path) + "/plot/" and prob.image_grids() == {}
    prob.train()
    assert sorted(os.listdir(prob.plot_dir)) == _files(SEQ_KEYS, (0, 1))
    grids = prob.image_grids()
    assert sorted(grids) == sorted(SEQ_KEYS)
    for key, g in grids.items():
        assert g.dtype == torch.uint8 and g.device.type == "cpu" and g.dim() == 3 and g.shape[2] == 3
        path = os.path.join(prob.plot_dir, "%s_epoch_1.png" % key.replace("/", "_"))
        assert np.array_equal(read_png(path), g.numpy()), key
    # the reference's rule (problems.py:589-593) for both sequence lengths, on every launch of both epochs
    nrow, take = (l, min(bs * l, 120)) if l > 1 else (int(math.sqrt(bs)), min(bs * l, 120))
    assert len(emu.grid_calls) == 14
    for call in emu.grid_calls:
        assert (call["nrow"], call["take"], call["padding"]) == (nrow, take, 2)
    calls = dict(zip(SEQ_KEYS, emu.grid_calls[7:]))          # (epoch 1, in the order the keys were kept)
    for key in SEQ_KEYS:
        assert calls[key]["logits"] == (key.startswith("Output") or key.startswith("Samples")), key
        assert len(calls[key]["srcs"]) == 2 and all(s.shape[1:] == (3, 64, 64) for s in calls[key]["srcs"]), key
        assert calls[key]["srcs"][0].shape[0] == (50 if key.startswith("Samples") else bs)
        N = 2 * min(calls[key]["srcs"][0].shape[0], take)
        assert tuple(grids[key].shape) == G.grid_shape(N, 64, 64, nrow, 2) + (3,), key
    # the inputs and targets are the last training batch's, exactly
    data, target = _last_batch(train)
    lo, hi = G.bounds([data[0][::l].numpy(), data[1][::l].numpy()], take, nrow, 2, 0)
    assert np.array_equal(grids["Input_img/train"].numpy(), lo)
    lo, hi = G.bounds([target[0][::l].numpy(), target[1][::l].numpy()], take, nrow, 2, 0)
    assert np.array_equal(grids["Target_img/train"].numpy(), lo)
    data, target = _last_batch(test)
    lo, hi = G.bounds([data[0][::l].numpy(), data[1][::l].numpy()], take, nrow, 2, 0)
    assert np.array_equal(grids["Input_img/validation"].numpy(), lo)
    # the reconstructions: the sigmoid criterion against the model's recon_x -- the engine's `last` still names the validation
    # step's after training; the training step's are the tensors the launch was handed (the pose logits left out)
    recon = [t.detach().numpy() for t in prob._step.last["recon_x"][:2]]
    for got, want in zip(calls["Output_img/validation"]["srcs"], recon):
        assert np.array_equal(got, want)
    for key in ("Output_img/train", "Output_img/validation", "Samples/latent_space"):
        lo, hi = G.bounds(calls[key]["srcs"], take, nrow, 2, 1)
        G.assert_within(grids[key].numpy(), lo, hi, key)
    assert not np.array_equal(calls["Output_img/train"]["srcs"][0], calls["Output_img/validation"]["srcs"][0])


def test_pillow_reads_the_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    prob = SeqModeling(T.args(no_cuda=True, batchsize=4, num_epochs=1, log_images=1), log_dir=str(tmp_path),
                       train_loader=SyntheticVisuoTactile(1, 4), test_loader=SyntheticVisuoTactile(1, 4, seed=7))
    prob.train()
    for key, g in prob.image_grids().items():
        with Image.open(os.path.join(prob.plot_dir, "%s_epoch_0.png" % key.replace("/", "_"))) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), g.numpy()), key


def test_logged_epochs_are_the_multiples_and_the_last(tmp_path, emu):
    prob = SeqModeling(T.args(no_cuda=True, batchsize=4, num_epochs=3, log_images=2), log_dir=str(tmp_path),
                       train_loader=SyntheticVisuoTactile(1, 4), test_loader=SyntheticVisuoTactile(1, 4, seed=7))
    prob.train()
    assert sorted(os.listdir(prob.plot_dir)) == _files(SEQ_KEYS, (0, 2))       # epoch 2: a multiple of 2 and the last, written once
    assert len(emu.grid_calls) == 14
    prob = SeqModeling(T.args(no_cuda=True, batchsize=4, num_epochs=2, log_images=5), log_dir=str(tmp_path / "b"),
                       train_loader=SyntheticVisuoTactile(1, 4), test_loader=SyntheticVisuoTactile(1, 4, seed=7))
    prob.train()
    assert sorted(os.listdir(prob.plot_dir)) == _files(SEQ_KEYS, (0, 1))       # epoch 1: the last one


def test_dyn_modeling_takes_whole_sequences(tmp_path, emu):
    bs, l = 2, 3
    prob = DynModeling(T.args(problem_type="dyn_modeling", no_cuda=True, batchsize=bs, num_epochs=1, log_images=1), log_dir=str(tmp_path),
                       seq_length=l, train_loader=SyntheticVisuoTactile(1, bs, l), test_loader=SyntheticVisuoTactile(1, bs, l, seed=7))
    prob.train()
    assert sorted(os.listdir(prob.plot_dir)) == _files(SEQ_KEYS, (0,))
    for call in emu.grid_calls:
        assert (call["nrow"], call["take"]) == (l, bs * l)
    assert tuple(prob.image_grids()["Input_img/train"].shape) == G.grid_shape(2 * bs * l, 64, 64, l, 2) + (3,)


@pytest.mark.parametrize("model_name", ["cnn-vae", "mlp-vae"])
def test_single_modality_models(tmp_path, emu, model_name):
    """cnn-vae: the single-tensor branch; mlp-vae: every tensor viewed as (-1, 3, H, W) first (problems.py:595-596)."""
    bs = 4
    S = 28 if model_name == "mlp-vae" else 64                  # (the MLP stack is the reference's 784-pixel one)
    train = SyntheticVisuoTactile(1, bs, size=S)
    prob = Reconstruction(T.args(problem_type="reconstruction", model_name=model_name, input_type="visual", use_pose=False,
                                 no_cuda=True, batchsize=bs, num_epochs=1, log_images=1, image_size=S), log_dir=str(tmp_path),
                          train_loader=train, test_loader=SyntheticVisuoTactile(1, bs, seed=7, size=S))
    prob.train()
    keys = [k for k in SEQ_KEYS if not k.startswith("Target")]
    assert sorted(os.listdir(prob.plot_dir)) == _files(keys, (0,))
    nrow, take = 2, bs                                          # reconstruction: int(sqrt(batchsize)), min(batchsize, 120)
    calls = dict(zip(keys, emu.grid_calls))
    for key, call in calls.items():
        # (mlp-vae: the 50 draws are 50 rows of S * S values, which the (-1, 3, S, S) view does not divide -- one-channel images)
        C = 1 if (model_name == "mlp-vae" and key.startswith("Samples")) else 3
        assert (call["nrow"], call["take"]) == (nrow, take) and len(call["srcs"]) == 1 and call["srcs"][0].shape[1:] == (C, S, S), key
    assert calls["Samples/latent_space"]["srcs"][0].shape[0] == 50 and calls["Input_img/train"]["srcs"][0].shape[0] == bs
    grids = prob.image_grids()
    lo, hi = G.bounds([_last_batch(train)[0][0].numpy()], take, nrow, 2, 0)
    assert np.array_equal(grids["Input_img/train"].numpy(), lo)
    calls = dict(zip(keys, emu.grid_calls))
    for key in ("Output_img/train", "Output_img/validation", "Samples/latent_space"):
        lo, hi = G.bounds(calls[key]["srcs"], take, nrow, 2, 1)
        G.assert_within(grids[key].numpy(), lo, hi, key)
        assert np.array_equal(read_png(os.path.join(prob.plot_dir, "%s_epoch_0.png" % key.replace("/", "_"))), grids[key].numpy())
    assert tuple(grids["Samples/latent_space"].shape) == G.grid_shape(min(50, take), S, S, nrow, 2) + (3,)


def test_regression_writes_nothing(tmp_path, emu):
    prob = Regression(T.args(problem_type="regression", model_name="regressor", input_type="visual", use_pose=False, no_cuda=True,
                             batchsize=4, num_epochs=1, log_images=1), log_dir=str(tmp_path),
                      train_loader=SyntheticVisuoTactile(1, 4), test_loader=SyntheticVisuoTactile(1, 4, seed=7))
    prob.train()
    assert emu.grid_calls == [] and prob.image_grids() == {}
    assert not os.path.exists(prob.plot_dir) or os.listdir(prob.plot_dir) == []


@pytest.mark.parametrize("over", [dict(), dict(log_images=0)])
def test_off_by_default(tmp_path, emu, over, monkeypatch):
    calls = []
    real = SeqModeling._sample
    monkeypatch.setattr(SeqModeling, "_sample", lambda self, n=50: calls.append(n) or real(self, n))
    prob = SeqModeling(T.args(no_cuda=True, batchsize=4, num_epochs=2, **over), log_dir=str(tmp_path),
                       train_loader=SyntheticVisuoTactile(1, 4), test_loader=SyntheticVisuoTactile(1, 4, seed=7))
    prob.train()
    assert calls == [] and emu.grid_calls == [] and prob.image_grids() == {}
    assert not os.path.exists(os.path.join(str(tmp_path), "plot")) and prob.plot_dir == str(tmp_path) + "/plot/"
    # ... and with the flag on the counter does count: once per logged epoch
    prob = SeqModeling(T.args(no_cuda=True, batchsize=4, num_epochs=2, log_images=1), log_dir=str(tmp_path / "on"),
                       train_loader=SyntheticVisuoTactile(1, 4), test_loader=SyntheticVisuoTactile(1, 4, seed=7))
    prob.train()
    assert calls == [50, 50]
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="--log-images"):
            SeqModeling(T.args(no_cuda=True, log_images=bad), log_dir=str(tmp_path / "bad"))


def test_backend_without_the_op_is_an_error(tmp_path):
    """An emulation written before the op: the logged epoch names the missing op, nothing falls back to torch ops."""
    from emu_backend_ema import EmuBackendEma
    old = ops.set_backend(EmuBackendEma())
    try:
        prob = SeqModeling(T.args(no_cuda=True, batchsize=4, num_epochs=1, log_images=1), log_dir=str(tmp_path),
                           train_loader=SyntheticVisuoTactile(1, 4))
        with pytest.raises(RuntimeError, match="image_grid"):
            prob.train()
    finally:
        ops.set_backend(old)


# ---- command line -----------------------------------------------------------------------------------------------------------------------
def test_log_images_flag():
    from mmdyn_hip.main import build_parser, main
    base = ["--problem-type", "seq_modeling", "--model-name", "cnn-mvae", "--input-type", "visuotactile", "--use-pose", "--no-cuda"]
    assert build_parser().parse_args(base).log_images == 0
    assert build_parser().parse_args(base + ["--log-images", "3"]).log_images == 3
    for bad in ("-1", "1.5", "x"):
        with pytest.raises(SystemExit):
            main(base + ["--log-images", bad, "--synthetic-batches", "1"])
    text = build_parser().format_help()
    assert "--log-images" in text and "noise" in text
