"""Drop-in module API + problem layer + fused engine, host logic on CPU (kernels emulated by
tests/emu_backend.py), checked against the golden vectors produced by the reference."""
import argparse
import atexit
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import setup_model, InjectedNoise, NoiseSource, ProductOfExperts
from mmdyn_hip.models.shapes import state_dict_shapes
from mmdyn_hip.problems.problems import SeqModeling, DynModeling, SyntheticVisuoTactile
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_batch, seeded_noise
from emu_backend import EmuBackend
from test_oracle_golden import summarize, close_summary, close_params, load

# the problems' log / checkpoint directory: one per test process, never a fixed path another user may own
LOG_DIR = tempfile.mkdtemp(prefix="mmdyn_test_logs_")
atexit.register(shutil.rmtree, LOG_DIR, True)

MODEL_KW = dict(condition_dim=0, input_dim=4096, architecture="cnn", conditional=False, categorical_conditions=False,
                latent_size=256)


@pytest.fixture(autouse=True)
def emu():
    old = ops.set_backend(EmuBackend())
    yield
    ops.set_backend(old)


def build(name, cross, use_pose=None, device="cpu", size=64):
    kw = dict(MODEL_KW, input_dim=size * size)
    if use_pose is not None:
        kw["use_pose"] = use_pose
    m = setup_model(name, cross_modal=cross, **kw)
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    return m.to(device).train()


def args(**over):
    d = dict(problem_type="seq_modeling", model_name="cnn-mvae", input_type="visuotactile", use_pose=True, lr=1e-3,
             dataset_path="", batchsize=4, criterion="crossentropy", optimizer="Adam", num_epochs=1, mask_loss=False,
             vis_pose=False, pose_multiplier=1000.0, save_name="t", no_cuda=False, kl_weight=1.0, latent_size=256,
             annealing_epochs=50, conditional=False)
    d.update(over)
    return argparse.Namespace(**d)


def check_forward_subsets(golden_dir, device):
    g = load(golden_dir, "mvae_forward_B3.npz")
    B = int(g["batch"])
    m = build("cnn-mvae", True, True, device)
    v, t, p = (torch.tensor(g[f"in{i}"]).to(device) for i in range(3))
    eps, masks = seeded_noise(B, 256, 8, 8, 99)
    m.noise = InjectedNoise(eps, masks)
    with torch.no_grad():
        for i, (a, b, c) in enumerate(g["subsets"]):
            vr, tr, pr, mu, lv = m([v if a else None, t if b else None], pose=p if c else None)
            np.testing.assert_allclose(mu.cpu().numpy(), g[f"s{i}/means"], rtol=1e-4, atol=3e-5)
            np.testing.assert_allclose(lv.cpu().numpy(), g[f"s{i}/log_var"], rtol=1e-4, atol=3e-5)
            np.testing.assert_allclose(pr.cpu().numpy(), g[f"s{i}/pose"], rtol=1e-4, atol=3e-5)
            close_summary(summarize(vr.cpu(), 256), g[f"s{i}/visual"], 3e-5, f"s{i} visual")
            close_summary(summarize(tr.cpu(), 256), g[f"s{i}/tactile"], 3e-5, f"s{i} tactile")
        vr, tr = m.inference(n=B)
        close_summary(summarize(vr.cpu(), 256), g["inference/visual"], 3e-5, "inference")
    sd = m.state_dict()
    for k in sd:
        if "running" in k or "num_batches" in k:
            np.testing.assert_allclose(sd[k].double().cpu().numpy(), g["buffer/" + k], rtol=2e-5, atol=2e-6, err_msg=k)


def check_reference_schedule_step(golden_dir, device, fname, use_pose):
    """fused=False: seven model() calls + autograd, as the reference does."""
    g = load(golden_dir, fname)
    B = int(g["batch"])
    prob = SeqModeling(args(use_pose=use_pose, no_cuda=(device == "cpu")), log_dir=LOG_DIR, fused=False)
    m = prob.model
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    inputs, targets = seeded_batch(B, 1234, with_pose=use_pose)
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass * int(g["n_steps"]), n_mask * int(g["n_steps"]), 4321)
    m.noise = InjectedNoise(eps, masks)
    prob._kl_weight = float(g["kl_weight"])
    x = {"model_input": [inputs[0].to(device), inputs[1].to(device)], "input_object_pose": [inputs[2].to(device)] if use_pose else None, "shock": None}
    t = {"target_output": [targets[0].to(device), targets[1].to(device)], "target_object_pose": [targets[2].to(device)] if use_pose else None, "loss_mask": None}
    prob._optimizer.zero_grad()
    outputs, loss = prob._evaluate_model(x, t)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(g["loss_step0"]), rel=1e-4)
    pm = outputs["perf_measure"]
    np.testing.assert_allclose([pm["visual"], pm["tactile"]], g["perf_measure"][:2], rtol=1e-4)
    np.testing.assert_allclose(outputs["means"].detach().cpu().numpy(), g["means"], rtol=1e-4, atol=3e-5)
    for k, p_ in m.named_parameters():
        close_summary(summarize(p_.grad.cpu()), g["grad/" + k], 1e-3, "grad " + k)
    prob._optimizer.step()
    for k, p_ in m.named_parameters():
        close_params(summarize(p_.detach().cpu()), g["param_step0/" + k], 1e-3, 1, "param " + k)
    sd = m.state_dict()
    for k in sd:
        if "running" in k or "num_batches" in k:
            np.testing.assert_allclose(sd[k].double().cpu().numpy(), g["buffer_step0/" + k], rtol=2e-5, atol=2e-6, err_msg=k)


def check_fused_engine(golden_dir, device, fname, use_pose, exact=False):
    g = load(golden_dir, fname)
    B, n_steps = int(g["batch"]), int(g["n_steps"])
    m = build("cnn-mvae", True, use_pose, device)
    inputs, targets = seeded_batch(B, 1234, with_pose=use_pose)
    inputs, targets = [x.to(device) for x in inputs], [x.to(device) for x in targets]
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass * n_steps, n_mask * n_steps, 4321)
    step = MVAEStep(m, lr=float(g["lr"]), pose_multiplier=float(g["pose_multiplier"]), noise=InjectedNoise(eps, masks),
                    exact_running_stats=exact)
    for s in range(n_steps):
        loss = step.forward(inputs, targets, float(g["kl_weight"]), train=True)
        assert float(loss) == pytest.approx(float(g[f"loss_step{s}"]), rel=1e-4), s
        if s == 0:
            np.testing.assert_allclose(step.partials[:n_pass].cpu().numpy(), g["loss_partials"], rtol=1e-4)
            np.testing.assert_allclose(step.last["means"].cpu().numpy(), g["means"], rtol=1e-4, atol=3e-5)
            np.testing.assert_allclose(step.last["log_var"].cpu().numpy(), g["log_var"], rtol=1e-4, atol=3e-5)
            close_summary(summarize(step.last["recon_x"][0].cpu(), 256), g["recon0"], 3e-5, "recon0")
            if use_pose:
                np.testing.assert_allclose(step.last["recon_x"][2].cpu().numpy(), g["recon2"], rtol=1e-4, atol=3e-5)
        handles = step.backward()
        if s == 0:
            for k, p_ in m.named_parameters():
                close_summary(summarize(p_.grad.cpu()), g["grad/" + k], 1e-3, "grad " + k)
        step.optimizer_step(handles)
        if s in (0, n_steps - 1):
            for k, p_ in m.named_parameters():
                close_params(summarize(p_.detach().cpu()), g[f"param_step{s}/" + k], float(g["lr"]), s + 1, f"param {k}")
    # encoder running statistics follow the reference exactly (4 identical EMA updates per step); the decoders' too
    # when the engine also runs the passes whose reconstructions the reference discards (exact_running_stats)
    sd = m.state_dict()
    for k in sd:
        if ("encoder" in k or exact) and ("running" in k or "num_batches" in k):
            np.testing.assert_allclose(sd[k].double().cpu().numpy(), g[f"buffer_step{n_steps - 1}/" + k], rtol=2e-5,
                                       atol=2e-3 if n_steps > 1 else 2e-6, err_msg=k)


def test_last_step_exact_running_stats_residual():
    """Checkpoint fidelity of the default schedule.  Reference schedule = the image decoders run on all
    7 passes of every step (exact_running_stats=True reproduces the reference's buffers: test_fused_engine_exact_running_
    stats).  Against it, after 3 "epochs" of 8 steps on fixed data: (live) live passes only on every step; (last) what
    Problem._train_epoch does by default: live passes only, the LAST step of each epoch exact.  Measured (printed; B = 2,
    first 24 steps of training): worst decoder buffer 24.7 % relative L2 off the reference schedule for (live), 10.6 %
    for (last) -- the discarded passes see different latents, so their batch statistics differ systematically and the
    last step's 7 updates only carry 1 - 0.9**7 = 52 % of a buffer.  Asserted: (last) < (live) and < 15 %.  Identical
    buffers need --exact-running-stats (every step exact)."""
    B, epochs, per = 2, 3, 8
    inputs, targets = seeded_batch(B, 1234, with_pose=True)
    bufs = {}
    for mode in ("exact", "live", "last"):
        m = build("cnn-mvae", True, True, "cpu")
        step = MVAEStep(m, lr=1e-3, noise=NoiseSource(3))
        for s in range(epochs * per):
            step.exact_running_stats = mode == "exact" or (mode == "last" and s % per == per - 1)
            step.train_step(inputs, targets, 0.02)
        sd = m.state_dict()
        bufs[mode] = {k: sd[k].double().numpy().copy() for k in sd if "decoder" in k and "running" in k}
    res = {mode: {k: float(np.linalg.norm(bufs[mode][k] - bufs["exact"][k]) / (np.linalg.norm(bufs["exact"][k]) + 1e-30))
                  for k in bufs["exact"]} for mode in ("live", "last")}
    worst = {mode: max(v.values()) for mode, v in res.items()}
    print("decoder running-buffer residual vs the reference schedule after", epochs * per, "steps:", worst)
    assert worst["last"] < worst["live"]
    assert worst["last"] < 0.15, worst


def check_fused_engine_mask_loss(device, mask_channels, B=3):
    """--mask-loss through the fused engine == the module path (seven... three model() calls + autograd, whose masked ELBO is
    pinned by the reference's elbo/*_masked vectors): loss, unmasked perf measures, every parameter gradient."""
    inputs, targets = seeded_batch(B, 77, with_pose=False)
    inputs, targets = [x.to(device) for x in inputs], [x.to(device) for x in targets]
    gen = torch.Generator().manual_seed(5)
    mask = (torch.rand(B, mask_channels, 64, 64, generator=gen) > 0.4).float().to(device)
    eps, masks = seeded_noise(B, 256, 3, 4, 4321)
    prob = SeqModeling(args(use_pose=False, mask_loss=True, no_cuda=(device == "cpu")), log_dir=LOG_DIR, fused=False)
    m = prob.model
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    m.noise = InjectedNoise(eps, masks)
    prob._kl_weight = 0.3
    x = {"model_input": inputs, "input_object_pose": None, "shock": None}
    t = {"target_output": targets, "target_object_pose": None, "loss_mask": mask}
    prob._optimizer.zero_grad()
    outputs, loss = prob._evaluate_model(x, t)
    loss.backward()
    m2 = build("cnn-mvae", True, False, device)
    step = MVAEStep(m2, noise=InjectedNoise(eps, masks))
    floss = step.forward(inputs, targets, 0.3, train=True, loss_mask=mask)
    step.backward()
    assert float(floss) == pytest.approx(float(loss.detach()), rel=2e-5)
    npx = B * targets[0][0].numel()
    acc = step.acc.cpu()
    assert float(acc[3, 1]) / npx == pytest.approx(outputs["perf_measure"]["visual"], rel=1e-5)
    assert float(acc[3, 2]) / npx == pytest.approx(outputs["perf_measure"]["tactile"], rel=1e-5)
    assert float(acc[0, 1]) != pytest.approx(float(acc[3, 1]), rel=1e-3)          # the loss slots hold the masked sums
    for (k, p1), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        d = float((p1.grad - p2.grad).norm() / (p1.grad.norm() + 1e-12))
        assert d < 1e-3, (k, d)


@pytest.mark.parametrize("mask_channels", [1, 3])
def test_fused_engine_mask_loss(mask_channels):
    check_fused_engine_mask_loss("cpu", mask_channels)


def test_exact_running_stats_flag_reaches_the_fused_step():
    """--exact-running-stats (main.py, a switch of this build) makes the fused step reproduce the decoders' BatchNorm
    running statistics of the reference's 7-forward schedule."""
    from mmdyn_hip.main import build_parser
    ns = build_parser().parse_args(["--problem-type", "seq_modeling", "--model-name", "cnn-mvae", "--input-type", "visuotactile",
                                    "--use-pose", "--exact-running-stats", "--no-cuda"])
    assert ns.exact_running_stats is True
    prob = SeqModeling(args(no_cuda=True, exact_running_stats=True), log_dir=LOG_DIR)
    assert prob._step is not None and prob._step.exact_running_stats is True
    assert SeqModeling(args(no_cuda=True), log_dir=LOG_DIR)._step.exact_running_stats is False


def test_mask_loss_engine_selection_and_errors():
    """--mask-loss runs the fused step when the model has no pose term; with --use-pose the reference fails on the (B, 7)
    pose term (problems.py:445-447) and so does the engine."""
    prob = SeqModeling(args(use_pose=False, mask_loss=True, no_cuda=True), log_dir=LOG_DIR)
    assert prob._step is not None
    prob = SeqModeling(args(use_pose=True, mask_loss=True, no_cuda=True), log_dir=LOG_DIR)
    assert prob._step is None
    inputs, targets = seeded_batch(2, 1)
    step = MVAEStep(build("cnn-mvae", True, True, "cpu"))
    with pytest.raises(ValueError):
        step.forward(inputs, targets, 1.0, loss_mask=torch.ones(2, 1, 64, 64))
    step = MVAEStep(build("cnn-mvae", True, False, "cpu"))
    with pytest.raises(ValueError):
        step.forward(inputs[:2], targets[:2], 1.0, loss_mask=torch.ones(2, 2, 64, 64))


def check_extended_size_vs_oracle(device, size, B, use_pose=True, n_steps=2, precision="fp32", loss_tol=1e-4, grad_tol=1e-3):
    """The 128 / 256 pixel extensions (BASELINE configs[3] / configs[4]; no reference architecture exists for them, the
    reference's FC is fixed at 256*5*5: models/shapes.py): fused engine against the CPU oracle's restatement of the same
    stack -- total ELBO and each partial, every gradient tensor, and the loss after an Adam step."""
    from oracle import mvae_oracle as O
    klw = 1.0 / 50
    sd = seeded_state_dict(state_dict_shapes("cnn-mvae", use_pose=use_pose, size=size), 0)
    prm, buf = O.split_state(sd)
    inputs, targets = seeded_batch(B, 1234, with_pose=use_pose, size=size)
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass * n_steps, n_mask * n_steps, 4321)
    m = build("cnn-mvae", True, use_pose, device, size=size)
    assert set(m.state_dict()) == set(sd), set(m.state_dict()) ^ set(sd)
    step = MVAEStep(m, noise=InjectedNoise(eps, masks), precision=precision)
    names = list(prm.keys())
    opt = O.Adam([prm[k] for k in names], lr=1e-3)
    gi, gt = [x.to(device) for x in inputs], [x.to(device) for x in targets]
    worst = 0.0
    for s in range(n_steps):
        opt.zero_grad()
        _, loss_o, partials_o = O.evaluate_mvae(prm, inputs, targets, eps[n_pass * s:n_pass * (s + 1)],
                                                masks[n_mask * s:n_mask * (s + 1)], klw, 1000.0, use_pose, buf)
        loss_o.backward()
        loss = step.forward(gi, gt, klw)
        assert float(loss) == pytest.approx(float(loss_o.detach()), rel=loss_tol), (size, s)
        np.testing.assert_allclose(step.partials[:n_pass].cpu().numpy(), [float(x.detach()) for x in partials_o],
                                   rtol=loss_tol if s == 0 else 5 * loss_tol)
        h = step.backward()
        if s == 0:
            assert tuple(step.last["recon_x"][0].shape) == (B, 3, size, size)
            named = dict(m.named_parameters())
            for k in names:
                a, b = named[k].grad.double().cpu() / step.loss_scale, prm[k].grad.double()    # (fp16 modes: static loss scale)
                err = float((a - b).norm() / (b.norm() + 1e-30))
                worst = max(worst, err)
                assert err < grad_tol, (k, err)
        step.optimizer_step(h)
        opt.step()
    return worst


@pytest.mark.parametrize("size,B,use_pose", [(128, 2, True), (128, 3, False), (256, 1, True)])
def test_extended_image_sizes(size, B, use_pose):
    check_extended_size_vs_oracle("cpu", size, B, use_pose, n_steps=1 if size == 256 else 2)


def test_fp16_precision_plumbing():
    """precision="fp16" (BASELINE configs[4] arithmetic) on the emulated kernels: operands rounded to IEEE half, fp32
    accumulate and storage; the fp32 oracle within the mode's stated tolerance."""
    check_extended_size_vs_oracle("cpu", 64, 3, True, n_steps=1, precision="fp16", loss_tol=2e-3, grad_tol=1e-1)


def test_fp16_overflow_guard_skips_the_step():
    """fp16 modes: a backward that overflowed (inf / NaN in the gradient buffer) does not reach the parameters -- the guarded Adam
    step skips it and counts it; the loss scale shrinks with the image area (4 * B at 64x64, B / 4 at 256x256)."""
    inputs, targets = seeded_batch(2, 5)
    eps, masks = seeded_noise(2, 256, 14, 16, 6)
    m = build("cnn-mvae", True, True, "cpu")
    step = MVAEStep(m, noise=InjectedNoise(eps, masks), precision="fp16")
    step.forward(inputs, targets, 0.02)
    h = step.backward()
    before = step.params.flat.clone()
    step.params.grad[5] = float("inf")
    step.optimizer_step(h)
    assert torch.equal(step.params.flat, before) and step.skipped_steps == 1
    step.forward(inputs, targets, 0.02)
    step.optimizer_step(step.backward())
    assert not torch.equal(step.params.flat, before) and step.skipped_steps == 1 and torch.isfinite(step.params.flat).all()
    assert step.loss_scale == 8.0
    i256, t256 = seeded_batch(1, 5, size=256)
    s256 = MVAEStep(build("cnn-mvae", True, True, "cpu", size=256), precision="fp16s")
    s256.forward(i256, t256, 0.02)
    assert s256.loss_scale == 0.25


def test_deferred_decoder_weight_gradients_equal_inline():
    """defer_wgrad: the decoders' weight-gradient GEMMs are queued during the decoder backward and launched afterwards (on
    their own streams in the replayed step) -- same calls, same operands: the gradient buffer is bit-identical."""
    inputs, targets = seeded_batch(3, 5)
    eps, masks = seeded_noise(3, 256, 7, 8, 6)
    grads = []
    for defer in (False, True):
        step = MVAEStep(build("cnn-mvae", True, True, "cpu"), noise=InjectedNoise(eps, masks), defer_wgrad=defer)
        step.forward(inputs, targets, 0.02)
        step.backward()
        grads.append(step.params.grad.clone())
    assert torch.equal(grads[0], grads[1])
    # the measured rule (engine.MVAEStep: profiles/r6/ab_defer_wgrad_16bit.txt): on in fp32 / fp32x3 and in the 16-bit storage modes
    # below 256 pixels; off for 16-bit matrix-core operands on fp32 storage, at 256 pixels in the storage modes, and data parallel
    assert MVAEStep(build("cnn-mvae", True, True, "cpu")).defer_wgrad
    assert MVAEStep(build("cnn-mvae", True, True, "cpu"), precision="fp32").defer_wgrad
    for prec in ("bf16s", "fp16s"):
        assert MVAEStep(build("cnn-mvae", True, True, "cpu"), precision=prec).defer_wgrad
        assert MVAEStep(build("cnn-mvae", True, True, "cpu", size=128), precision=prec).defer_wgrad
        assert not MVAEStep(build("cnn-mvae", True, True, "cpu", size=256), precision=prec).defer_wgrad
    for prec in ("bf16", "fp16"):
        assert not MVAEStep(build("cnn-mvae", True, True, "cpu"), precision=prec).defer_wgrad
    assert not MVAEStep(build("cnn-mvae", True, True, "cpu"), precision="bf16s", defer_wgrad=False).defer_wgrad


def test_fp32x3_precision_plumbing():
    """precision="fp32x3": fp32 storage and results, the GEMMs allowed onto the bf16 matrix cores through the exact three-term
    operand split.  On the emulated kernels (fp32 arithmetic) the mode is pure plumbing: same tolerances as "fp32", the backend
    sees precision "fp32" + fp32_split while a step runs and is restored afterwards."""
    from mmdyn_hip import ops
    check_extended_size_vs_oracle("cpu", 64, 3, True, n_steps=1, precision="fp32x3")
    assert ops.B.precision == "fp32" and not getattr(ops.B, "fp32_split", False)
    assert MVAEStep(build("cnn-mvae", True, True, "cpu"), precision="fp32x3").defer_wgrad
    with pytest.raises(ValueError):
        MVAEStep(build("cnn-mvae", True, True, "cpu"), precision="fp32x2")


def test_three_term_split_is_exact_and_its_dropped_products_are_below_fp32_rounding():
    """The arithmetic of csrc/common.h split3_bf16 (the X3 kernels), restated in numpy: hi = bf16(x), mid = bf16(x - hi),
    lo = x - hi - mid with round-to-nearest-even conversions leaves three bf16 values whose sum IS x, and the three cross products
    the kernels drop (mid.lo, lo.mid, lo.lo) are together below 2^-23 |a||b| -- less than ONE fp32 rounding of the product."""
    import numpy as np
    rng = np.random.default_rng(0)

    def bf16_rne(v):
        u = v.view(np.uint32).astype(np.uint64)
        return ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)

    def split(x):
        hi = bf16_rne(x)
        r = x - hi
        mid = bf16_rne(r)
        return hi, mid, r - mid
    a = (rng.standard_normal(200000) * 10.0 ** rng.integers(-20, 20, 200000)).astype(np.float32)
    b = (rng.standard_normal(200000) * 10.0 ** rng.integers(-10, 10, 200000)).astype(np.float32)
    ah, am, al = split(a)
    bh, bm, bl = split(b)
    for t in (ah, am, al, bh, bm, bl):
        assert np.array_equal(bf16_rne(t), t)                                    # every term is a bf16 value
    f = lambda v: v.astype(np.float64)
    assert np.array_equal(f(ah) + f(am) + f(al), f(a)) and np.array_equal(f(bh) + f(bm) + f(bl), f(b))
    six = f(ah) * f(bh) + f(ah) * f(bm) + f(am) * f(bh) + f(am) * f(bm) + f(ah) * f(bl) + f(al) * f(bh)
    exact = f(a) * f(b)
    rel = (six - exact) / exact
    assert np.abs(rel).max() <= 2.0 ** -23 and abs(rel.mean()) < 1e-10           # bounded and unbiased
    fp32_product = (a * b).astype(np.float64)                                     # one RNE rounding of the exact product
    assert np.sqrt((rel ** 2).mean()) < np.sqrt((((fp32_product - exact) / exact) ** 2).mean())


def test_fp16s_precision_plumbing():
    """precision="fp16s": as "fp16" with the convolution-level activations, their gradients and the packed weights stored
    in IEEE half (3 more mantissa bits than the bf16 of "bf16s" at the same bytes); FC level, logits and losses stay fp32."""
    from mmdyn_hip import layers, ops
    worst16s = check_extended_size_vs_oracle("cpu", 64, 3, True, n_steps=1, precision="fp16s", loss_tol=2e-3, grad_tol=1e-1)
    worstb = check_extended_size_vs_oracle("cpu", 64, 3, True, n_steps=1, precision="bf16s", loss_tol=5e-3, grad_tol=2e-1)
    assert worst16s < worstb, (worst16s, worstb)          # half storage is the more accurate of the two 16-bit storage modes
    assert ops.B.precision == "fp32" and layers.ACT_DTYPE == torch.float32 and layers.W_DTYPE == torch.float32
    inputs, targets = seeded_batch(2, 5)
    eps, masks = seeded_noise(2, 256, 7, 8, 6)
    step = MVAEStep(build("cnn-mvae", True, True, "cpu"), noise=InjectedNoise(eps, masks), precision="fp16s")
    step.forward(inputs, targets, 0.02)
    assert step.ctx["ev"]["stages"][0]["a"].dtype == torch.float16 and step.ctx["dv"]["stages"][2]["y"].dtype == torch.float16
    assert step.ctx["lgv"].dtype == torch.float32 and step.ctx["ov"].dtype == torch.float32
    assert step.loss_scale == 8.0


def test_extended_size_module_api_and_checks():
    """MVAE.forward / inference of a 128-pixel model, and the input-size check of a 64-pixel one."""
    from oracle import mvae_oracle as O
    m = build("cnn-mvae", True, True, "cpu", size=128)
    inputs, _ = seeded_batch(2, 7, size=128)
    eps, masks = seeded_noise(2, 256, 1, 2, 5)
    m.noise = InjectedNoise(eps + [torch.zeros(3, 256)], masks)
    with torch.no_grad():
        vr, tr, pr, mu, lv = m([inputs[0], inputs[1]], pose=inputs[2])
    prm, buf = O.split_state(seeded_state_dict(state_dict_shapes("cnn-mvae", use_pose=True, size=128), 0))
    ov, ot, op, omu, olv = O.mvae_forward(prm, inputs[0], inputs[1], inputs[2], eps[0], iter(masks), True, buf)
    assert tuple(vr.shape) == (2, 3, 128, 128)
    torch.testing.assert_close(mu, omu.detach(), rtol=1e-4, atol=3e-5)
    torch.testing.assert_close(vr, ov.detach(), rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(tr, ot.detach(), rtol=1e-3, atol=1e-4)
    assert tuple(m.inference(n=3)[1].shape) == (3, 3, 128, 128)
    m64 = build("cnn-mvae", True, True, "cpu")
    with pytest.raises(ValueError):
        m64([inputs[0], inputs[1]], pose=inputs[2])


def test_mvae_forward_subsets(golden_dir):
    check_forward_subsets(golden_dir, "cpu")


@pytest.mark.parametrize("fname,use_pose", [("mvae_pose_B4.npz", True), ("mvae_nopose_B4.npz", False)])
def test_reference_schedule_step(golden_dir, fname, use_pose):
    check_reference_schedule_step(golden_dir, "cpu", fname, use_pose)


@pytest.mark.parametrize("fname,use_pose", [("mvae_pose_B4.npz", True), ("mvae_nopose_B4.npz", False)])
def test_fused_engine_matches_reference(golden_dir, fname, use_pose):
    check_fused_engine(golden_dir, "cpu", fname, use_pose)


@pytest.mark.parametrize("fname,use_pose", [("mvae_pose_B4.npz", True), ("mvae_nopose_B4.npz", False)])
def test_fused_engine_exact_running_stats(golden_dir, fname, use_pose):
    check_fused_engine(golden_dir, "cpu", fname, use_pose, exact=True)


def check_vae_config1(golden_dir, device):
    g = load(golden_dir, "vae_visual_B16.npz")
    prob = SeqModeling(args(model_name="cnn-vae", input_type="visual", use_pose=False, no_cuda=(device == "cpu")),
                       log_dir=LOG_DIR, fused=False)
    m = prob.model
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    eps, masks = seeded_noise(16, 256, 2, 2, 31)
    m.noise = InjectedNoise(eps, masks)
    prob._kl_weight = float(g["kl_weight"])
    x, y = torch.tensor(g["x"]).to(device), torch.tensor(g["y"]).to(device)
    for s in range(2):
        prob._optimizer.zero_grad()
        out, loss = prob._evaluate_model({"model_input": x, "shock": None}, {"target_output": y, "loss_mask": None})
        loss.backward()
        assert float(loss.detach()) == pytest.approx(float(g[f"loss_step{s}"]), rel=1e-4)
        if s == 0:
            assert out["perf_measure"]["visual"] == pytest.approx(float(g["perf_measure"]), rel=1e-4)
            for k, p_ in m.named_parameters():
                close_summary(summarize(p_.grad.cpu()), g["grad/" + k], 1e-3, "grad " + k)
        prob._optimizer.step()


def test_vae_config1(golden_dir):
    check_vae_config1(golden_dir, "cpu")


def test_product_of_experts_module(golden_dir):
    g = load(golden_dir, "small_ops.npz")
    mu = torch.tensor(g["poe/mu"], requires_grad=True)
    lv = torch.tensor(g["poe/logvar"], requires_grad=True)
    pm, plv = ProductOfExperts()(mu, lv)
    np.testing.assert_allclose(pm.detach().numpy(), g["poe/out_mu"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(plv.detach().numpy(), g["poe/out_logvar"], rtol=1e-5, atol=1e-5)
    (pm.sum() + plv.sum()).backward()
    assert torch.isfinite(mu.grad).all() and torch.isfinite(lv.grad).all()


def test_parse_input_and_training_loop(golden_dir, tmp_path):
    g = load(golden_dir, "small_ops.npz")
    data = [torch.tensor(g[f"parse/data{i}"]) for i in range(5)]
    target = [torch.tensor(g[f"parse/target{i}"]) for i in range(4)]
    for cls, tag in ((SeqModeling, "seq"), (DynModeling, "dyn")):
        for it in ("visual", "tactile", "visuotactile"):
            p = cls.__new__(cls)
            p._seq_length, p._device, p.parameters = int(g["parse/seq_length"]), torch.device("cpu"), {"input_type": it}
            x, t = p.parse_input([d.clone() for d in data], [d.clone() for d in target])
            mi, to = x["model_input"], t["target_output"]
            if not isinstance(mi, list):
                mi, to = [mi], [to]
            pre = f"parse/{tag}/{it}/"
            for j in range(len(mi)):
                np.testing.assert_array_equal(mi[j].numpy(), g[pre + f"model_input{j}"])
                np.testing.assert_array_equal(to[j].numpy(), g[pre + f"target_output{j}"])
            np.testing.assert_array_equal(t["target_object_pose"][0].numpy(), g[pre + "target_pose"])
            np.testing.assert_array_equal(x["shock"].numpy(), g[pre + "shock"])
    # KL annealing + one tiny epoch through the fused engine, checkpoint format
    prob = SeqModeling(args(num_epochs=1, no_cuda=True), log_dir=str(tmp_path), fused=True,
                       train_loader=SyntheticVisuoTactile(2, 2), test_loader=SyntheticVisuoTactile(1, 2, seed=7))
    sched = []
    for e in range(60):
        prob._anneal_KL(e)
        sched.append(prob._kl_weight)
    np.testing.assert_allclose(sched, g["anneal/kl"])
    prob.train()
    ck = [f for f in os.listdir(prob.checkpoint_dir) if f.endswith(".ckpt")]
    assert ck == ["epoch_0.ckpt"]
    state = torch.load(os.path.join(prob.checkpoint_dir, ck[0]), weights_only=False)
    assert set(state) == {"model", "loss", "epoch"}
    assert list(state["model"].keys()) == list(state_dict_shapes("cnn-mvae", use_pose=True).keys())
    assert os.path.exists(os.path.join(str(tmp_path), "results.pkl"))


def check_conditional(golden_dir, device):
    """--conditional cnn-mvae through the module API against vectors from the reference (B=2, condition_dim=3)."""
    g = load(golden_dir, "mvae_conditional_B2.npz")
    B = int(g["batch"])
    kw = dict(MODEL_KW)
    kw.update(conditional=True, condition_dim=3, use_pose=True)
    m = setup_model("cnn-mvae", cross_modal=True, **kw)
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    m.to(device).train()
    assert m.visual_encoder.linear_means.weight.shape == (256, 515) and m.visual_decoder.upsample[0].weight.shape == (6400, 259)
    prob = SeqModeling.__new__(SeqModeling)
    prob._model, prob._kl_weight, prob._pose_multiplier = m, float(g["kl_weight"]), 1000.0
    prob.parameters = {"use_pose": True, "model_name": "cnn-mvae", "mask_loss": False, "input_type": "visuotactile"}
    inputs, targets = seeded_batch(B, 321)
    eps, masks = seeded_noise(B, 256, 7, 8, 77)
    m.noise = InjectedNoise(eps, masks)
    cond = torch.tensor(g["cond"]).to(device)
    outputs, loss = prob._evaluate_mvae(x=[t.to(device) for t in inputs], targets=[t.to(device) for t in targets], condition=cond)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(g["loss"]), rel=1e-4)
    np.testing.assert_allclose(outputs["means"].detach().cpu().numpy(), g["means"], rtol=1e-4, atol=3e-5)
    np.testing.assert_allclose(outputs["recon_x"][2].detach().cpu().numpy(), g["recon2"], rtol=1e-4, atol=3e-5)
    for k, p_ in m.named_parameters():
        close_summary(summarize(p_.grad.cpu()), g["grad/" + k], 1e-3, "grad " + k)


def test_conditional_mvae(golden_dir):
    check_conditional(golden_dir, "cpu")


def check_fused_engine_conditional(golden_dir, device):
    """The same --conditional step through the fused engine: loss, means, pose reconstruction and every parameter gradient
    against the reference's vectors; a condition is required, and refused by an unconditional model."""
    g = load(golden_dir, "mvae_conditional_B2.npz")
    B = int(g["batch"])
    kw = dict(MODEL_KW)
    kw.update(conditional=True, condition_dim=3, use_pose=True)
    m = setup_model("cnn-mvae", cross_modal=True, **kw)
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    m.to(device).train()
    inputs, targets = seeded_batch(B, 321)
    inputs, targets = [t.to(device) for t in inputs], [t.to(device) for t in targets]
    eps, masks = seeded_noise(B, 256, 7, 8, 77)
    cond = torch.tensor(g["cond"]).to(device)
    step = MVAEStep(m, noise=InjectedNoise(eps, masks))
    loss = step.forward(inputs, targets, float(g["kl_weight"]), train=True, condition=cond)
    assert float(loss) == pytest.approx(float(g["loss"]), rel=1e-4)
    np.testing.assert_allclose(step.last["means"].cpu().numpy(), g["means"], rtol=1e-4, atol=3e-5)
    np.testing.assert_allclose(step.last["recon_x"][2].cpu().numpy(), g["recon2"], rtol=1e-4, atol=3e-5)
    step.backward()
    for k, p_ in m.named_parameters():
        close_summary(summarize(p_.grad.cpu()), g["grad/" + k], 1e-3, "grad " + k)
    with pytest.raises(ValueError):
        step.forward(inputs, targets, 1.0)
    with pytest.raises(ValueError):
        MVAEStep(build("cnn-mvae", True, True, device)).forward(inputs, targets, 1.0, condition=cond)
    return step, inputs, targets, cond


def test_fused_engine_conditional(golden_dir):
    check_fused_engine_conditional(golden_dir, "cpu")


def check_conditional_loops(tmp_path, no_cuda):
    """--conditional through Problem.train(): cnn-mvae (shock-conditioned: the fused step) and cnn-vae with the SGD option
    (module API)."""
    for i, over in enumerate((dict(model_name="cnn-mvae"), dict(model_name="cnn-vae", input_type="visual", optimizer="SGD"))):
        prob = SeqModeling(args(num_epochs=1, no_cuda=no_cuda, conditional=True, batchsize=2, **over),
                           log_dir=str(tmp_path / str(i)), train_loader=SyntheticVisuoTactile(2, 2, shock_dim=3),
                           test_loader=SyntheticVisuoTactile(1, 2, seed=7, shock_dim=3))
        assert prob.condition_dim == 3 and (prob._step is not None) == (i == 0)
        before = {k: v.detach().clone() for k, v in prob.model.state_dict().items()}
        prob.train()
        after = prob.model.state_dict()
        fl = [k for k in before if before[k].dtype.is_floating_point]
        assert all(not torch.equal(before[k], after[k]) for k in fl)
        assert all(torch.isfinite(v).all() for v in after.values())
    with pytest.raises(ValueError):
        SeqModeling(args(conditional=True, no_cuda=no_cuda), log_dir=str(tmp_path / "x"),
                    train_loader=SyntheticVisuoTactile(1, 2), test_loader=SyntheticVisuoTactile(1, 2))


def test_conditional_training_loops(tmp_path):
    check_conditional_loops(tmp_path, no_cuda=True)


def check_regressor(golden_dir, device, tmp_path):
    """Regressor baseline through setup_model + the Regression problem against vectors from the reference."""
    from mmdyn_hip.problems.problems import Regression
    g = load(golden_dir, "regressor_B4.npz")
    B = int(g["batch"])
    _, masks = seeded_noise(B, 256, 1, 2, 55)
    x, pose, cond = (torch.tensor(g[k]).to(device) for k in ("x", "pose", "cond"))
    for tag in ("plain", "cond"):
        m = setup_model("regressor", out_dim=7, conditional=tag == "cond", num_classes=3)
        assert list(m.state_dict().keys()) == [str(k) for k in g[tag + "/keys"]]
        m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
        m.to(device).train()
        m.noise = InjectedNoise([], [masks[0] if tag == "plain" else masks[1]])
        prob = Regression.__new__(Regression)
        prob._model, prob._conditional = m, tag == "cond"
        out, loss = prob._evaluate_model({"model_input": x, "shock": cond}, pose)
        loss.backward()
        assert float(loss.detach()) == pytest.approx(float(g[tag + "/loss"]), rel=1e-4)
        np.testing.assert_allclose(out["outputs"].detach().cpu().numpy(), g[tag + "/out"], rtol=1e-4, atol=3e-5)
        for k, p_ in m.named_parameters():
            close_summary(summarize(p_.grad.cpu()), g[f"{tag}/grad/" + k], 1e-3, "grad " + k)
        for k, b in m.named_buffers():
            np.testing.assert_allclose(b.double().cpu().numpy(), g[f"{tag}/buffer/" + k], rtol=1e-4, atol=1e-5, err_msg=k)
    with pytest.raises(TypeError):
        setup_model("regressor")             # num_classes=None: the reference raises the same TypeError (models.py:37)
    # one tiny epoch through Problem.train()
    prob = Regression(args(problem_type="regression", model_name="regressor", input_type="tactile", num_epochs=1,
                           no_cuda=device == "cpu", conditional=True, batchsize=2),
                      log_dir=str(tmp_path), train_loader=SyntheticVisuoTactile(2, 2, shock_dim=3),
                      test_loader=SyntheticVisuoTactile(1, 2, seed=7, shock_dim=3))
    prob.train()
    assert os.path.exists(os.path.join(str(tmp_path), "results.pkl"))


def test_regressor(golden_dir, tmp_path):
    check_regressor(golden_dir, "cpu", tmp_path)


def test_bf16_precision_plumbing():
    """MVAEStep(precision='bf16') switches the matrix-core precision of the backend for the duration of each call
    (the emulation rounds the GEMM operands to bf16) and leaves the default in place afterwards."""
    from mmdyn_hip import ops
    from mmdyn_hip.engine import MVAEStep
    B, klw = 2, 0.02
    inputs, targets = seeded_batch(B, 5)
    eps, masks = seeded_noise(B, 256, 7, 8, 6)
    losses = {}
    from mmdyn_hip import layers
    grads = {}
    for prec in ("fp32", "bf16", "bf16s"):
        m = build("cnn-mvae", True, True, "cpu")
        step = MVAEStep(m, noise=InjectedNoise(eps, masks), precision=prec)
        losses[prec] = float(step.forward(inputs, targets, klw))
        if prec == "bf16s":                      # conv-level activations are stored in bf16, FC level / logits in fp32
            assert step.ctx["ev"]["stages"][0]["a"].dtype == torch.bfloat16 and step.ctx["dv"]["stages"][2]["y"].dtype == torch.bfloat16
            assert step.ctx["lgv"].dtype == torch.float32 and step.ctx["ov"].dtype == torch.float32
        step.backward()
        assert ops.B.precision == "fp32" and layers.ACT_DTYPE == torch.float32
        assert torch.isfinite(step.params.grad).all()
        grads[prec] = step.params.grad.clone()
    for prec in ("bf16", "bf16s"):
        r = abs(losses[prec] - losses["fp32"]) / abs(losses["fp32"])
        assert 1e-8 < r < 5e-3, (prec, r)
        assert float((grads[prec] - grads["fp32"]).norm() / grads["fp32"].norm()) < 0.1
    with pytest.raises(ValueError):
        MVAEStep(build("cnn-mvae", True, True, "cpu"), precision="fp8")


def check_mlp_vae(golden_dir, device):
    """'mlp-vae' through setup_model and the Reconstruction criterion against vectors from the reference."""
    g = load(golden_dir, "mlp_vae_B6.npz")
    m = setup_model("mlp-vae", input_dim=784, architecture="mlp", latent_size=32, condition_dim=0, conditional=False,
                    categorical_conditions=False)
    assert list(m.state_dict().keys()) == [str(k) for k in g["keys"]]
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    m.to(device).train()
    m.noise = InjectedNoise([torch.tensor(g["eps"]), torch.randn(3, 32)], [])
    x = torch.tensor(g["x"]).to(device)
    recon, mu, lv = m(x)
    prob = SeqModeling.__new__(SeqModeling)
    prob._kl_weight = 0.1
    loss = prob._elbo_loss(recon, x, mu, lv)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(g["loss"]), rel=1e-4)
    np.testing.assert_allclose(recon.detach().cpu().numpy(), g["recon"], rtol=1e-4, atol=3e-5)
    for k, p_ in m.named_parameters():
        close_summary(summarize(p_.grad.cpu()), g["grad/" + k], 1e-3, "grad " + k)
    assert tuple(m.inference(3).shape) == (3, 784)


def test_mlp_vae(golden_dir):
    check_mlp_vae(golden_dir, "cpu")


def check_dyn_modeling_and_cli(tmp_path, no_cuda):
    """BASELINE configs[3]'s problem type at the reference's own resolution: dyn_modeling (one-step predictor,
    problems.py:765-803) trains through the fused engine on sequences of 3 frames; and the CLI (main.py flags)
    drives seq_modeling / reconstruction end to end on synthetic batches."""
    from mmdyn_hip.main import main
    prob = DynModeling(args(problem_type="dyn_modeling", num_epochs=1, no_cuda=no_cuda, batchsize=2),
                       log_dir=str(tmp_path / "dyn"), seq_length=3,
                       train_loader=SyntheticVisuoTactile(2, 2, seq_length=3), test_loader=SyntheticVisuoTactile(1, 2, 3, seed=7))
    assert prob._step is not None
    prob.train()
    assert prob._step.last["means"].shape[0] == 6            # every frame of the 2 x 3 batch is a sample
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        mv = ["--input-type", "visuotactile", "--model-name", "cnn-mvae"]
        for extra in (mv + ["--problem-type", "seq_modeling", "--use-pose"], mv + ["--problem-type", "reconstruction"],
                      mv + ["--problem-type", "seq_modeling", "--mask-loss"],       # (with pose the reference raises too)
                      mv + ["--problem-type", "seq_modeling", "--use-pose", "--conditional", "--optimizer", "SGD"],
                      ["--problem-type", "seq_modeling", "--model-name", "cnn-vae", "--input-type", "tactile"],
                      ["--problem-type", "regression", "--model-name", "regressor", "--input-type", "visual"]):
            argv = ["--batchsize", "2", "--num-epochs", "1", "--synthetic-batches", "2", "--save-name", "cli"] + extra \
                + (["--no-cuda"] if no_cuda else [])
            p = main(argv)
            assert os.path.exists(os.path.join(p.log_dir, "results.pkl"))
    finally:
        os.chdir(cwd)


def test_dyn_modeling_and_cli(tmp_path):
    check_dyn_modeling_and_cli(tmp_path, no_cuda=True)


def check_eval_mode(golden_dir, device):
    """model.eval() on the HIP modules: running-estimate BatchNorm, no dropout, buffers untouched; back in train()
    the batch-statistics path is used again."""
    from mmdyn_hip.utils.seeded_init import seeded_running_stats
    g = load(golden_dir, "eval_mode_B3.npz")
    B = int(g["batch"])
    inputs, _ = seeded_batch(B, 4242, with_pose=True)
    inputs = [x.to(device) for x in inputs]
    eps = [torch.tensor(g[f"eps{i}"]) for i in range(4)]
    m = build("cnn-mvae", True, True, device)
    m.load_state_dict(seeded_running_stats({k: v.cpu() for k, v in m.state_dict().items()}))
    m.eval()
    m.noise = InjectedNoise(eps[:2], [])
    v, t, p, mu, lv = m([inputs[0], inputs[1]], pose=inputs[2])
    np.testing.assert_allclose(v[0].cpu().numpy(), g["mvae/visual0"], rtol=1e-4, atol=3e-5)
    close_summary(summarize(t.cpu(), 256), g["mvae/tactile"], 3e-5, "tactile")
    np.testing.assert_allclose(p.detach().cpu().numpy(), g["mvae/pose"], rtol=1e-4, atol=3e-5)
    np.testing.assert_allclose(mu.detach().cpu().numpy(), g["mvae/means"], rtol=1e-4, atol=3e-5)
    iv, it = m.inference(n=B)
    np.testing.assert_allclose(iv[0].cpu().numpy(), g["mvae/inference_visual0"], rtol=1e-4, atol=3e-5)
    close_summary(summarize(it.cpu(), 256), g["mvae/inference_tactile"], 3e-5, "inference tactile")
    for k, b in m.named_buffers():
        np.testing.assert_allclose(b.double().cpu().numpy(), g["mvae/buffer/" + k], rtol=1e-6, err_msg=k)
    m.train()                                                   # batch statistics again: the buffers move
    m.noise = InjectedNoise([eps[3]], [torch.ones(B, 512, dtype=torch.uint8)] * 2)
    m([inputs[0], inputs[1]], pose=inputs[2])
    assert int(m.visual_encoder.conv_net[3].num_batches_tracked) == 4
    vae = build("cnn-vae", False, None, device)
    vae.load_state_dict(seeded_running_stats({k: v.cpu() for k, v in vae.state_dict().items()}))
    vae.eval()
    vae.noise = InjectedNoise([eps[2]], [])
    r, mu, _ = vae(inputs[1])
    np.testing.assert_allclose(r[0].cpu().numpy(), g["vae/recon0"], rtol=1e-4, atol=3e-5)
    reg = setup_model("regressor", out_dim=7, conditional=False, num_classes=0)
    reg.load_state_dict(seeded_running_stats(seeded_state_dict(reg.state_dict(), 0)))
    reg.to(device).eval()
    np.testing.assert_allclose(reg(inputs[0]).detach().cpu().numpy(), g["regressor/out"], rtol=1e-4, atol=3e-5)


def test_eval_mode(golden_dir):
    check_eval_mode(golden_dir, "cpu")


def check_inference_engine(golden_dir, device):
    """engine.MVAEInference (prepacked weights, two streams, HIP-graph replay) == the eval-mode module forward ==
    the reference in eval mode; replays draw fresh latent noise; subsets of modalities work."""
    from mmdyn_hip.engine import MVAEInference
    from mmdyn_hip.utils.seeded_init import seeded_running_stats
    g = load(golden_dir, "eval_mode_B3.npz")
    B = int(g["batch"])
    inputs, _ = seeded_batch(B, 4242, with_pose=True)
    inputs = [x.to(device) for x in inputs]
    m = build("cnn-mvae", True, True, device)
    m.load_state_dict(seeded_running_stats({k: v.cpu() for k, v in m.state_dict().items()}))
    m.eval()
    eng = MVAEInference(m)
    eng.noise = InjectedNoise([torch.tensor(g["eps0"]), torch.tensor(g["eps1"])], [])
    eng.use_graph = False                                   # injected noise: compare with the reference's vectors
    v, t, p, mu, lv = eng([inputs[0], inputs[1]], pose=inputs[2])
    np.testing.assert_allclose(v[0].cpu().numpy(), g["mvae/visual0"], rtol=1e-4, atol=3e-5)
    close_summary(summarize(t.cpu(), 256), g["mvae/tactile"], 3e-5, "tactile")
    np.testing.assert_allclose(p.cpu().numpy(), g["mvae/pose"], rtol=1e-4, atol=3e-5)
    np.testing.assert_allclose(mu.cpu().numpy(), g["mvae/means"], rtol=1e-4, atol=3e-5)
    iv, it = eng.inference(B)
    np.testing.assert_allclose(iv[0].cpu().numpy(), g["mvae/inference_visual0"], rtol=1e-4, atol=3e-5)
    # device noise + graph replay (on the GPU): deterministic means, fresh latent draws per call, subsets
    eng = MVAEInference(m, seed=5)
    outs = [tuple(x.clone() for x in eng([inputs[0], inputs[1]], pose=inputs[2])) for _ in range(3)]
    for o in outs[1:]:
        assert torch.equal(o[3], outs[0][3]) and torch.equal(o[4], outs[0][4])       # means / log_var: no randomness
    assert not torch.equal(outs[1][0], outs[0][0]) and not torch.equal(outs[2][0], outs[1][0])   # z differs per call
    np.testing.assert_allclose(outs[0][3].cpu().numpy(), g["mvae/means"], rtol=1e-4, atol=3e-5)
    v_only = eng([inputs[0], None])
    assert v_only[2] is not None and tuple(v_only[0].shape) == (B, 3, 64, 64)
    a, b = eng.inference(5), None
    assert tuple(a[0].shape) == (5, 3, 64, 64)
    for prec, tol in (("bf16", 2e-2), ("bf16s", 3e-2), ("fp16", 5e-3), ("fp16s", 5e-3)):   # reduced-precision serving: close to fp32
        e2 = MVAEInference(m, precision=prec, seed=5)
        o2 = e2([inputs[0], inputs[1]], pose=inputs[2])
        np.testing.assert_allclose(o2[3].cpu().numpy(), g["mvae/means"], rtol=tol, atol=tol)
        assert o2[0].dtype == torch.float32
    for k, bb in m.named_buffers():
        np.testing.assert_allclose(bb.double().cpu().numpy(), g["mvae/buffer/" + k], rtol=1e-6, err_msg=k)


def test_inference_engine(golden_dir):
    check_inference_engine(golden_dir, "cpu")
