"""The exponential moving average of the parameters, host side (no GPU): MVAEStep(ema_decay) on the emulation against the recurrence
applied to snapshots of the parameters, the averaged state_dict and model, FusedAdam / FusedSGD(ema_decay), the one average an
engine and its fallback optimiser share, the --ema-decay / --ema-warmup flags, the checkpoint keys and the wrappers' argument
checks.  The kernels are emulated by tests/emu_backend_ema.py."""
import pytest
import torch

from mmdyn_hip import _lib, ops
from mmdyn_hip.engine import MVAEInference, MVAEStep
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.problems.problems import FusedAdam, FusedSGD, SeqModeling, SyntheticVisuoTactile
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise
from emu_backend_ema import EmuBackendEma, ema_reference, tick_values
import test_model_emu as T

D = 0.9


@pytest.fixture(autouse=True)
def emu():
    old = ops.set_backend(EmuBackendEma())
    yield
    ops.set_backend(old)


def rnd(n, seed):
    g = torch.Generator().manual_seed(seed + n)
    return torch.rand(n, generator=g) * 2 - 1


def _engine(B=4, use_pose=True, **kw):
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    eps, masks = seeded_noise(B, 256, n_pass, n_mask, 4321)
    return MVAEStep(T.build("cnn-mvae", True, use_pose, "cpu"), noise=InjectedNoise(eps, masks), precision="fp32", **kw)


def _train(step, inputs, targets, use_pose=True):
    """One train_step on freshly injected noise (an InjectedNoise is used up by the step that draws it)."""
    n_pass, n_mask = (7, 8) if use_pose else (3, 4)
    step.noise = InjectedNoise(*seeded_noise(inputs[0].shape[0], 256, n_pass, n_mask, 4321))
    return step.train_step(inputs, targets, 0.02)


def _recur(e, p, n, d=D, warmup=False):
    """One update of the recurrence: the average after update number n + 1, from the average ``e`` and the new parameters ``p``."""
    omd, _ = tick_values(n, d, warmup)
    return ema_reference(e.reshape(-1), p.reshape(-1), omd).view_as(e)


# ---- C ABI and wrappers ----------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_argument_errors():
    lib = _lib.load()
    for name in ("mmdyn_ema_tick", "mmdyn_ema_update", "mmdyn_adam_step_ema"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES
    assert lib.mmdyn_abi_version() == 6
    a, b = 4096, 8192             # (any non-null, aligned, disjoint addresses: the checks below return before a launch)
    assert lib.mmdyn_ema_tick(None, None, None) == -2
    assert lib.mmdyn_ema_update(None, b, a, 4, None) == -2
    assert lib.mmdyn_ema_update(a, None, a, 4, None) == -2
    assert lib.mmdyn_ema_update(a, b, None, 4, None) == -2
    assert lib.mmdyn_ema_update(a, b, a, -1, None) == -1
    assert lib.mmdyn_ema_update(a + 2, b, a, 4, None) == -1            # not 4-byte aligned
    assert lib.mmdyn_ema_update(a, a, a, 4, None) == -1                # ema is p
    assert lib.mmdyn_ema_update(a, a + 12, a, 4, None) == -1           # ema overlaps p
    assert lib.mmdyn_ema_update(a, a + 16, a, 0, None) == 0            # nothing to do: no launch
    args = (4, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0, None)
    assert lib.mmdyn_adam_step_ema(a, a, a, a, None, a, None, a, *args) == -2
    assert lib.mmdyn_adam_step_ema(a, a, a, a, b, a, None, None, *args) == -2
    assert lib.mmdyn_adam_step_ema(None, a, a, a, b, a, None, a, *args) == -2
    assert lib.mmdyn_adam_step_ema(a, a, a, a, a, a, None, a, *args) == -1          # ema is p
    assert lib.mmdyn_adam_step_ema(a, a, a, a, b + 4, a, None, a, *args) == -1      # ema not 16-byte aligned


def test_wrappers_reject_bad_arguments_before_any_launch():
    hip = ops.HipBackend()
    p, e = torch.zeros(8), torch.zeros(8)
    good = torch.zeros(4, dtype=torch.float64)
    for st in (torch.zeros(3, dtype=torch.float64), torch.zeros(4), torch.zeros(5, dtype=torch.float64), None):
        with pytest.raises(ValueError):
            hip.ema_tick(st)
        with pytest.raises(ValueError):
            hip.ema_update(e, p, st)
        with pytest.raises(ValueError):
            hip.adam_step_ema(p, p, p, p, e, torch.zeros(3, dtype=torch.float64), None, st, 1e-3, 0.9, 0.999, 1e-8, 1.0)
    with pytest.raises(ValueError, match="as many elements"):
        hip.ema_update(torch.zeros(7), p, good)
    with pytest.raises(ValueError, match="alias"):
        hip.ema_update(p, p, good)
    big = torch.zeros(12)
    with pytest.raises(ValueError, match="alias"):
        hip.ema_update(big[2:10], big[0:8], good)
    with pytest.raises(ValueError, match="alias"):
        hip.adam_step_ema(p, p, p, p, p, torch.zeros(3, dtype=torch.float64), None, good, 1e-3, 0.9, 0.999, 1e-8, 1.0)
    with pytest.raises(ValueError, match="six doubles"):
        hip.adam_step_ema(p, p, p, p, e, torch.zeros(3, dtype=torch.float64), None, good, 1e-3, 0.9, 0.999, 1e-8, 1.0, guarded=True)
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf"), None, "0.9", True, 1j):
        with pytest.raises(ValueError):
            ops.check_ema_decay(bad, "decay")
        with pytest.raises(ValueError):
            ops.new_ema_state(bad, False, "cpu")
    assert ops.check_ema_decay(0, "decay") == 0.0 and ops.check_ema_decay(0.9999, "decay") == 0.9999
    assert ops.new_ema_state(0.9999, True, "cpu").tolist() == [0.0, 0.9999, 0.0, 1.0]


def test_tick_rule():
    """Warm-up: d_n = min(d, (1 + n) / (10 + n)) for the count before the update -- 0.1, 2/11, 0.25, ... until d is the smaller."""
    st = ops.new_ema_state(0.5, True, "cpu")
    for n, want in enumerate((0.1, 2 / 11, 0.25, 4 / 13, 5 / 14, 0.4, 7 / 16, 8 / 17, 0.5, 0.5)):
        ops.B.ema_tick(st)
        assert float(st[2]) == 1.0 - want and float(st[0]) == n + 1
    st = ops.new_ema_state(0.9999, False, "cpu")
    ops.B.ema_tick(st)
    assert float(st[2]) == 1.0 - 0.9999 and float(st[0]) == 1.0
    skipped = torch.tensor([0, 0, 0, 0, 1, 1], dtype=torch.float64)
    before = st.clone()
    ops.B.ema_tick(st, skipped)                                       # a step the guard skipped: nothing moves
    assert torch.equal(st, before)


# ---- fused engine ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [False, True])
def test_engine_average_follows_the_recurrence(warmup):
    B = 4
    inputs, targets = seeded_batch(B, 1234)
    step = _engine(B, ema_decay=D, ema_warmup=warmup)
    assert step.ema_updates == 0 and torch.equal(step.ema_flat, step.params.flat)
    assert step.ema_flat.data_ptr() != step.params.flat.data_ptr()
    want = step.params.flat.clone()
    named = dict(step.model.named_parameters())
    for n in range(3):
        _train(step, inputs, targets)
        want = _recur(want, step.params.flat, n, warmup=warmup)
        got = step.ema_params()
        assert list(got) == list(named)
        for k, p in named.items():
            o = step.params.offsets[k]
            assert got[k].shape == p.shape
            assert torch.equal(got[k].reshape(-1), want[o:o + p.numel()]), (n, k)
        assert not torch.equal(step.ema_flat, step.params.flat)
    assert step.ema_updates == 3 and float(step.ema_state[0]) == 3.0


def test_engine_without_ema_is_the_engine_as_it_was():
    B = 4
    inputs, targets = seeded_batch(B, 1234)
    plain, off = _engine(B), _engine(B, ema_decay=None)
    for e in (plain, off):
        for _ in range(2):
            _train(e, inputs, targets)
        assert e.ema is None and e.ema_flat is None and e.ema_state is None and e.ema_updates == 0
    for a, b in ((plain.params.flat, off.params.flat), (plain.adam_m, off.adam_m), (plain.adam_v, off.adam_v),
                 (plain.adam_state, off.adam_state)):
        assert torch.equal(a, b)
    for call in (off.ema_params, off.ema_state_dict, off.ema_model):
        with pytest.raises(ValueError, match="ema_decay"):
            call()
    # the average leaves the step itself alone
    on = _engine(B, ema_decay=D)
    for _ in range(2):
        _train(on, inputs, targets)
    for a, b in ((plain.params.flat, on.params.flat), (plain.adam_m, on.adam_m), (plain.adam_v, on.adam_v),
                 (plain.adam_state, on.adam_state)):
        assert torch.equal(a, b)


def test_engine_with_clipping_keeps_the_average_of_the_clipped_steps():
    B = 4
    inputs, targets = seeded_batch(B, 1234)
    clipped, both = _engine(B, max_grad_norm=1e-3), _engine(B, max_grad_norm=1e-3, ema_decay=D)
    want = both.params.flat.clone()
    for n in range(2):
        _train(clipped, inputs, targets)
        _train(both, inputs, targets)
        want = _recur(want, both.params.flat, n)
    assert both.clipped_steps == 2 and both.ema_updates == 2
    assert torch.equal(clipped.params.flat, both.params.flat) and torch.equal(clipped.clip, both.clip)
    assert torch.equal(both.ema_flat, want)


def test_engine_rejects_bad_ema_decay():
    m = T.build("cnn-mvae", True, True, "cpu")
    for bad in (1, 1.0, -0.1, float("nan"), "0.9", True):
        with pytest.raises(ValueError):
            MVAEStep(m, ema_decay=bad)


def test_ema_state_dict_and_model():
    B = 4
    inputs, targets = seeded_batch(B, 1234)
    step = _engine(B, ema_decay=D)
    twin = step.ema_model()
    _train(step, inputs, targets)
    live = step.model.state_dict()
    sd = step.ema_state_dict()
    assert list(sd) == list(live)
    params = dict(step.model.named_parameters())
    buffers = dict(step.model.named_buffers())
    assert set(params) | set(buffers) == set(sd) and buffers
    for k, v in sd.items():
        if k in params:
            assert v.shape == live[k].shape and not torch.equal(v, live[k]), k
            assert v.data_ptr() == step.ema[k].data_ptr()
        else:
            assert v.data_ptr() == buffers[k].data_ptr(), k            # the live buffer itself
    # the model: one object, of the model's class, in eval mode, on the storage of ema_flat and of the live buffers
    assert step.ema_model() is twin and type(twin) is type(step.model) and not twin.training and step.model.training
    lo, hi = step.ema_flat.data_ptr(), step.ema_flat.data_ptr() + 4 * step.ema_flat.numel()
    for k, p in twin.named_parameters():
        assert p.data_ptr() == step.ema[k].data_ptr() and lo <= p.data_ptr() < hi and not p.requires_grad
        assert p.untyped_storage().data_ptr() == step.ema_flat.untyped_storage().data_ptr()
        assert torch.equal(p, sd[k])
    for k, b in twin.named_buffers():
        assert b is buffers[k]
    assert [k for k, _ in twin.named_parameters()] == list(params) and list(twin.state_dict()) == list(live)
    # a fresh model loaded from the dict holds the same values; the live model was not touched by any of this
    fresh = T.build("cnn-mvae", True, True, "cpu")
    fresh.load_state_dict(sd)
    for (k, a), (_, b) in zip(fresh.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(a, b), k
    assert step.params.still_attached()
    # serving: the engine built on the averaged model packs the average, and refresh() follows further training
    eng = MVAEInference(twin, precision="fp32", use_graph=False)
    w = "conv_net.0.weight"
    assert eng.P["ve"][w].data_ptr() == step.ema["visual_encoder." + w].data_ptr()
    before = eng.P["ve"][w].clone()
    _train(step, inputs, targets)
    eng.refresh()
    assert not torch.equal(eng.P["ve"][w], before) and torch.equal(eng.P["ve"][w], step.ema["visual_encoder." + w])


# ---- module-path optimisers ------------------------------------------------------------------------------------------------------
SIZES = (7, 1003)


@pytest.mark.parametrize("which", ["adam", "sgd"])
@pytest.mark.parametrize("warmup", [False, True])
def test_fused_optimisers_keep_the_average(which, warmup):
    ps = [torch.nn.Parameter(rnd(n, 60 + i)) for i, n in enumerate(SIZES)]
    names = ["a.weight", "b.bias"]
    kw = dict(ema_decay=D, ema_warmup=warmup, ema_names=names)
    opt = FusedAdam(ps, lr=1e-2, **kw) if which == "adam" else FusedSGD(ps, lr=1e-2, momentum=0.9, weight_decay=5e-4, **kw)
    assert opt.ema_updates == 0 and list(opt.ema_params()) == names
    want = [p.detach().clone() for p in ps]
    for s in range(2):
        for i, p in enumerate(ps):
            p.grad = rnd(p.numel(), 70 + 10 * s + i)
        before = [p.detach().clone() for p in ps]
        opt.step()
        for i, p in enumerate(ps):
            assert not torch.equal(p.detach(), before[i])
            want[i] = _recur(want[i], p.detach(), s, warmup=warmup)
            assert torch.equal(opt.ema_params()[names[i]], want[i]), (s, i)
    assert opt.ema_updates == 2


def test_fused_optimisers_without_ema_decay_launch_nothing_new():
    """ema_decay=None never touches the new ops (a backend without them serves it); a bad value is a ValueError."""
    from emu_backend import EmuBackend
    old = ops.set_backend(EmuBackend())
    try:
        for cls in (FusedAdam, FusedSGD):
            p = torch.nn.Parameter(rnd(7, 1))
            opt = cls([p], lr=1e-3)
            p.grad = rnd(7, 2)
            opt.step()
            assert opt.ema_decay is None and opt.ema_updates == 0
            with pytest.raises(ValueError, match="ema_decay"):
                opt.ema_params()
    finally:
        ops.set_backend(old)
    for cls in (FusedAdam, FusedSGD):
        for bad in (1.0, -0.5, float("nan"), "x"):
            with pytest.raises(ValueError):
                cls([torch.nn.Parameter(rnd(7, 1))], ema_decay=bad)
        with pytest.raises(ValueError, match="ema_names"):
            cls([torch.nn.Parameter(rnd(7, 1))], ema_decay=D, ema_names=["a", "b"])


# ---- one average per model -------------------------------------------------------------------------------------------------------
def test_engine_and_fallback_optimiser_share_one_average():
    """One engine step, then one step of a FusedAdam built on the engine's average (the gradients are those the engine's backward
    left in the parameters' .grad): count 2, and the engine's buffer holds the recurrence over both."""
    B = 4
    inputs, targets = seeded_batch(B, 1234)
    step = _engine(B, ema_decay=D)
    names = [k for k, _ in step.model.named_parameters()]
    opt = FusedAdam(step.model.parameters(), lr=1e-3, ema_names=names, ema_shared=step)
    assert opt.ema_decay == D and opt._ema_state is step.ema_state
    want = step.params.flat.clone()
    _train(step, inputs, targets)
    want = _recur(want, step.params.flat, 0)
    assert step.ema_updates == 1 and opt.ema_updates == 1 and torch.equal(step.ema_flat, want)
    flat1 = step.params.flat.clone()
    opt.step()
    assert not torch.equal(step.params.flat, flat1)
    want = _recur(want, step.params.flat, 1)
    assert step.ema_updates == 2 and opt.ema_updates == 2
    for k, e in opt.ema_params().items():
        o = step.params.offsets[k]
        assert e.data_ptr() == step.ema[k].data_ptr()
        assert torch.equal(e.reshape(-1), want[o:o + e.numel()]), k
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdam(step.model.parameters(), ema_names=names, ema_shared=_engine(B))
    with pytest.raises(ValueError, match="ema_names"):
        FusedAdam(step.model.parameters(), ema_shared=step)


def test_problem_keeps_one_average_whichever_path_steps(tmp_path):
    """A Problem with an engine: `_fused_applicable` is false only for a batch that is not the loader's list of tensors, and the
    module path of a cnn-mvae asserts on exactly that (`_evaluate_mvae` takes lists), so no valid batch of one epoch changes path.
    What can be driven is the fallback optimiser itself: an epoch of two fused steps, then its step -- one count, one buffer."""
    prob = SeqModeling(T.args(no_cuda=True, ema_decay=D, batchsize=2), log_dir=str(tmp_path), train_loader=SyntheticVisuoTactile(2, 2))
    step, opt = prob._step, prob._optimizer
    assert step is not None and step.ema_decay == D and opt._ema_state is step.ema_state
    assert not prob._fused_applicable(torch.zeros(2, 3)) and not prob._fused_applicable({'model_input': torch.zeros(2, 3)})
    want = step.params.flat.clone()
    prob._anneal_KL(0)
    prob._train_epoch(0)
    assert prob.ema_updates == 2
    ema2 = step.ema_flat.clone()
    opt.step()
    assert prob.ema_updates == 3 and step.ema_updates == 3 and opt.ema_updates == 3
    assert torch.equal(step.ema_flat, _recur(ema2, step.params.flat, 2))
    assert not torch.equal(step.ema_flat, want)
    for k, e in opt.ema_params().items():
        assert e.data_ptr() == step.ema[k].data_ptr()


# ---- command line and checkpoint -------------------------------------------------------------------------------------------------
def test_ema_flags_reach_the_engine_and_the_optimiser(tmp_path):
    from mmdyn_hip.main import build_parser, main
    base = ["--problem-type", "seq_modeling", "--model-name", "cnn-mvae", "--input-type", "visuotactile", "--use-pose", "--no-cuda"]
    a = build_parser().parse_args(base + ["--ema-decay", "0.999", "--ema-warmup"])
    assert a.ema_decay == 0.999 and a.ema_warmup is True
    a = build_parser().parse_args(base)
    assert a.ema_decay == 0 and a.ema_warmup is False
    for bad in ("1.0", "-0.1", "nan"):
        with pytest.raises(SystemExit):
            main(base + ["--ema-decay", bad, "--synthetic-batches", "1"])
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="--ema-decay"):
            SeqModeling(T.args(no_cuda=True, ema_decay=bad), log_dir=str(tmp_path))
    for over in (dict(), dict(ema_decay=0.0), dict(ema_decay=0)):
        prob = SeqModeling(T.args(no_cuda=True, **over), log_dir=str(tmp_path))
        assert prob._step.ema is None and prob._step.ema_decay is None and prob._optimizer.ema_decay is None
        assert prob.ema_state_dict() is None
    prob = SeqModeling(T.args(no_cuda=True, ema_decay=0.999, ema_warmup=True), log_dir=str(tmp_path))
    assert prob._step.ema_decay == 0.999 and prob._step.ema_warmup and prob._step.ema_state.tolist() == [0.0, 0.999, 0.0, 1.0]
    prob = SeqModeling(T.args(no_cuda=True, ema_decay=0.99, optimizer="SGD", model_name="cnn-vae", input_type="visual"),
                       log_dir=str(tmp_path))
    assert prob._step is None and isinstance(prob._optimizer, FusedSGD) and prob._optimizer.ema_decay == 0.99
    assert list(prob._optimizer.ema_params()) == [k for k, _ in prob._model.named_parameters()]


@pytest.mark.parametrize("fused", [True, False])
def test_checkpoint_holds_the_average_beside_the_model(tmp_path, fused):
    over = {} if fused else dict(model_name="cnn-vae", input_type="visual")

    def run(sub, **kw):
        d = tmp_path / sub
        prob = SeqModeling(T.args(no_cuda=True, batchsize=2, **over, **kw), log_dir=str(d), train_loader=SyntheticVisuoTactile(2, 2),
                           test_loader=SyntheticVisuoTactile(1, 2))
        assert (prob._step is not None) == fused
        prob._anneal_KL(0)
        prob._train_epoch(0)
        prob._test_epoch(0)
        return prob, torch.load(d / "checkpoint" / "epoch_0.ckpt", weights_only=False)

    prob, ck = run("off")
    assert set(ck) == {"model", "loss", "epoch"}
    prob, ck = run("on", ema_decay=D)
    assert set(ck) == {"model", "loss", "epoch", "model_ema", "ema_updates"}
    assert ck["ema_updates"] == 2 and list(ck["model_ema"]) == list(ck["model"])
    params = {k for k, _ in prob._model.named_parameters()}
    live = prob.ema_state_dict()
    for k, v in ck["model_ema"].items():
        assert v.device.type == "cpu" and torch.equal(v, live[k]) and v.data_ptr() != live[k].data_ptr()
        if k in params:
            assert not torch.equal(v, ck["model"][k]), k
        elif "num_batches" not in k:
            assert torch.equal(v, ck["model"][k]), k
    fresh = T.build("cnn-mvae", True, True, "cpu") if fused else None
    if fresh is not None:
        fresh.load_state_dict(ck["model_ema"])
