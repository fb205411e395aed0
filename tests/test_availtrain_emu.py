"""The fused training step on mixed-modality batches on the CPU (``MVAEStep(available=, target_available=)``, emulation backend of
tests/emu_backend_availtrain.py) against the torch-autograd yardstick of tests/availtrain_cases.py.  Tolerances are those of
tests/test_weighted_emu.py: loss and partials 1e-4 relative, every gradient tensor 1e-3 relative L2."""
import numpy as np
import pytest
import torch

import availtrain_cases as A
import test_model_emu as TM
from emu_backend_availtrain import EmuBackendAvailTrain
from emu_backend_iw import Recorder
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.problems.problems import DynModeling, SeqModeling, SyntheticVisuoTactile
from mmdyn_hip.utils.seeded_init import seeded_state_dict

REL, GREL = 1e-4, 1e-3


@pytest.fixture(autouse=True)
def emu_availtrain():
    old = ops.set_backend(EmuBackendAvailTrain())
    yield
    ops.set_backend(old)


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / (want.double().norm() + 1e-30))


def engine_run(device, name, kl="batch", w=None, tables=True, train=True, precision=None, available=None, target_available=None,
               backward=True, **kw):
    """One forward (+ backward) of a fresh engine on seeded weights and the case's noise.  ``tables``: True the case's own, False
    none (the plain step), or give ``available`` / ``target_available``.  -> (step, loss, partials, last_rows, {name: gradient})."""
    use_pose, B, inputs, targets, eps, masks, mask, tin, ttg = A.case(name)
    if tables is True:
        available, target_available = tin, ttg
    m = TM.build("cnn-mvae", True, use_pose, device)
    step = MVAEStep(m, pose_multiplier=A.POSE_MULTIPLIER, noise=InjectedNoise(eps, masks),
                    **({} if precision is None else {"precision": precision}), **kw)
    dv = lambda t: None if t is None else t.to(device)
    loss = float(step.forward([dv(x) for x in inputs], [dv(x) for x in targets], A.KL_WEIGHT, train=train, loss_mask=dv(mask),
                              sample_weight=dv(w), kl=kl, available=dv(available), target_available=dv(target_available)))
    partials, rows = step.partials[:step.P].clone(), None if step.last_rows is None else dict(step.last_rows)
    grads = None
    if train and backward:
        step.backward()
        grads = {k: (p.grad / step.loss_scale).clone() for k, p in m.named_parameters()}
    return step, loss, partials, rows, grads


def check_engine_vs_yardstick(device, name, kl, weighted, precision=None):
    """Loss, per-pass partials, per-sample rows, the per-term tables and every parameter gradient against the yardstick."""
    B = A.CASES[name][1]
    w = A.weights(B) if weighted else None
    prm, loss_y, partials_y, rows_y = A.yardstick(name, kl, w)
    keys = list(prm)
    gy = dict(zip(keys, torch.autograd.grad(loss_y, [prm[k] for k in keys], retain_graph=True)))
    step, loss, partials, rows, grads = engine_run(device, name, kl, w, precision=precision)
    print(name, kl, "weighted" if weighted else "w=1", precision, "loss", loss, "yardstick", float(loss_y.detach()))
    assert loss == pytest.approx(float(loss_y.detach()), rel=REL)
    np.testing.assert_allclose(partials.cpu().numpy(), partials_y.detach().numpy(), rtol=REL)
    np.testing.assert_allclose(rows["rows"].cpu().numpy(), rows_y.detach().numpy(), rtol=REL)
    _, terms, _ = A.yardstick_terms(name)
    pm = torch.tensor([1.0, 1.0, A.POSE_MULTIPLIER], dtype=torch.float64)
    got = torch.stack([rows["bce_v_rows"].cpu(), rows["bce_t_rows"].cpu(), rows["mse_rows"].cpu()]) * pm[:, None, None]
    np.testing.assert_allclose(got.numpy(), terms.detach().double().numpy(), rtol=REL, atol=0)
    tgt = A.full_table(A.case(name)[8], B)
    assert torch.equal(rows["present"].cpu(), tgt.double().sum(0))
    np.testing.assert_allclose((rows["term_sums"].cpu() * pm[:, None]).numpy(), terms.detach().double().sum(2).numpy(), rtol=REL)
    worst = {k: rel_l2(gr.cpu(), gy[k]) for k, gr in grads.items()}
    print("worst gradient tensor", max(worst.items(), key=lambda kv: kv[1]))
    bad = {k: v for k, v in worst.items() if v >= GREL}
    assert not bad, bad
    step.close()


def check_ones_equals_plain(device, name, precision=None, exact=True):
    """All-ones tables against the plain step on the same noise: the loss to 1e-4, the gradients equal (``exact``) or, where the
    plain step is not itself bitwise run to run, within the difference of two plain runs."""
    B = A.CASES[name][1]
    s0, l0, p0, r0, g0 = engine_run(device, name, tables=False, precision=precision)
    ones = torch.ones(B, 3 if A.CASES[name][0] else 2)
    s1, l1, p1, r1, g1 = engine_run(device, name, kl="sample", tables=False, precision=precision, available=ones, target_available=ones)
    assert r0 is None and r1 is not None
    assert l1 == pytest.approx(l0, rel=REL)
    np.testing.assert_allclose(p1.cpu().numpy(), p0.cpu().numpy(), rtol=REL)
    if exact:
        for k in g0:
            assert torch.equal(g1[k], g0[k]), k
    worst = max(rel_l2(g1[k], g0[k]) for k in g0)
    s0.close(), s1.close()
    return worst


def column_grads(device, name, column, which, precision=None):
    """Parameter gradients with one column of the ``which`` ("input" / "target") table set to zero."""
    use_pose, B, *_, tin, ttg = A.case(name)
    tin, ttg = tin.clone(), ttg.clone()
    (tin if which == "input" else ttg)[:, column] = 0
    step, _, _, _, grads = engine_run(device, name, "sample", A.weights(B), tables=False, precision=precision, available=tin,
                                      target_available=ttg)
    step.close()
    return grads


PREFIX = {"input": ["visual_encoder.", "tactile_encoder.", "pose_encoder."],
          "target": ["visual_decoder.", "tactile_decoder.", "pose_decoder."]}


def check_zero_column(device, name, column, which, precision=None):
    grads = column_grads(device, name, column, which, precision)
    pre = PREFIX[which][column]
    hit = [k for k in grads if k.startswith(pre)]
    assert hit
    for k in hit:
        assert float(grads[k].abs().max()) == 0.0, k
    others = [k for k in grads if not k.startswith(pre)]
    assert any(float(grads[k].abs().max()) > 0 for k in others)


# ---- the tests (CPU, emulation backend) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kl", ["batch", "sample"])
@pytest.mark.parametrize("name", ["pose", "nopose"])
def test_engine_vs_yardstick(name, kl, weighted):
    check_engine_vs_yardstick("cpu", name, kl, weighted)


@pytest.mark.parametrize("name", ["pose", "nopose"])
def test_all_ones_tables_equal_the_plain_step(name):
    check_ones_equals_plain("cpu", name)


@pytest.mark.parametrize("which,column", [("target", 0), ("target", 1), ("target", 2), ("input", 0), ("input", 1), ("input", 2)])
def test_zero_column_gives_exact_zero_gradients(which, column):
    check_zero_column("cpu", "pose", column, which)


def test_nan_weight_of_an_absent_term_reaches_nothing():
    """w_b = NaN in a row that holds no target at all (the term weights are selections) would still reach the KL: so the row's weight
    is finite and the NaN sits where only a product with the table would find it -- in the TABLE entries of an absent target."""
    name = "pose"
    B = A.CASES[name][1]
    ops.set_backend(EmuBackendAvailTrain())
    tab = torch.full((2, B), float("nan"), dtype=torch.float64)
    tab2 = tab.clone()
    tav = torch.zeros(B, 4, dtype=torch.uint8)
    loss, out = torch.zeros(1), torch.zeros(B)
    ops.B.elbo_assemble_avail_weighted(tab, tab2, None, None, None, torch.ones(B), tav, loss, None, out, None, None, None, None, 2, B,
                                       1.0, 1.0)
    assert float(loss) == 0.0 and float(out.abs().max()) == 0.0 and float(tab.abs().max()) == 0.0 and float(tab2.abs().max()) == 0.0
    wt = torch.empty(3, B)
    w = torch.full((B,), float("nan"))
    ops.B.term_weights(tav, w, wt, B)
    assert float(wt.abs().max()) == 0.0


def test_eval_step_equals_forward_without_train():
    name = "pose"
    use_pose, B, inputs, targets, eps, masks, mask, tin, ttg = A.case(name)
    s0, l0, p0, r0, _ = engine_run("cpu", name, "sample", train=False)
    m = TM.build("cnn-mvae", True, use_pose, "cpu")
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    step = MVAEStep(m, pose_multiplier=A.POSE_MULTIPLIER, noise=InjectedNoise(eps, masks))
    loss = float(step.eval_step(inputs, targets, A.KL_WEIGHT, kl="sample", available=tin, target_available=ttg))
    assert loss == l0
    assert step.ctx is None
    for k, p in m.named_parameters():
        assert torch.equal(before[k], p.detach()), k
    _, loss_y, _, rows_y = A.yardstick(name, "sample")
    assert loss == pytest.approx(float(loss_y.detach()), rel=REL)
    np.testing.assert_allclose(step.last_rows["rows"].numpy(), rows_y.detach().numpy(), rtol=REL)
    s0.close(), step.close()


def mixed_loader(seq_length, n_seq=2, seed=5):
    """One synthetic loader batch whose availability table is replaced by a fixed mixed one (both, tactile, visual, nothing, ...)."""
    data, target = list(SyntheticVisuoTactile(1, n_seq, seq_length, seed=seed))[0]
    pattern = torch.tensor([[1., 1.], [0., 1.], [1., 0.], [0., 0.]])
    data[3] = pattern.repeat(data[3].shape[0] // 4 + 1, 1)[1:data[3].shape[0] + 1].contiguous()
    return data, target


def test_synthetic_loader_draws_a_seeded_mixed_table():
    ones = list(SyntheticVisuoTactile(1, 16, 1, seed=5))[0]
    a, b = (list(SyntheticVisuoTactile(1, 16, 1, seed=5, absent=0.35))[0] for _ in range(2))
    assert torch.equal(ones[0][3], torch.ones(16, 2))
    assert torch.equal(a[0][3], b[0][3]) and 0 < float(a[0][3].sum()) < 32
    for x, y in zip(ones[0][:3] + ones[1], a[0][:3] + a[1]):
        assert torch.equal(x, y)             # every other tensor is what it was


def present_means(step, target_available):
    """The performance measures recomputed from the fused step's per-term tables: the single-modality passes (1: visual, 2: tactile,
    6: pose), means over the rows whose TARGET is present."""
    from mmdyn_hip.models.functional import availability_table
    lr = step.last_rows
    B = lr["rows"].shape[0]
    tgt = availability_table(target_available, B, "cpu") != 0
    npx = step.last['recon_x'][0][0].numel()
    out = {}
    for key, tab, p, col, per in (("visual", "bce_v_rows", 1, 0, npx), ("tactile", "bce_t_rows", 2, 1, npx), ("pose", "mse_rows", 6, 2, 7)):
        rows = lr[tab][p].cpu()
        out[key] = float(rows[tgt[:, col]].sum()) / (max(int(tgt[:, col].sum()), 1) * per)
    return out


@pytest.mark.parametrize("cls,l", [(SeqModeling, 1), (DynModeling, 3)])
def test_problem_layer_fused_against_module_path(cls, l):
    data, target = mixed_loader(l)
    res = {}
    for fused in (True, False):
        prob = cls(TM.args(use_availability=True, no_cuda=True, problem_type="dyn_modeling" if cls is DynModeling else "seq_modeling"),
                   log_dir=TM.LOG_DIR, seq_length=l, fused=fused)
        assert (prob._step is not None) == fused
        prob.model.load_state_dict(seeded_state_dict(prob.model.state_dict(), 0))
        prob._kl_weight = A.KL_WEIGHT
        inputs, targets = prob.parse_input(data, target)
        kw = prob._avail_kw(inputs)
        assert set(kw) == {"available", "target_available"}
        B = inputs['model_input'][0].shape[0]
        eps, masks = A.seeded_noise(B, 256, 7, 8, 99)
        if fused:
            prob._step.noise = InjectedNoise(eps, masks)
            loss = prob._step.eval_step(*prob._fused_io(inputs, targets), prob._kl_weight, kl="sample", **kw)
            res[fused] = (float(loss), prob._fused_perf_present(), present_means(prob._step, kw["target_available"]))
            prob._step.close()
        else:
            prob.model.noise = InjectedNoise(eps, masks)
            with torch.no_grad():
                outputs, loss = prob._evaluate_model(inputs, targets)
            res[fused] = (float(loss), outputs['perf_measure'])
    print("fused", res[True], "module", res[False])
    assert res[True][0] == pytest.approx(res[False][0], rel=REL)
    for k, v in res[True][2].items():
        assert res[True][1][k] == pytest.approx(v, rel=1e-6), k
        assert res[False][1][k] == pytest.approx(v, rel=REL), k
    # the target table: the final target frame of a sequence and the pose always count; DynModeling rolls the input column
    has = data[3]
    want = torch.ones(has.shape[0] // l if cls is SeqModeling else has.shape[0], 3)
    if cls is DynModeling:
        want[:, :2] = torch.roll(has, -1, dims=0)
        want[l - 1::l, :2] = 1
    assert torch.equal(kw["target_available"].cpu().float(), want)
    assert not torch.equal(kw["target_available"].cpu().float()[:, :2], kw["available"].cpu().float())


def test_flag_off_passes_no_tables():
    from mmdyn_hip.main import build_parser
    base = ["--problem-type", "seq_modeling", "--model-name", "cnn-mvae", "--input-type", "visuotactile", "--use-pose", "--no-cuda"]
    ns = build_parser().parse_args(base)
    assert ns.use_availability is False and ns.synthetic_absent == 0.0
    ns = build_parser().parse_args(base + ["--use-availability", "--synthetic-absent", "0.3"])
    assert ns.use_availability is True and ns.synthetic_absent == 0.3
    prob = SeqModeling(TM.args(no_cuda=True), log_dir=TM.LOG_DIR, fused=True)
    inputs, _ = prob.parse_input(*mixed_loader(1))
    assert prob._avail_kw(inputs) == {}
    prob._step.close()


def test_module_path_gradients_follow_the_tables():
    """--reference-schedule with --use-availability: one optimiser step of the module path on a batch whose tactile TARGETS are all
    absent leaves the tactile decoder where it was and moves the rest."""
    data, target = mixed_loader(3)
    prob = DynModeling(TM.args(use_availability=True, no_cuda=True, problem_type="dyn_modeling"), log_dir=TM.LOG_DIR, seq_length=3,
                       fused=False)
    inputs, targets = prob.parse_input(data, target)
    kw = prob._avail_kw(inputs)
    kw["target_available"][:, 1] = 0
    before = {k: p.detach().clone() for k, p in prob.model.named_parameters()}
    _, loss = prob._evaluate_mvae(prob._fused_io(inputs, targets)[0], prob._fused_io(inputs, targets)[1], **kw)
    loss.backward()
    grads = {k: p.grad for k, p in prob.model.named_parameters()}
    assert all(float(g.abs().max()) == 0.0 for k, g in grads.items() if k.startswith("tactile_decoder."))
    assert all(float(g.abs().max()) > 0.0 for k, g in grads.items() if k.startswith("visual_decoder.") and k.endswith("weight"))
    assert len(before) == len(grads)


def test_train_epoch_with_availability_runs_and_reports_present_means():
    loader = SyntheticVisuoTactile(2, 2, 1, seed=5, absent=0.35)
    prob = SeqModeling(TM.args(use_availability=True, no_cuda=True), log_dir=TM.LOG_DIR, train_loader=loader, test_loader=loader,
                       fused=True)
    rec = Recorder(ops.B)
    old = ops.set_backend(rec)
    try:
        perf = prob._train_epoch(0)
        val = prob._test_epoch(0)
    finally:
        ops.set_backend(old)
    assert "poe_bwd_avail_weighted" in rec.ops and "poe_bwd" not in rec.ops
    assert set(perf) == {"visual", "tactile", "pose"} and all(np.isfinite(v) and v > 0 for v in perf.values())
    assert set(val) == {"visual", "tactile", "pose"} and all(np.isfinite(v) and v > 0 for v in val.values())
    prob._step.close()


def recorded_step(name, **kw):
    use_pose, B, inputs, targets, eps, masks, mask, tin, ttg = A.case(name)
    m = TM.build("cnn-mvae", True, use_pose, "cpu")
    step = MVAEStep(m, pose_multiplier=A.POSE_MULTIPLIER, noise=InjectedNoise(eps, masks))
    rec = Recorder(ops.B)
    old = ops.set_backend(rec)
    try:
        step.train_step(inputs, targets, A.KL_WEIGHT, loss_mask=mask, **kw)
    finally:
        ops.set_backend(old)
    step.close()
    return rec.ops


@pytest.mark.parametrize("name", ["pose", "nopose"])
def test_call_count_is_the_weighted_step_plus_one(name):
    use_pose, B, *_, tin, ttg = A.case(name)
    plain = recorded_step(name)
    assert recorded_step(name, available=None, target_available=None) == plain
    assert not any("avail" in op or "weighted" in op or op == "term_weights" for op in plain)
    weighted = recorded_step(name, sample_weight=A.weights(B), kl="sample")
    for kw in (dict(available=tin, target_available=ttg), dict(target_available=ttg, sample_weight=A.weights(B))):
        mixed = recorded_step(name, kl="sample", **kw)
        assert len(mixed) == len(weighted) + 1
        swap = {"poe_fwd": "poe_fwd_avail", "poe_bwd_weighted": "poe_bwd_avail_weighted",
                "elbo_assemble_weighted": "elbo_assemble_avail_weighted"}
        rest = list(mixed)
        rest.remove("term_weights")
        assert rest == [swap.get(op, op) for op in weighted]


def test_validation_errors_fire_before_any_backend_call():
    use_pose, B, inputs, targets, eps, masks, mask, tin, ttg = A.case("nopose")
    m = TM.build("cnn-mvae", True, False, "cpu")
    step = MVAEStep(m)
    rec = Recorder(ops.B)
    old = ops.set_backend(rec)
    try:
        for call in (step.forward, step.train_step, step.eval_step):
            with pytest.raises(ValueError):
                call(inputs, targets, 1.0, available=torch.ones(B + 1, 2))
            with pytest.raises(ValueError):
                call(inputs, targets, 1.0, available=torch.ones(B, 4))
            with pytest.raises(ValueError):
                call(inputs, targets, 1.0, target_available=torch.ones(B))
            with pytest.raises(ValueError):
                call(inputs, targets, 1.0, available=torch.ones(B, 2, dtype=torch.complex64))
            with pytest.raises(ValueError):
                call(inputs, targets, 1.0, available=tin, kl="mean")
        with pytest.raises(ValueError):
            step.forward(inputs, targets, 1.0, train=False, rows=True, available=tin)
        step.pg = object()               # a process group: data-parallel training with tables is not built
        with pytest.raises(ValueError, match="not built"):
            step.train_step(inputs, targets, 1.0, available=tin)
        with pytest.raises(ValueError, match="not built"):
            step.train_step(inputs, targets, 1.0, target_available=ttg)
        step.pg = None
        assert rec.ops == []
    finally:
        ops.set_backend(old)
    # a backend from before the new ops: an error that names the op, before anything is launched
    from emu_backend_refine import EmuBackendRefine
    rec = Recorder(EmuBackendRefine())
    old = ops.set_backend(rec)
    try:
        with pytest.raises(RuntimeError, match="has no op"):
            step.train_step(inputs, targets, 1.0, available=tin)
        assert rec.ops == []
    finally:
        ops.set_backend(old)
    step.close()


def test_tables_of_any_numeric_dtype_give_the_same_step():
    name = "nopose"
    _, B, *_, tin, ttg = A.case(name)
    base = engine_run("cpu", name, "sample", backward=False)
    for dt, scale in ((torch.bool, 1), (torch.int64, 7), (torch.float64, -2.5)):
        cast = lambda t: (t * scale).to(dt) if dt is not torch.bool else t != 0
        got = engine_run("cpu", name, "sample", tables=False, available=cast(tin), target_available=cast(ttg), backward=False)
        assert got[1] == base[1]
        got[0].close()
    base[0].close()
