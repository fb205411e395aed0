"""Conditions end to end on a real MI355X: mmdyn_concat_condition through the C ABI, bit for bit against torch.cat + zero padding;
the checks of tests/test_conditions_emu.py on the HIP library (module API, fused engine eager and graph-replayed, per-sample
rows, serving engine) against tests/golden/conditions.npz; the serving engine's replay safety and its bad-index report.

No case is shape-skipped on an MI355X; nothing here reads anything but the repository tree."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cond_cases as C
import test_conditions_emu as TC
from mmdyn_hip import ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import InjectedNoise, NoiseSource
from test_oracle_golden import load

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = ops.B
GUARD = 256          # floats kept behind ``out``: they must come back untouched

SHAPES = [(1, 512, 3, 544), (256, 512, 5, 544), (37, 64, 5, 96), (130, 64, 1, 96), (5, 7, 2, 32)]


def reference_join(x, block, width):
    rows = x.shape[0]
    return torch.cat((x, block, torch.zeros(rows, width - x.shape[1] - block.shape[1])), dim=-1)


@pytest.mark.parametrize("source", ["float", "index"])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("rows,K,cd,width", SHAPES)
def test_concat_condition_abi(rows, K, cd, width, strided, source):
    """The entry point itself (ctypes, raw pointers): x dense or with a row stride larger than K, both condition sources, NaN
    planted in the destination beforehand (the padding is written), a guard region behind ``out`` untouched."""
    lib = HIP.lib
    g = torch.Generator().manual_seed(rows * 1000 + K + cd)
    ldx = K + (12 if K % 4 == 0 else 3) if strided else K
    xs = torch.randn(rows, ldx, generator=g)
    x = xs[:, :K]
    if source == "float":
        cond = torch.randn(rows, cd, generator=g)
        block, idx = cond, None
    else:
        idx = torch.randint(0, cd, (rows,), generator=g)
        block, cond = F.one_hot(idx, cd).float(), None
    want = reference_join(x, block, width)
    buf = torch.full((rows * width + GUARD,), float("nan"), device=DEV)
    buf[rows * width:] = 7.0
    xd = xs.to(DEV)
    cd_dev = None if cond is None else cond.to(DEV)
    idx_dev = None if idx is None else idx.to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = lib.mmdyn_concat_condition(xd.data_ptr(), None if cd_dev is None else cd_dev.data_ptr(),
                                    None if idx_dev is None else idx_dev.data_ptr(), buf.data_ptr(), bad.data_ptr(), rows, K, ldx,
                                    cd, width, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = buf[:rows * width].reshape(rows, width).cpu()
    assert torch.equal(got, want)                                  # bitwise (NaN anywhere would fail it)
    assert torch.equal(buf[rows * width:].cpu(), torch.full((GUARD,), 7.0))
    assert int(bad.item()) == 0
    # ... and through the backend method, as layers.concat_condition calls it
    out = torch.full((rows, width), float("nan"), device=DEV)
    HIP.concat_condition(xd[:, :K], cd_dev if idx is None else idx_dev, out, K, cd, None)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("rows,K,cd,width", SHAPES)
def test_concat_condition_bad_index(rows, K, cd, width):
    """An out-of-range index is ordinary input: that row's condition block is all zero, the flag is set, every other row is
    right and the guard region stays untouched; the flag word is nullable."""
    g = torch.Generator().manual_seed(77 + rows)
    x = torch.randn(rows, K, generator=g)
    idx = torch.randint(0, cd, (rows,), generator=g)
    bad_rows = sorted({0, rows // 2, rows - 1})
    for r, v in zip(bad_rows, (cd, -1, 2 ** 40)):
        idx[r] = v
    block = torch.zeros(rows, cd)
    ok = (idx >= 0) & (idx < cd)
    block[ok] = F.one_hot(idx[ok], cd).float()
    want = reference_join(x, block, width)
    for with_flag in (True, False):
        buf = torch.full((rows * width + GUARD,), float("nan"), device=DEV)
        buf[rows * width:] = 7.0
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        HIP.concat_condition(x.to(DEV), idx.to(DEV), buf[:rows * width].view(rows, width), K, cd, bad if with_flag else None)
        torch.cuda.synchronize()
        assert torch.equal(buf[:rows * width].reshape(rows, width).cpu(), want)
        assert torch.equal(buf[rows * width:].cpu(), torch.full((GUARD,), 7.0))
        assert int(bad.item()) == (1 if with_flag else 0)


def test_concat_condition_argument_errors():
    lib = HIP.lib
    x, c, i = torch.zeros(4, 64, device=DEV), torch.zeros(4, 3, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.zeros(4, 96, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda xp, cp, ip, op, *dims: lib.mmdyn_concat_condition(xp, cp, ip, op, None, *dims, st)
    assert call(x.data_ptr(), c.data_ptr(), i.data_ptr(), out.data_ptr(), 4, 64, 64, 3, 96) == -2      # both sources
    assert call(x.data_ptr(), None, None, out.data_ptr(), 4, 64, 64, 3, 96) == -2                      # neither
    assert call(None, c.data_ptr(), None, out.data_ptr(), 4, 64, 64, 3, 96) == -2
    assert call(x.data_ptr(), c.data_ptr(), None, None, 4, 64, 64, 3, 96) == -2
    assert call(x.data_ptr(), c.data_ptr(), None, out.data_ptr(), 4, 64, 64, 3, 80) == -1              # width % 32
    assert call(x.data_ptr(), c.data_ptr(), None, out.data_ptr(), 4, 64, 64, 40, 96) == -1             # K + cd > width
    assert call(x.data_ptr(), c.data_ptr(), None, out.data_ptr(), 4, 64, 60, 3, 96) == -1              # ldx < K
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                                               # nothing was launched


# ---- the model layers on the HIP library -------------------------------------------------------------------------------------
def test_module_train(golden_dir):
    TC.check_module_train(golden_dir, DEV)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_engine_train(golden_dir, precision):
    TC.check_engine_train(golden_dir, DEV, precision)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_engine_rows(golden_dir, precision):
    TC.check_engine_rows(golden_dir, DEV, precision)


def test_onehot_equivalence():
    TC.check_onehot_equivalence(DEV)


def test_categorical_vae(golden_dir):
    TC.check_vae(golden_dir, DEV)


def test_graphed_step_equals_eager():
    """train_step_graphed (the class indices are one more static input of the capture) == eager train_step, step for step, with
    a new condition every step -- losses and parameters at the bound of the existing graph-vs-eager test; then the engine's
    bad-index word reports a planted index through the replayed graphs and is clear after a good step."""
    from mmdyn_hip.utils.seeded_init import seeded_batch
    B, klw, steps = 8, 0.02, 4
    inputs, targets = seeded_batch(B, 93)
    gi, gt = [x.to(DEV) for x in inputs], [x.to(DEV) for x in targets]
    conds = [C.indices(B, 40 + s).to(DEV) for s in range(steps)]
    out = []
    for graphed in (False, True):
        m = TC.build("cnn-mvae", True, True, DEV).train()
        step = MVAEStep(m, noise=NoiseSource(94))
        run = step.train_step_graphed if graphed else step.train_step
        losses = [float(run(gi, gt, klw, condition=c)) for c in conds]
        torch.cuda.synchronize()
        out.append((losses, step.params.flat.clone()))
        if graphed:
            assert step._graph is not None          # really replayed from graphs
            assert not step.bad_condition()
            bad = conds[0].clone()
            bad[3] = C.CAT_DIM
            float(step.train_step_graphed(gi, gt, klw, condition=bad))
            assert step.bad_condition()
            with pytest.raises(ValueError):
                step.check_condition()
            float(step.train_step_graphed(gi, gt, klw, condition=conds[0]))
            assert not step.bad_condition()
        step.close()
    print("eager", out[0][0], "graphed", out[1][0])
    assert out[0][0] == pytest.approx(out[1][0], rel=1e-6)
    assert float((out[0][1] - out[1][1]).norm() / out[0][1].norm()) < 1e-6


# ---- the serving engine ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("categorical", [True, False], ids=["categorical", "real"])
def test_inference_engine(golden_dir, categorical):
    TC.check_inference_engine(golden_dir, DEV, categorical)


@pytest.mark.parametrize("categorical", [True, False], ids=["categorical", "real"])
def test_inference_score(golden_dir, categorical):
    """score(condition=): the outputs of the joint pass against the fixture, and its per-sample terms against the same terms
    computed here in fp64 from those outputs (1e-5: the bound tests/test_elbo_rows_gpu.py holds the row kernels to)."""
    g = load(golden_dir, "conditions.npz")
    tag = "b" if categorical else "c"
    inputs, eps, cond, z, cs = C.eval_case(categorical)
    inputs, cond = [t.to(DEV) for t in inputs], cond.to(DEV)
    m, eng = TC.serving(categorical, DEV)
    eng.use_graph = False
    eng.noise = InjectedNoise([eps["joint"].clone()], [])
    res = eng.score([inputs[0], inputs[1]], pose=inputs[2], condition=cond, kl_weight=C.KL_WEIGHT, pose_multiplier=C.POSE_MULTIPLIER)
    v, t, p = res["recon_x"]
    TC.close_summary(TC.summarize(v.cpu(), 256), g[f"{tag}/joint/visual"], TC.SUM_TOL, "visual")
    np.testing.assert_allclose(res["means"].cpu().numpy(), g[f"{tag}/joint/means"], **TC.OUT_TOL)
    np.testing.assert_allclose(res["log_var"].cpu().numpy(), g[f"{tag}/joint/log_var"], **TC.OUT_TOL)
    np.testing.assert_allclose(p.cpu().numpy(), g[f"{tag}/joint/pose"], **TC.OUT_TOL)
    # the row kernels against fp64 on the pass's own outputs (pinned to the fixture above at the engine's tolerance)
    mu, lv = res["means"].double().cpu(), res["log_var"].double().cpu()
    kl = (-0.5 * (1 + lv - mu.pow(2) - lv.exp())).sum(1)
    bv = F.binary_cross_entropy_with_logits(v.double().cpu(), inputs[0].double().cpu(), reduction="none").sum((1, 2, 3))
    bt = F.binary_cross_entropy_with_logits(t.double().cpu(), inputs[1].double().cpu(), reduction="none").sum((1, 2, 3))
    mse = ((p.double().cpu() - inputs[2].double().cpu()) ** 2).sum(1)
    np.testing.assert_allclose(res["bce_visual"].cpu().numpy(), bv.numpy(), rtol=1e-5)
    np.testing.assert_allclose(res["bce_tactile"].cpu().numpy(), bt.numpy(), rtol=1e-5)
    np.testing.assert_allclose(res["mse_pose"].cpu().numpy(), mse.numpy(), rtol=1e-5)
    np.testing.assert_allclose(res["kl"].cpu().numpy(), kl.numpy(), rtol=1e-5)
    want = bv + bt + C.POSE_MULTIPLIER * mse + C.KL_WEIGHT * kl
    np.testing.assert_allclose(res["rows"].cpu().numpy(), want.numpy(), rtol=TC.REL)
    with pytest.raises(ValueError):
        eng.score([inputs[0], inputs[1]], pose=inputs[2])


@pytest.mark.parametrize("categorical", [True, False], ids=["categorical", "real"])
def test_replay_safety(categorical):
    """Two different conditions of the same shape through ONE captured graph each equal the eager result; a third call with the
    first condition reproduces the first result bit for bit (means / log_var carry no noise; the reconstructions are compared
    through inference-free outputs)."""
    inputs, eps, cond, z, cs = C.eval_case(categorical)
    inputs = [t.to(DEV) for t in inputs]
    c0 = cond.to(DEV)
    c1 = ((c0 + 1) % C.CAT_DIM) if categorical else (1.0 - c0)
    m, eng = TC.serving(categorical, DEV, seed=5)
    _, eager = TC.serving(categorical, DEV, seed=5)
    eager.use_graph = False
    x = [inputs[0], inputs[1]]
    got = []
    for c in (c0, c1, c0):
        out = eng.forward(x, pose=inputs[2], condition=c.clone())
        got.append([o.clone() for o in out])
    assert len([k for k in eng._graphs if k[0] == "fwd"]) == 1                 # one capture served all three
    for c, o in zip((c0, c1), got):
        want = eager.forward(x, pose=inputs[2], condition=c)
        assert torch.equal(o[3], want[3]) and torch.equal(o[4], want[4])       # means / log_var: no randomness
    assert not torch.equal(got[0][3], got[1][3])                               # the condition matters
    assert torch.equal(got[2][3], got[0][3]) and torch.equal(got[2][4], got[0][4])
    # the reconstructions, noise injected: the decoders' join too replays with the condition of the request
    zz = z.to(DEV)
    outs = []
    for c in (c0, c1, c0):
        eng.noise = InjectedNoise([zz.clone()] * 2, [])
        eng.use_graph = False
        outs.append([o.clone() for o in eng.inference(C.SAMPLE_N, c)])
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1]) and not torch.equal(outs[0][0], outs[1][0])
    # ... and the captured sampler: same condition shape, different conditions, one graph
    eng.use_graph, eng.noise = True, NoiseSource(5)
    a = eng.inference(C.SAMPLE_N, c0)[0].clone()
    b = eng.inference(C.SAMPLE_N, c1)[0].clone()
    assert len([k for k in eng._graphs if k[0] == "sample"]) == 1 and not torch.equal(a, b)
    eng.close()


def test_bad_condition_report():
    """bad_condition() reports a planted out-of-range index through a captured graph and is clear after a good request."""
    inputs, eps, cond, z, cs = C.eval_case(True)
    inputs, cond = [t.to(DEV) for t in inputs], cond.to(DEV)
    m, eng = TC.serving(True, DEV, seed=1)
    x = [inputs[0], inputs[1]]
    good = [o.clone() for o in eng.forward(x, pose=inputs[2], condition=cond)]
    assert not eng.bad_condition()
    bad = cond.clone()
    bad[1] = C.CAT_DIM + 3
    out = eng.forward(x, pose=inputs[2], condition=bad)
    assert eng.bad_condition()
    assert torch.isfinite(out[3]).all() and torch.equal(out[3][0], good[3][0]) and not torch.equal(out[3][1], good[3][1])
    out = eng.forward(x, pose=inputs[2], condition=cond)
    assert not eng.bad_condition() and torch.equal(out[3], good[3])
    eng.close()
