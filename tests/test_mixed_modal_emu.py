"""Mixed-modality batches on the CPU: the per-row availability through the module API, the serving engine (forward / score /
complete) and the problem layer, on the emulation backend (tests/emu_backend_avail.py), against tests/golden/mixed_modal.npz -- the
reference's own whole-batch results of every modality subset on the seeded case of tests/avail_cases.py, row b taken from the run of
row b's subset.  The ``check_*`` functions take the device: the GPU suite (tests/test_mixed_modal_gpu.py) runs them on the HIP
library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import avail_cases as A
from emu_backend_avail import EmuBackendAvail
from mmdyn_hip import ops
from mmdyn_hip._lib import MmdynError
from mmdyn_hip.engine import MVAEInference
from mmdyn_hip.models import setup_model, InjectedNoise
from mmdyn_hip.models import functional as Fn
from mmdyn_hip.problems.problems import Reconstruction, SeqModeling
from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats
from test_conditions_emu import OUT_TOL, SUM_TOL, REL          # the tolerances that file applies to the same quantities
from test_oracle_golden import summarize, close_summary, load


@pytest.fixture(autouse=True)
def emu_avail():
    old = ops.set_backend(EmuBackendAvail())
    yield
    ops.set_backend(old)


def build(categorical, device="cpu"):
    m = setup_model("cnn-mvae", cross_modal=True, **A.model_kw(categorical))
    m.load_state_dict(seeded_running_stats(seeded_state_dict(m.state_dict(), 0)))
    return m.to(device).eval()


def serving(categorical, device, **kw):
    m = build(categorical, device)
    return m, MVAEInference(m, **kw)


def case_on(categorical, device, blank=None):
    """The case's tensors on the device.  ``blank``: a value written into the rows of every modality the row does NOT hold."""
    inputs, eps, cond = A.case(categorical)
    inputs = [t.clone() for t in inputs]
    if blank is not None:
        for m in range(3):
            for b, s in enumerate(A.row_subsets()):
                if not s[m]:
                    inputs[m][b] = blank
    return [t.to(device) for t in inputs], eps, None if cond is None else cond.to(device)


def against_fixture(out, g, tag, who):
    v, t, p, mu, lv = out
    np.testing.assert_allclose(mu.cpu().numpy(), g[f"{tag}/means"], **OUT_TOL, err_msg=who)
    np.testing.assert_allclose(lv.cpu().numpy(), g[f"{tag}/log_var"], **OUT_TOL, err_msg=who)
    np.testing.assert_allclose(p.cpu().numpy(), g[f"{tag}/pose"], **OUT_TOL, err_msg=who)
    for b in range(A.BATCH):
        close_summary(summarize(v[b].cpu(), 256), g[f"{tag}/visual"][b], SUM_TOL, f"{who} visual row {b}")
        close_summary(summarize(t[b].cpu(), 256), g[f"{tag}/tactile"][b], SUM_TOL, f"{who} tactile row {b}")


def check_fixture(golden_dir, device, categorical, precision="fp32x3"):
    """1. MVAE.forward(available=) in eval() and MVAEInference.forward(available=) against the reference's per-subset runs; the
    rows of an absent modality hold a constant the reference never saw."""
    g = load(golden_dir, "mixed_modal.npz")
    assert g["row_subset"].tolist() == [list(s) for s in A.row_subsets()]
    tag = "cat" if categorical else "plain"
    inputs, eps, cond = case_on(categorical, device, blank=0.25)
    m, eng = serving(categorical, device, precision=precision)
    eng.use_graph = False                                   # injected noise: compare with the reference's vectors
    av = A.available(3).to(device)
    m.noise = InjectedNoise([eps.clone()], [])
    with torch.no_grad():
        against_fixture(m([inputs[0], inputs[1]], pose=inputs[2], condition=cond, available=av), g, tag, "module")
    eng.noise = InjectedNoise([eps.clone()], [])
    against_fixture(eng.forward([inputs[0], inputs[1]], pose=inputs[2], condition=cond, available=av), g, tag, "engine")
    return m, eng


def check_row_equivalence(device, categorical=False):
    """2. Every row of the mixed result equals, exactly, the row of the engine's own whole-batch forward of that row's subset."""
    inputs, eps, cond = case_on(categorical, device)
    m, eng = serving(categorical, device)
    eng.use_graph = False
    eng.noise = InjectedNoise([eps.clone()], [])
    mixed = [o.clone() for o in eng.forward([inputs[0], inputs[1]], pose=inputs[2], condition=cond, available=A.available(3))]
    for s in sorted(set(A.SUBSETS)):
        eng.noise = InjectedNoise([eps.clone()], [])
        whole = eng.forward([inputs[0] if s[0] else None, inputs[1] if s[1] else None], pose=inputs[2] if s[2] else None,
                            condition=cond)
        for b, sb in enumerate(A.row_subsets()):
            if sb == s:
                for a, w in zip(mixed, whole):
                    assert torch.equal(a[b], w[b]), (s, b)


def poe_formula(heads, on, eps_noise, L):
    """The product of experts of the emulation, restated here for torch autograd in fp64: prior first, then each present expert,
    eps added twice, an absent (row, expert) selected out."""
    e = 1e-8
    B = on.shape[0]
    sumT = torch.ones(B, L, dtype=torch.float64) / ((1.0 + e) + e)
    sumMuT = torch.zeros(B, L, dtype=torch.float64)
    for m, h in enumerate(heads):
        if h is None:
            continue
        T = 1.0 / ((torch.exp(h[:, L:]) + e) + e)
        row = on[:, m:m + 1]
        sumT = torch.where(row, sumT + T, sumT)
        sumMuT = torch.where(row, sumMuT + h[:, :L] * T, sumMuT)
    mu = sumMuT / sumT
    lv = torch.log(1.0 / sumT + e)
    return mu, lv, eps_noise * torch.exp(0.5 * lv) + mu


def check_backward(device):
    """3. The differentiable path (models.functional.PoEReparamAvailFn, what MVAE.forward(available=) calls): head gradients
    against torch autograd on the formula above in fp64.  Bound: the kernel's chain is ~30 fp32 roundings (2^-24 each) through
    sums whose terms cancel, so an element may be off by that many ulps of the LARGEST gradient of its tensor: 1e-4 of the
    tensor's maximum, the relative bound the suite puts on outputs (OUT_TOL's rtol).  Absent pairs are exactly 0."""
    L, B = 64, A.BATCH
    gen = torch.Generator().manual_seed(5)
    on = A.available(3, torch.bool)
    table = Fn.availability_table(on, B, device)
    heads = [(0.5 * torch.randn(B, 2 * L, generator=gen)) for _ in range(3)]
    eps_noise = torch.randn(B, L, generator=gen)
    w = [torch.randn(B, L, generator=gen) for _ in range(3)]
    hd = [h.clone().to(device).requires_grad_(True) for h in heads]
    mu, lv, z = Fn.PoEReparamAvailFn.apply(eps_noise.to(device), L, table, *hd)
    (mu * w[0].to(device)).sum().add((lv * w[1].to(device)).sum()).add((z * w[2].to(device)).sum()).backward()
    h64 = [h.double().requires_grad_(True) for h in heads]
    mu64, lv64, z64 = poe_formula(h64, on, eps_noise.double(), L)
    ((mu64 * w[0]).sum() + (lv64 * w[1]).sum() + (z64 * w[2]).sum()).backward()
    np.testing.assert_allclose(mu.detach().cpu().numpy(), mu64.detach().numpy(), rtol=1e-5, atol=1e-6)
    for m in range(3):
        got, want = hd[m].grad.cpu(), h64[m].grad
        bound = 1e-4 * float(want.abs().max())
        print("expert", m, "largest gradient deviation", float((got.double() - want).abs().max()), "bound", bound)
        assert float((got.double() - want).abs().max()) <= bound
        for b in range(B):
            if not on[b, m]:
                assert torch.equal(got[b], torch.zeros(2 * L)), (m, b)
            else:
                assert float(got[b].abs().max()) > 0


def check_module_backward(device):
    """3b. MVAE.forward(available=) in train() mode is differentiable end to end: finite gradients everywhere, and the encoders'
    heads get none from a batch whose rows all lack that modality."""
    m = setup_model("cnn-mvae", cross_modal=True, **A.model_kw(False))
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    m.to(device).train()
    inputs, eps, _ = case_on(False, device)
    av = A.available(3)
    av[:, 1] = 0                                            # no row holds the tactile image
    masks = [torch.ones(A.BATCH, 512, dtype=torch.uint8)] * 2
    m.noise = InjectedNoise([eps.clone()], masks)
    v, t, p, mu, lv = m([inputs[0], inputs[1]], pose=inputs[2], available=av)
    (v.sum() + t.sum() + p.sum() + (mu * lv).sum()).backward()
    for k, p_ in m.named_parameters():
        assert p_.grad is not None and torch.isfinite(p_.grad).all(), k
    assert float(m.tactile_encoder.linear_means.weight.grad.abs().max()) == 0.0
    assert float(m.visual_encoder.linear_means.weight.grad.abs().max()) > 0.0


def check_interface(device):
    """4. Prior-only row; [B, 2] vs [B, 3] tables; a None modality overrides the table; ValueError cases; a table together with
    with_prior = 0 is refused with the library's argument error."""
    inputs, eps, _ = case_on(False, device)
    m, eng = serving(False, device)
    eng.use_graph = False
    x, B, L = [inputs[0], inputs[1]], A.BATCH, A.LATENT
    # two runs are compared output by output on the emulation; on a device by the outputs the table reaches without passing
    # through a decoder (means, log_var) -- the decoders are not part of this feature and their repeatability is not claimed here
    same = lambda p_, q_: all(torch.equal(a_, b_) for a_, b_ in (zip(p_, q_) if str(device) == "cpu" else zip(p_[3:], q_[3:])))

    def fwd(x_, pose, av, who=eng):
        who.noise = InjectedNoise([eps.clone()], [])
        with torch.no_grad():
            return [o.clone() for o in who.forward(x_, pose=pose, available=av)] if who is eng else \
                [o.clone() for o in who(x_, pose=pose, available=av)]

    # a row that holds nothing is the prior alone: mu = 0, logvar = logf(1 / (1 / (1 + 2e-8)) + 1e-8), as the kernel evaluates it
    av = A.available(3)
    av[3] = 0
    one, e = torch.ones(1), 1e-8
    sumT = one / ((one + e) + e)
    want_lv = float(torch.log(1.0 / sumT + e))
    for who in (eng, m):
        out = fwd(x, inputs[2], av.to(device), who)
        assert torch.equal(out[3][3].cpu(), torch.zeros(L))
        assert torch.equal(out[4][3].cpu(), torch.full((L,), want_lv))
        assert all(torch.isfinite(o).all() for o in out)
    # [B, 2] = (visual, tactile) as the dataset yields it (float64): the pose counts as present in every row
    full = A.available(3)
    full[:, 2] = 1
    a2, a3 = fwd(x, inputs[2], A.available(2).to(device)), fwd(x, inputs[2], full.to(device))
    assert same(a2, a3)
    # any numeric dtype gives the same table
    for dt in (torch.bool, torch.uint8, torch.int32, torch.int64, torch.float32, torch.float16):
        assert torch.equal(Fn.availability_table(A.available(3, torch.float64).to(dt), B, device),
                           Fn.availability_table(A.available(3), B, device))
    assert torch.equal(Fn.availability_table(A.available(3) * -3.5, B, device), Fn.availability_table(A.available(3), B, device))
    # a modality passed as None is absent in every row whatever the table says
    no_v = A.available(3)
    no_v[:, 0] = 0
    for who in (eng, m):
        a = fwd([None, inputs[1]], inputs[2], A.available(3).to(device), who)
        b = fwd(x, inputs[2], no_v.to(device), who)
        assert same(a, b)
    # the table is data, never a None: all present == the whole-batch path
    ones = torch.ones(B, 3)
    eng.noise = InjectedNoise([eps.clone()], [])
    whole = [o.clone() for o in eng.forward(x, pose=inputs[2])]
    assert same(fwd(x, inputs[2], ones.to(device)), whole)
    # wrong shape or a non-numeric dtype
    for bad in (torch.ones(B, 4), torch.ones(B), torch.ones(B - 1, 3), torch.ones(B, 1), torch.ones(B, 3, dtype=torch.complex64)):
        for call in (lambda: eng.forward(x, pose=inputs[2], available=bad), lambda: m(x, pose=inputs[2], available=bad),
                     lambda: eng.score(x, pose=inputs[2], available=bad), lambda: eng.complete(x, pose=inputs[2], available=bad),
                     lambda: eng.score(x, pose=inputs[2], target_available=bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        eng.forward(x, pose=inputs[2], available=[["a", "b"]] * B)
    # the backend: a table of another shape / dtype, and a table without the prior
    table = Fn.availability_table(A.available(3), B, device)
    h = [torch.zeros(B, 2 * L, device=device) for _ in range(2)]
    p = {"mu": [t[:, :L] for t in h], "lv": [t[:, L:] for t in h], "dmu": [t[:, :L] for t in h], "dlv": [t[:, L:] for t in h],
         "ld": [2 * L] * 2}
    mu, lv = torch.zeros(B, L, device=device), torch.zeros(B, L, device=device)
    with pytest.raises(ValueError):
        ops.B.poe_fwd_avail([p], [table[:, :3].contiguous()], None, mu, lv, None, None, True, 1, B, L)
    with pytest.raises(ValueError):
        ops.B.poe_fwd_avail([p], [table.to(torch.int32)], None, mu, lv, None, None, True, 1, B, L)
    with pytest.raises(MmdynError, match="MMDYN_ERR"):
        ops.B.poe_fwd_avail([p], [table], None, mu, lv, None, None, False, 1, B, L)
    with pytest.raises(MmdynError, match="MMDYN_ERR"):
        ops.B.poe_bwd_avail([p], [table], None, mu, lv, None, mu, lv, 0.0, False, 1, B, L)
    ops.B.poe_fwd_avail([p], None, None, mu, lv, None, None, False, 1, B, L)           # no table: the prior-less form is served


def check_score(device, categorical=False):
    """5. score(available=): a row's ``rows`` entry is the sum of exactly its available terms, an excluded term's entry is 0, an
    included one is what the same request scores with every target present; kl is every row's own."""
    inputs, eps, cond = case_on(categorical, device, blank=0.25)
    m, eng = serving(categorical, device)
    eng.use_graph = False
    x, on = [inputs[0], inputs[1]], A.available(3, torch.bool)
    kw = dict(pose=inputs[2], condition=cond, kl_weight=A.KL_WEIGHT, pose_multiplier=A.POSE_MULTIPLIER)
    clone = lambda r: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}
    eng.noise = InjectedNoise([eps.clone()], [])
    res = clone(eng.score(x, available=A.available(3).to(device), **kw))
    eng.noise = InjectedNoise([eps.clone()], [])
    every = clone(eng.score(x, available=A.available(3).to(device), target_available=torch.ones(A.BATCH, 3), **kw))
    # (two runs of the row kernels: their fp64 block sums meet in atomics, so "the same" is the 1e-12 that
    #  tests/test_elbo_rows_gpu.py puts on such pairs, RTOL_SAME; the zeros below are exact)
    again = lambda a, b: np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-12)
    assert torch.equal(res["means"], every["means"])
    again(res["kl"], every["kl"])
    for m_, key in enumerate(("bce_visual", "bce_tactile", "mse_pose")):
        got, full = res[key].cpu(), every[key].cpu()
        again(got[on[:, m_]], full[on[:, m_]])
        assert float(full.min()) > 0
        assert torch.equal(got[~on[:, m_]], torch.zeros(int((~on[:, m_]).sum()), dtype=torch.float64))
    want = res["bce_visual"] + res["bce_tactile"] + A.POSE_MULTIPLIER * res["mse_pose"] + A.KL_WEIGHT * res["kl"]
    np.testing.assert_allclose(res["rows"].cpu().numpy(), want.cpu().numpy(), rtol=1e-6)           # (fp32 rounding of the sum)
    full_rows = every["bce_visual"] + every["bce_tactile"] + A.POSE_MULTIPLIER * every["mse_pose"] + A.KL_WEIGHT * every["kl"]
    np.testing.assert_allclose(every["rows"].cpu().numpy(), full_rows.cpu().numpy(), rtol=1e-6)
    # the terms themselves against fp64 on the pass's own outputs, at the bound tests/test_conditions_gpu.py holds them to
    v, t, p = [r.double().cpu() for r in res["recon_x"]]
    bv = F.binary_cross_entropy_with_logits(v, inputs[0].double().cpu(), reduction="none").sum((1, 2, 3))
    mse = ((p - inputs[2].double().cpu()) ** 2).sum(1)
    np.testing.assert_allclose(res["bce_visual"].cpu().numpy(), (bv * on[:, 0]).numpy(), rtol=1e-5)
    np.testing.assert_allclose(res["mse_pose"].cpu().numpy(), (mse * on[:, 2]).numpy(), rtol=1e-5)
    # explicit targets: every target counts unless target_available says otherwise
    eng.noise = InjectedNoise([eps.clone()], [])
    explicit = eng.score(x, targets=[inputs[0], inputs[1], inputs[2]], available=A.available(3).to(device), **kw)
    again(explicit["bce_visual"], every["bce_visual"])
    np.testing.assert_allclose(explicit["rows"].cpu().numpy(), every["rows"].cpu().numpy(), rtol=1e-6)


def check_complete(device, categorical=False, sigmoid_atol=0.0):
    """6. complete(): present rows are the inputs bit for bit; absent rows are sigmoid of the logits forward(available=) returns
    (which check_fixture pins to the reference), the pose decoder's output for the pose.  ``sigmoid_atol``: 0 where both sides
    are torch.sigmoid (the emulation); on the device see tests/test_mixed_modal_gpu.py."""
    inputs, eps, cond = case_on(categorical, device, blank=0.25)
    m, eng = serving(categorical, device)
    eng.use_graph = False
    x, on, av = [inputs[0], inputs[1]], A.available(3, torch.bool), A.available(3).to(device)
    for sample, noise in ((True, eps), (False, torch.zeros_like(eps))):
        eng.noise = InjectedNoise([eps.clone()], [])
        done = [o.clone() for o in eng.complete(x, pose=inputs[2], available=av, condition=cond, sample=sample)]
        eng.noise = InjectedNoise([noise.clone()], [])
        v, t, p, _, _ = eng.forward(x, pose=inputs[2], condition=cond, available=av)
        for m_, (got, src, fill) in enumerate(zip(done, inputs, (torch.sigmoid(v), torch.sigmoid(t), p))):
            rows = on[:, m_].to(got.device)
            assert torch.equal(got[rows], src[rows]), (sample, m_)
            if m_ == 2:
                assert torch.equal(got[~rows], fill[~rows])
            else:
                dev_ = float((got[~rows] - fill[~rows]).abs().max())
                print("sample" if sample else "mean", "modality", m_, "largest deviation from torch.sigmoid", dev_)
                assert dev_ <= sigmoid_atol
                assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    # a modality that is not given at all is reconstructed in every row; no table: everything given comes back
    eng.noise = InjectedNoise([eps.clone()], [])
    done = eng.complete([inputs[0], None], pose=inputs[2], available=av, condition=cond)
    assert not torch.equal(done[1], inputs[1]) and torch.equal(done[0][on[:, 0].to(done[0].device)], inputs[0][on[:, 0].to(done[0].device)])
    done = eng.complete(x, pose=inputs[2], condition=cond)
    assert all(torch.equal(a, b) for a, b in zip(done, inputs))


class CountAll:
    """Wraps the active backend and counts every op call by name."""

    def __init__(self, inner):
        self._inner, self.calls = inner, {}

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr) or name.startswith("_"):
            return attr

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return attr(*a, **k)
        return counted


def counted(fn):
    counting = CountAll(ops.B)
    old = ops.set_backend(counting)
    try:
        fn()
    finally:
        ops.set_backend(old)
    return counting.calls


def check_call_count(device, categorical=False):
    """7. The mixed request issues the backend calls of the joint request of the same shape, the PoE call replaced one for one;
    score likewise (the assembly is replaced by its sibling); complete adds one select per returned modality."""
    inputs, eps, cond = case_on(categorical, device)
    m, eng = serving(categorical, device)
    eng.use_graph = False
    x, av = [inputs[0], inputs[1]], A.available(3).to(device)
    joint = counted(lambda: eng.forward(x, pose=inputs[2], condition=cond))
    mixed = counted(lambda: eng.forward(x, pose=inputs[2], condition=cond, available=av))
    assert joint.pop("poe_fwd") == 1 and mixed.pop("poe_fwd_avail") == 1
    assert mixed == joint, (mixed, joint)
    assert sum(mixed.values()) > 10                          # (the wrapper really sees the launches)
    js = counted(lambda: eng.score(x, pose=inputs[2], condition=cond))
    ms = counted(lambda: eng.score(x, pose=inputs[2], condition=cond, available=av))
    assert js.pop("poe_fwd") == 1 and ms.pop("poe_fwd_avail") == 1
    assert js.pop("elbo_assemble_rows") == 1 and ms.pop("elbo_assemble_rows_avail") == 1
    assert ms == js, (ms, js)
    done = counted(lambda: eng.complete(x, pose=inputs[2], condition=cond, available=av, sample=True))
    assert done.pop("complete_select") == 3 and done.pop("poe_fwd_avail") == 1
    assert done == mixed
    mean = counted(lambda: eng.complete(x, pose=inputs[2], condition=cond, available=av))
    assert sum(mean.values()) < sum(done.values()) + 4       # the posterior mean draws no noise


def problem_of(m, model_name, conditional, device, cls=SeqModeling):
    prob = cls.__new__(cls)
    prob._model, prob._conditional, prob._device, prob._seq_length = m, conditional, torch.device(device), 1
    prob.parameters = {"use_pose": True, "model_name": model_name, "mask_loss": False, "input_type": "visuotactile"}
    return prob


def check_problem_layer(device, categorical=False):
    """8. Reconstruction.complete (inherited by SeqModeling) on the dict parse_input returns for a dataset batch
    [visual, tactile, pose, available_modals(, shock)]."""
    inputs, eps, cond = case_on(categorical, "cpu", blank=0.25)
    m = build(categorical, device)
    prob = problem_of(m, "cnn-mvae", categorical, device)
    data = [inputs[0], inputs[1], inputs[2], A.available(2)] + ([cond] if categorical else [])
    x, _ = prob.parse_input(data, [inputs[0], inputs[1], inputs[2], torch.ones(A.BATCH, 1, 64, 64)])
    assert x["input_available_modals"].dtype == torch.float64 and tuple(x["input_available_modals"].shape) == (A.BATCH, 2)
    v, t, p = prob.complete(x)
    on = A.available(2, torch.bool)
    for got, src, rows in ((v, inputs[0], on[:, 0]), (t, inputs[1], on[:, 1])):
        assert torch.equal(got.cpu()[rows], src[rows]) and not torch.equal(got.cpu()[~rows], src[~rows])
        assert torch.isfinite(got).all() and float(got.min()) >= 0 and float(got.max()) <= 1
    assert torch.equal(p.cpu(), inputs[2])                   # [B, 2]: the pose is present wherever it is given
    # the engine beside it gives the same completion
    eng = MVAEInference(m)
    eng.use_graph = False
    want = eng.complete([t_.to(device) for t_ in inputs[:2]], pose=inputs[2].to(device), available=A.available(2),
                        condition=None if cond is None else cond.to(device))
    np.testing.assert_allclose(want[0].cpu().numpy(), v.cpu().numpy(), **OUT_TOL)
    np.testing.assert_allclose(want[1].cpu().numpy(), t.cpu().numpy(), **OUT_TOL)
    with pytest.raises(ValueError, match="cnn-mvae"):
        problem_of(m, "cnn-vae", categorical, device, Reconstruction).complete(x)
    with pytest.raises(ValueError):
        prob.complete(inputs[0])


# ---- the CPU suite ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("categorical", [False, True], ids=["plain", "categorical"])
def test_fixture(golden_dir, categorical):
    check_fixture(golden_dir, "cpu", categorical)


def test_row_equivalence():
    check_row_equivalence("cpu")


def test_backward():
    check_backward("cpu")


def test_module_backward():
    check_module_backward("cpu")


def test_interface():
    check_interface("cpu")


@pytest.mark.parametrize("categorical", [False, True], ids=["plain", "categorical"])
def test_score(categorical):
    check_score("cpu", categorical)


@pytest.mark.parametrize("categorical", [False, True], ids=["plain", "categorical"])
def test_complete(categorical):
    check_complete("cpu", categorical)


def test_call_count():
    check_call_count("cpu")


@pytest.mark.parametrize("categorical", [False, True], ids=["plain", "categorical"])
def test_problem_layer(categorical):
    check_problem_layer("cpu", categorical)


def test_emulation_keeps_nan_out():
    """The emulation selects (torch.where), as the kernels do: NaN / Inf in the head words of an absent (row, expert) reach no
    output, forward or backward, and the absent gradient rows come back as zeros from a NaN-filled buffer."""
    B, L = A.BATCH, 32
    gen = torch.Generator().manual_seed(9)
    on = A.available(3, torch.bool)
    table = Fn.availability_table(on, B, "cpu")
    heads = [torch.randn(B, 2 * L, generator=gen) for _ in range(3)]
    dirty = [h.clone() for h in heads]
    for m in range(3):
        dirty[m][~on[:, m]] = float("nan") if m != 1 else float("inf")
    eps_noise = torch.randn(B, L, generator=gen)
    outs = []
    for hs in (heads, dirty):
        mu, lv, z = (torch.empty(B, L) for _ in range(3))
        ds = [torch.full_like(h, float("nan")) for h in hs]
        ops.B.poe_fwd_avail([Fn._pass(hs, None, L)], [table], eps_noise, mu, lv, z, None, True, 1, B, L)
        ops.B.poe_bwd_avail([Fn._pass(hs, ds, L)], [table], eps_noise, mu, lv, torch.ones(B, L), None, None, 0.1, True, 1, B, L)
        outs.append([mu, lv, z] + ds)
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    for m in range(3):
        assert torch.equal(outs[1][3 + m][~on[:, m]], torch.zeros(int((~on[:, m]).sum()), 2 * L))
