"""The train step with the plane-row forms of the 3-channel layers' kernel (layers.CONV1_PLANES, layers.OUT3_RECOMPUTE) against
the same step with both switches off: two eager fp32x3 steps at batch 128 from the same state, batch and noise must leave the
same bits everywhere -- loss, the 7 partial ELBOs, every parameter and Adam moment, every BatchNorm buffer.  A recording proxy
around the backend shows that the "on" run went through the new launches (and never split the encoders' 32-channel activation
in a launch of its own), so the comparison cannot pass by exercising nothing."""
import pytest
import torch

from mmdyn_hip import engine, layers, ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import NoiseSource
from mmdyn_hip.ops import CONV, IM2COL3
from mmdyn_hip.utils.seeded_init import seeded_batch
import test_model_emu as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 128
NEW_OPS = ("conv3_fwd_planes", "conv3_dgrad_bn_stats", "conv3_dgrad_bn_apply_planes")


class Recording:
    """Forwards everything to the wrapped backend (attribute writes included) and notes the name and arguments of every call."""

    def __init__(self, inner):
        object.__setattr__(self, "_inner", inner)
        object.__setattr__(self, "calls", [])

    def __getattr__(self, attr):
        fn = getattr(self._inner, attr)
        if not callable(fn):
            return fn

        def wrapped(*a, **k):
            self.calls.append((attr, a))
            return fn(*a, **k)
        return wrapped

    def __setattr__(self, attr, value):
        setattr(self._inner, attr, value)

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)

    def a1_splits(self):
        """stand-alone splits of an encoder's first activation: [B * 32 * 32][32]"""
        return sum(1 for n, a in self.calls if n == "split_planes" and a[1].C == 32 and a[1].rows == B * 1024)

    def dgrad3(self):
        """du-writing input-gradient launches of the last decoder layer"""
        return sum(1 for n, a in self.calls if n == "igemm_nt_dgrad_bn" and a[9] == IM2COL3)


def run(on, monkeypatch):
    monkeypatch.setattr(layers, "CONV1_PLANES", on)
    monkeypatch.setattr(layers, "OUT3_RECOMPUTE", on)
    rec = Recording(ops.B)
    old = ops.set_backend(rec)
    try:
        m = T.build("cnn-mvae", True, True, DEV)
        step = MVAEStep(m, noise=NoiseSource(11), precision="fp32x3")
        inputs, targets = seeded_batch(B, 5)
        gi, gt = [x.to(DEV) for x in inputs], [x.to(DEV) for x in targets]
        out = []
        for _ in range(2):
            loss = step.train_step(gi, gt, 0.02)
            out.append((loss.detach().clone().reshape(-1), step.partials[:7].clone()))
        torch.cuda.synchronize()
        # the consumers of both routes take plane operands at this batch (the decoders' 4 groups, the encoders' one)
        prev = engine._select_precision("fp32x3")
        try:
            assert layers.planes_served(CONV, 4, B, 32, 32, 16, 64) and layers.planes_served(CONV, 1, B, 32, 32, 16, 64)
        finally:
            engine._restore_precision(prev)
        state = dict(params=step.params.flat.clone(), adam_m=step.adam_m.clone(), adam_v=step.adam_v.clone())
        for k, b in m.named_buffers():
            state["buffer " + k] = b.detach().clone()
        step.close()
    finally:
        ops.set_backend(old)
    return out, state, rec


def test_two_steps_equal_with_the_switches_on_and_off(monkeypatch):
    on, s_on, r_on = run(True, monkeypatch)
    off, s_off, r_off = run(False, monkeypatch)
    # what ran: every first-layer forward and every last-layer input gradient of the "off" run has its new launch in the "on" run
    assert r_off.a1_splits() > 0 and r_off.dgrad3() > 0 and all(r_off.count(n) == 0 for n in NEW_OPS)
    assert r_on.count("conv3_fwd_planes") == r_off.a1_splits() and r_on.a1_splits() == 0
    assert r_on.count("conv3_dgrad_bn_stats") == r_on.count("conv3_dgrad_bn_apply_planes") == r_off.dgrad3() and r_on.dgrad3() == 0
    for s, ((l1, p1), (l0, p0)) in enumerate(zip(on, off)):
        assert torch.isfinite(l1).all()
        assert torch.equal(l1, l0), (s, float(l1), float(l0))
        assert torch.equal(p1, p0), (s, p1.tolist(), p0.tolist())
    assert set(s_on) == set(s_off) and any(k.startswith("buffer ") for k in s_on)
    for k in s_on:
        assert torch.equal(s_on[k], s_off[k]), (k, float((s_on[k].double() - s_off[k].double()).abs().max()))
