"""The switches of the 3-channel layers' plane-row launches (layers.CONV1_PLANES, layers.OUT3_RECOMPUTE) under the CPU emulation
backend: it has neither the new ops nor the plane query, so with the switches on the step must issue exactly the launches it issues
with them off -- one train step gives the same bits either way.  Guards the ``getattr(ops.B, ..., None)`` gate of the two routes."""
import pytest
import torch

from mmdyn_hip import layers, ops
from mmdyn_hip.engine import MVAEStep
from mmdyn_hip.models import InjectedNoise
from mmdyn_hip.utils.seeded_init import seeded_batch, seeded_noise
from emu_backend import EmuBackend
import test_model_emu as T

NEW_OPS = ("conv3_fwd_planes", "conv3_dgrad_bn_stats", "conv3_dgrad_bn_apply_planes")


@pytest.fixture(autouse=True)
def emu():
    old = ops.set_backend(EmuBackend())
    yield
    ops.set_backend(old)


def one_step(on, monkeypatch):
    monkeypatch.setattr(layers, "CONV1_PLANES", on)
    monkeypatch.setattr(layers, "OUT3_RECOMPUTE", on)
    B = 4
    m = T.build("cnn-mvae", True, True)
    inputs, targets = seeded_batch(B, 1234)
    eps, masks = seeded_noise(B, 256, 7, 8, 4321)
    step = MVAEStep(m, noise=InjectedNoise(eps, masks))
    loss = step.train_step(inputs, targets, 0.02)
    state = {"loss": loss.detach().clone().reshape(-1), "partials": step.partials[:7].clone(), "params": step.params.flat.clone()}
    for k, b in m.named_buffers():
        state["buffer " + k] = b.detach().clone()
    step.close()
    return state


def test_switches_fall_back_without_the_ops(monkeypatch):
    assert layers.CONV1_PLANES and layers.OUT3_RECOMPUTE                     # the product's defaults
    assert all(getattr(ops.B, n, None) is None for n in NEW_OPS)
    # the gate itself: no op on this backend -> None (the caller keeps its launches), whatever the switch says
    assert all(layers._conv3_plane_op(n, True, 64, torch.zeros(1)) is None for n in NEW_OPS)
    on, off = one_step(True, monkeypatch), one_step(False, monkeypatch)
    assert set(on) == set(off)
    for k in on:
        assert torch.isfinite(on[k].double()).all(), k
        assert torch.equal(on[k], off[k]), k
