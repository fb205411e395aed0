#!/usr/bin/env python3
"""Generate tests/golden/elbo_rows.npz: the reference's per-sample ELBO (``reduce=False``, problems.py:401-458, 473-546, 683-716)
on the seeded cases of tests/rows_cases.py, by RUNNING THE REFERENCE on the CPU with the helpers of make_golden.py (same stand-in
modules for its non-numeric imports, same injected noise).  Results only: the inputs are regenerated from their seeds.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_rows.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
import rows_cases as C  # noqa: E402

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats  # noqa: E402

P, M = G.P, G.M


def make_self(model, use_pose, model_name, mask_loss, input_type="visuotactile", conditional=False):
    """make_golden.make_self with a recorder that keeps each pass's VECTOR (its own takes float() of the result)."""
    s = G.make_self(model, use_pose, model_name, kl_weight=C.KL_WEIGHT, pose_multiplier=C.POSE_MULTIPLIER, input_type=input_type,
                    conditional=conditional)
    s.parameters["mask_loss"] = mask_loss
    s.passes = []

    def elbo(self, *a, **k):
        r = P.Reconstruction._mvae_elbo_loss(self, *a, **k)
        self.passes.append(r.detach().clone())
        return r

    s._mvae_elbo_loss = types.MethodType(elbo, s)
    return s


def seq_io(inputs, targets, use_pose, mask, cond):
    x = {"model_input": [inputs[0], inputs[1]], "input_object_pose": [inputs[2]] if use_pose else None, "shock": cond}
    t = {"target_output": [targets[0], targets[1]], "target_object_pose": [targets[2]] if use_pose else None, "loss_mask": mask}
    return x, t


def gen_mvae(name, out):
    use_pose, B, mask_c, conditional = C.MVAE_CASES[name]
    inputs, targets, eps, masks, mask, cond = C.mvae_case(name)
    kw = dict(G.MODEL_KW)
    kw.update(use_pose=use_pose)
    if conditional:
        kw.update(conditional=True, condition_dim=3)
    model = M.setup_model("cnn-mvae", cross_modal=True, **kw)
    sd = seeded_state_dict(model.state_dict(), 0)
    for reduce in (False, None):       # the same weights, buffers and noise for the per-sample and the scalar call
        model.load_state_dict(sd)
        model.train()
        slf = make_self(model, use_pose, "cnn-mvae", mask is not None, conditional=conditional)
        x, t = seq_io(inputs, targets, use_pose, mask, cond)
        with G.Injector(eps, masks) as inj, torch.no_grad():
            outputs, loss = P.SeqModeling._evaluate_model(slf, x, t, reduce=reduce)
            assert inj.used_eps == len(eps) and inj.used_masks == len(masks)
        if reduce is False:
            assert loss.shape == (B,) and loss.dtype == torch.float32
            out[name + "/rows"] = loss.numpy()
            out[name + "/pass_rows"] = torch.stack(slf.passes).numpy()
            out[name + "/means"] = outputs["means"].numpy()
        else:
            out[name + "/scalar"] = np.float64(loss.item())
    print(name, out[name + "/rows"], "mean", out[name + "/rows"].mean(), "scalar", out[name + "/scalar"])


def gen_vae(name, out):
    x, y, eps, masks, mask = C.vae_case(name)
    model = G.build("cnn-vae", False)
    sd = seeded_state_dict(model.state_dict(), 0)
    for reduce in (False, None):
        model.load_state_dict(sd)
        model.train()
        slf = make_self(model, False, "cnn-vae", mask is not None, input_type="visual")
        with G.Injector(eps, masks), torch.no_grad():
            outputs, loss = P.SeqModeling._evaluate_model(slf, {"model_input": x, "shock": None},
                                                          {"target_output": y, "loss_mask": mask}, reduce=reduce)
        if reduce is False:
            assert loss.shape == (C.VAE_BATCH,)
            out[name + "/rows"] = loss.numpy()
        else:
            out[name + "/scalar"] = np.float64(loss.item())
    print(name, out[name + "/rows"][:4], "scalar", out[name + "/scalar"])


def gen_eval(out):
    """The serving case: model.eval() (BatchNorm on running estimates, dropout off), one joint pass, per-sample terms."""
    inputs, targets, eps = C.eval_case()
    model = G.build("cnn-mvae", True, use_pose=True)
    model.load_state_dict(seeded_running_stats(model.state_dict()))
    model.eval()
    with torch.no_grad(), G.Injector([eps], []):
        v, t, p, mu, lv = model([inputs[0], inputs[1]], pose=inputs[2])
    out["eval/bce_visual"] = F.binary_cross_entropy_with_logits(v, targets[0], reduction="none").sum((1, 2, 3)).numpy()
    out["eval/bce_tactile"] = F.binary_cross_entropy_with_logits(t, targets[1], reduction="none").sum((1, 2, 3)).numpy()
    out["eval/mse_pose"] = F.mse_loss(p, targets[2], reduction="none").sum(1).numpy()
    out["eval/kl"] = (-0.5 * (1 + lv - mu.pow(2) - lv.exp())).sum(1).numpy()
    # against the INPUTS as targets too (the default of MVAEInference.score)
    out["eval/self_bce_visual"] = F.binary_cross_entropy_with_logits(v, inputs[0], reduction="none").sum((1, 2, 3)).numpy()
    out["eval/self_bce_tactile"] = F.binary_cross_entropy_with_logits(t, inputs[1], reduction="none").sum((1, 2, 3)).numpy()
    out["eval/self_mse_pose"] = F.mse_loss(p, inputs[2], reduction="none").sum(1).numpy()
    print("eval", out["eval/bce_visual"], out["eval/mse_pose"], out["eval/kl"])


if __name__ == "__main__":
    out = {"kl_weight": np.float64(C.KL_WEIGHT), "pose_multiplier": np.float64(C.POSE_MULTIPLIER),
           "torch_version": torch.__version__}
    for name in C.MVAE_CASES:
        gen_mvae(name, out)
    for name in C.VAE_CASES:
        gen_vae(name, out)
    gen_eval(out)
    np.savez_compressed(os.path.join(HERE, "elbo_rows.npz"), **out)
    print("elbo_rows.npz", os.path.getsize(os.path.join(HERE, "elbo_rows.npz")), "bytes")
