#!/usr/bin/env python3
"""Generate tests/golden/weighted_elbo.npz: the reference's weighted per-sample loss ``(w * rows).sum() / B`` on its ``reduce=False``
branch (problems.py:401-458, 473-546) and the gradient of that scalar for every parameter, by RUNNING THE REFERENCE on the CPU
with the helpers of make_golden.py / make_golden_rows.py on seeded cases of tests/rows_cases.py and the weights of
tests/weighted_cases.py.  Results only: per parameter tensor a seeded subset of gradient elements and the tensor's L2 norm.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_weighted.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
import make_golden_rows as R  # noqa: E402
import rows_cases as C  # noqa: E402
import weighted_cases as W  # noqa: E402

import torch  # noqa: E402

from mmdyn_hip.utils.seeded_init import seeded_state_dict  # noqa: E402

P, M = G.P, G.M


def keep(model, name, w, rows, out):
    B = rows.shape[0]
    loss = (w * rows).sum() / B
    model.zero_grad()
    loss.backward()
    out[name + "/w"] = w.numpy()
    out[name + "/rows"] = rows.detach().numpy()
    out[name + "/loss"] = np.float64(loss.item())
    for k, p in model.named_parameters():
        g = p.grad.detach().reshape(-1)
        out[f"{name}/gnorm/{k}"] = np.float64(g.double().norm().item())
        out[f"{name}/gsample/{k}"] = g[W.sample_index(k, g.numel())].numpy()
    print(name, "w", w.numpy(), "loss", loss.item())


def gen_mvae(name, out):
    use_pose, B, mask_c, conditional = C.MVAE_CASES[name]
    inputs, targets, eps, masks, mask, cond = C.mvae_case(name)
    kw = dict(G.MODEL_KW)
    kw.update(use_pose=use_pose)
    model = M.setup_model("cnn-mvae", cross_modal=True, **kw)
    model.load_state_dict(seeded_state_dict(model.state_dict(), 0))
    model.train()
    slf = R.make_self(model, use_pose, "cnn-mvae", mask is not None)
    x, t = R.seq_io(inputs, targets, use_pose, mask, cond)
    with G.Injector(eps, masks):
        _, rows = P.SeqModeling._evaluate_model(slf, x, t, reduce=False)
    keep(model, name, W.weights(B), rows, out)


def gen_vae(name, out):
    x, y, eps, masks, mask = C.vae_case(name)
    model = G.build("cnn-vae", False)
    model.load_state_dict(seeded_state_dict(model.state_dict(), 0))
    model.train()
    slf = R.make_self(model, False, "cnn-vae", mask is not None, input_type="visual")
    with G.Injector(eps, masks):
        _, rows = P.SeqModeling._evaluate_model(slf, {"model_input": x, "shock": None}, {"target_output": y, "loss_mask": mask},
                                                reduce=False)
    keep(model, name, W.weights(C.VAE_BATCH), rows, out)


if __name__ == "__main__":
    out = {"kl_weight": np.float64(C.KL_WEIGHT), "pose_multiplier": np.float64(C.POSE_MULTIPLIER), "torch_version": torch.__version__}
    for name in W.MVAE_NAMES:
        gen_mvae(name, out)
    gen_vae(W.VAE_NAME, out)
    np.savez_compressed(os.path.join(HERE, "weighted_elbo.npz"), **out)
    print("weighted_elbo.npz", os.path.getsize(os.path.join(HERE, "weighted_elbo.npz")), "bytes")
