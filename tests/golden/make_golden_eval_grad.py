#!/usr/bin/env python3
"""Generate tests/golden/eval_grad.npz: gradients THROUGH the reference's MVAE in ``eval()`` mode (BatchNorm2d frozen at its running
estimates, Dropout the identity), by RUNNING THE REFERENCE on the CPU with the helpers of make_golden.py: cnn-mvae with pose,
seeded weights and seeded running statistics, B = 3, injected reparametrisation noise.  Stored (results only):

  * the scalar ``_mvae_elbo_loss`` of the joint pass (visual + tactile + pose in, all three reconstructed);
  * its gradient w.r.t. every parameter and w.r.t. both input images;
  * for each image decoder alone, d(sum(logits * r)) / dz for a fixed r.

A tensor of at most FULL elements is stored whole, a larger one as ``summarize(t, 256)`` (sum, L2 norm, element count, 256 evenly
spaced elements); the image gradients additionally with sample 0 whole.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_eval_grad.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
import eval_grad_cases as C  # noqa: E402

import torch  # noqa: E402

from mmdyn_hip.utils.seeded_init import seeded_running_stats  # noqa: E402


def keep(out, key, t):
    t = t.detach().clone()              # (a copy: the decoder passes below accumulate into the same .grad tensors)
    out[key] = t.numpy() if t.numel() <= C.FULL else G.summarize(t, 256)


if __name__ == "__main__":
    inputs, targets, eps, z, r = C.case()
    model = G.build("cnn-mvae", True, use_pose=True)
    model.load_state_dict(seeded_running_stats(model.state_dict()))
    model.eval()
    buffers = {k: b.clone() for k, b in model.named_buffers()}
    slf = G.make_self(model, True, "cnn-mvae", kl_weight=C.KL_WEIGHT, pose_multiplier=C.POSE_MULTIPLIER)
    v, t, p = (x.clone() for x in inputs)
    v.requires_grad_(True), t.requires_grad_(True)
    with G.Injector([eps], []):
        vr, tr, pr, mu, lv = model([v, t], pose=p)
    loss = slf._mvae_elbo_loss([vr, tr, pr], list(targets), mu, lv)
    model.zero_grad()
    loss.backward()
    out = {"batch": C.B, "kl_weight": np.float64(C.KL_WEIGHT), "pose_multiplier": np.float64(C.POSE_MULTIPLIER),
           "torch_version": torch.__version__, "loss": np.float64(loss.item()), "eps": eps.numpy(), "z": z.numpy(),
           "means": mu.detach().clone().numpy()}
    for k, prm in model.named_parameters():
        keep(out, "grad/" + k, prm.grad)
    for name, x in (("visual", v), ("tactile", t)):
        out[f"gx/{name}"] = G.summarize(x.grad, 256)
        out[f"gx/{name}0"] = x.grad[0].clone().numpy()
    for name, dec in (("visual", model.visual_decoder), ("tactile", model.tactile_decoder)):
        zz = z.clone().requires_grad_(True)
        (dec(zz) * r).sum().backward()
        out[f"dz/{name}"] = zz.grad.clone().numpy()
    for k, b in model.named_buffers():
        assert torch.equal(b, buffers[k]), k                      # eval(): the forward leaves the running estimates alone
    np.savez_compressed(os.path.join(HERE, "eval_grad.npz"), **out)
    print("eval_grad.npz", os.path.getsize(os.path.join(HERE, "eval_grad.npz")), "bytes; loss", loss.item())
