#!/usr/bin/env python3
"""Generate tests/golden/conditions.npz: the reference's conditional models -- categorical (one-hot) and real-valued conditions,
vae.py:231-237, 286-291, 337-344; problems.py:463-465 -- on the seeded cases of tests/cond_cases.py, by RUNNING THE REFERENCE on the
CPU with the helpers of make_golden.py (same stand-in modules for its non-numeric imports, same injected noise).  Results only:
the inputs are regenerated from their seeds.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_conditions.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
import cond_cases as C  # noqa: E402

import torch  # noqa: E402

from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats  # noqa: E402

P, M = G.P, G.M
summarize = G.summarize


def make_self(model, use_pose, model_name, input_type="visuotactile"):
    s = G.make_self(model, use_pose, model_name, kl_weight=C.KL_WEIGHT, pose_multiplier=C.POSE_MULTIPLIER, input_type=input_type,
                    conditional=True)
    s.passes = []

    def elbo(self, *a, **k):
        r = P.Reconstruction._mvae_elbo_loss(self, *a, **k)
        (self.passes if r.dim() else self.partials).append(r.detach().clone() if r.dim() else float(r.detach()))
        return r

    s._mvae_elbo_loss = types.MethodType(elbo, s)
    s._criterion = s._elbo_loss
    return s


def gen_train(out):
    """(a) categorical cnn-mvae + pose, one train-mode step and one Adam step; (e) the reduce=False rows of the same call."""
    inputs, targets, eps, masks, idx = C.train_case()
    model = M.setup_model("cnn-mvae", cross_modal=True, **C.model_kw(True, True))
    sd = seeded_state_dict(model.state_dict(), 0)
    model.load_state_dict(sd)
    model.train()
    assert model.visual_encoder.linear_means.weight.shape == (C.LATENT, 512 + C.CAT_DIM)
    assert model.visual_decoder.upsample[0].weight.shape == (6400, C.LATENT + C.CAT_DIM)
    opt = torch.optim.Adam(model.parameters(), lr=C.LR)
    slf = make_self(model, True, "cnn-mvae")
    with G.Injector(eps, masks) as inj:
        opt.zero_grad()
        outputs, loss = slf._evaluate_mvae(x=list(inputs), targets=list(targets), condition=idx)
        loss.backward()
        assert inj.used_eps == 7 and inj.used_masks == 8
    out["a/loss"] = np.float64(loss.item())
    out["a/loss_partials"] = np.array(slf.partials, dtype=np.float64)
    out["a/means"] = outputs["means"].detach().numpy()
    out["a/recon2"] = outputs["recon_x"][2].detach().numpy()
    out["a/recon0"] = summarize(outputs["recon_x"][0], 256)
    grads = dict((n, p_.grad) for n, p_ in model.named_parameters())
    for n, g_ in grads.items():
        out["a/grad/" + n] = summarize(g_)
    for n in C.COND_WEIGHTS:
        out["a/grad_cond/" + n] = summarize(grads[n][:, -C.CAT_DIM:], 256)        # the condition columns alone
    opt.step()
    for n, p_ in model.named_parameters():
        out["a/param_step0/" + n] = summarize(p_)
    # (e) the per-sample rows of the same weights, inputs and noise
    model.load_state_dict(sd)
    model.train()
    slf = make_self(model, True, "cnn-mvae")
    x = {"model_input": [inputs[0], inputs[1]], "input_object_pose": [inputs[2]], "shock": idx}
    t = {"target_output": [targets[0], targets[1]], "target_object_pose": [targets[2]], "loss_mask": None}
    with G.Injector(eps, masks), torch.no_grad():
        _, rows = P.SeqModeling._evaluate_model(slf, x, t, reduce=False)
    assert rows.shape == (C.TRAIN_BATCH,)
    out["e/rows"] = rows.numpy()
    out["e/pass_rows"] = torch.stack(slf.passes).numpy()
    print("train", out["a/loss"], out["a/loss_partials"], "rows", out["e/rows"])


def gen_eval(tag, categorical, out):
    """(b) / (c): model.eval(), MVAE.forward of three subsets and MVAE.inference(n, c) with the latent injected."""
    inputs, eps, cond, z, cs = C.eval_case(categorical)
    model = M.setup_model("cnn-mvae", cross_modal=True, **C.model_kw(categorical, True))
    model.load_state_dict(seeded_running_stats(seeded_state_dict(model.state_dict(), 0)))
    model.eval()
    with torch.no_grad():
        for name, (a, b, c) in C.SUBSETS.items():
            with G.Injector([eps[name]], []):
                v, t, p, mu, lv = model([inputs[0] if a else None, inputs[1] if b else None], pose=inputs[2] if c else None,
                                        condition=cond)
            out[f"{tag}/{name}/visual"] = summarize(v, 256)
            out[f"{tag}/{name}/tactile"] = summarize(t, 256)
            out[f"{tag}/{name}/pose"] = p.numpy()
            out[f"{tag}/{name}/means"] = mu.numpy()
            out[f"{tag}/{name}/log_var"] = lv.numpy()
        with G.Injector([z], []):
            v, t = model.inference(n=C.SAMPLE_N, c=cs)
        out[f"{tag}/inference/visual"] = summarize(v, 256)
        out[f"{tag}/inference/tactile"] = summarize(t, 256)
    print(tag, out[f"{tag}/joint/means"][0, :4])


def gen_vae(out):
    """(d) categorical cnn-vae: Reconstruction._evaluate_model (the labels are the conditions), backward, inference."""
    x, labels, eps, masks, z, cs = C.vae_case()
    model = M.setup_model("cnn-vae", cross_modal=False, **C.model_kw(True))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 0))
    model.train()
    slf = make_self(model, False, "cnn-vae", input_type="visual")
    with G.Injector(eps, masks):
        outputs, loss = P.Reconstruction._evaluate_model(slf, x, labels)
        loss.backward()
    out["d/loss"] = np.float64(loss.item())
    out["d/means"] = outputs["means"].detach().numpy()
    out["d/log_var"] = outputs["log_var"].detach().numpy()
    out["d/recon"] = summarize(outputs["recon_x"], 256)
    for n, p_ in model.named_parameters():
        out["d/grad/" + n] = summarize(p_.grad)
    model.eval()
    with torch.no_grad(), G.Injector([z], []):
        v = model.inference(n=C.SAMPLE_N, c=cs)
    out["d/inference"] = summarize(v, 256)
    print("vae", out["d/loss"])


if __name__ == "__main__":
    out = {"kl_weight": np.float64(C.KL_WEIGHT), "pose_multiplier": np.float64(C.POSE_MULTIPLIER), "torch_version": torch.__version__}
    gen_train(out)
    gen_eval("b", True, out)
    gen_eval("c", False, out)
    gen_vae(out)
    np.savez_compressed(os.path.join(HERE, "conditions.npz"), **out)
    print("conditions.npz", os.path.getsize(os.path.join(HERE, "conditions.npz")), "bytes")
