"""CPU emulation of the global-norm clipping ops (mmdyn_grad_sumsq, mmdyn_grad_clip_coef, mmdyn_adam_step_clipped,
mmdyn_sgd_step_clipped): :class:`EmuBackend` plus those four operations restated with torch in fp64.  Tests install it with
``ops.set_backend``; never imported by the product."""
import math

import numpy as np
import torch

from emu_backend import EmuBackend


def _clip(clip, name):
    if not torch.is_tensor(clip) or clip.dtype != torch.float64 or clip.numel() != 4:
        raise ValueError(f"mmdyn_{name}: clip must be four fp64 values")


def clip_factor(grad_scale, coef):
    """f = float32(double(float32(grad_scale)) * coef): the fp32 factor the clipped steps multiply the gradient by."""
    return float(np.float32(np.float64(np.float32(grad_scale)) * np.float64(coef)))


class EmuBackendGradClip(EmuBackend):

    def grad_sumsq_blocks(self, n):
        return self.lib.mmdyn_grad_sumsq_blocks(int(n))

    def grad_sumsq(self, g, partials, clip, accumulate=False):
        _clip(clip, "grad_sumsq")
        need = self.grad_sumsq_blocks(g.numel())
        if partials is None or partials.dtype != torch.float64 or partials.numel() < need:
            raise ValueError(f"mmdyn_grad_sumsq: partials must be an fp64 workspace of at least {need} values")
        partials[:need] = float("nan")                  # (a workspace: nothing of it survives a call)
        s = float((g.double() ** 2).sum())
        clip[0] = float(clip[0]) + s if accumulate else s

    def grad_clip_coef(self, clip, grad_scale, max_norm):
        _clip(clip, "grad_clip_coef")
        max_norm = np.float64(np.float32(max_norm))
        if not max_norm > 0:
            raise ValueError("mmdyn_grad_clip_coef: max_norm must be a real number > 0")
        with np.errstate(all="ignore"):                 # (IEEE arithmetic on a non-finite sum, as on the device)
            norm = np.abs(np.float64(np.float32(grad_scale))) * np.sqrt(np.float64(float(clip[0])))
            c = max_norm / (norm + np.float64(1e-6))
        coef = float(c) if (c < 1.0 or np.isnan(c)) else 1.0
        clip[1], clip[2] = float(norm), coef
        if coef < 1.0 and math.isfinite(norm):
            clip[3] += 1

    def adam_step_clipped(self, p, g, m, v, state, clip, lr, beta1, beta2, eps, grad_scale, guarded=False):
        _clip(clip, "adam_step_clipped")
        if state.numel() < (6 if guarded else 3):
            raise ValueError("mmdyn_hip: the guarded Adam step keeps six doubles of state")
        if guarded and not math.isfinite(float(clip[1])):
            state[4] += 1
            state[5] = 1
            return
        if guarded:
            state[5] = 0
        self.adam_step(p, g, m, v, state, lr, beta1, beta2, eps, clip_factor(grad_scale, float(clip[2])), guarded=False)

    def sgd_step_clipped(self, p, g, buf, clip, lr, momentum, weight_decay, grad_scale, first):
        _clip(clip, "sgd_step_clipped")
        self.sgd_step(p, g, buf, lr, momentum, weight_decay, clip_factor(grad_scale, float(clip[2])), first)
