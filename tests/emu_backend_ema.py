"""CPU emulation of the parameter-average ops (mmdyn_ema_tick, mmdyn_ema_update, mmdyn_adam_step_ema): :class:`EmuBackendGradClip`
plus those three operations restated -- the tick in numpy fp64, the update as float32(e + omd * float32(p - e)) evaluated in fp64 from
the fp32 inputs.  Tests install it with ``ops.set_backend``; never imported by the product."""
import numpy as np
import torch

from emu_backend_gradclip import EmuBackendGradClip


def _state(es, name):
    if not torch.is_tensor(es) or es.dtype != torch.float64 or es.numel() != 4:
        raise ValueError(f"mmdyn_{name}: ema_state must be four fp64 values")


def tick_values(n, d, warmup):
    """(1 - d_n, n + 1) of one tick in numpy fp64: the two operations of the kernel, in its order."""
    n, d = np.float64(n), np.float64(d)
    dn = d
    if warmup:
        w = (np.float64(1.0) + n) / (np.float64(10.0) + n)
        dn = w if w < d else d
    return np.float64(1.0) - dn, n + np.float64(1.0)


def ema_reference(e, p, omd):
    """float32(e + omd * float32(p - e)) with omd = float32(1 - d_n): fp64 arithmetic on the fp32 inputs, ONE final rounding (the
    product of two fp32 values is exact in fp64, and the fp64 sum rounds far below half an fp32 ulp of the result)."""
    omd = np.float64(np.float32(omd))
    e64, p64 = e.detach().double().numpy(), p.detach().double().numpy()
    diff = (p64 - e64).astype(np.float32).astype(np.float64)
    return torch.from_numpy((e64 + omd * diff).astype(np.float32))


class EmuBackendEma(EmuBackendGradClip):

    def ema_tick(self, ema_state, adam_state=None):
        _state(ema_state, "ema_tick")
        if adam_state is not None and float(adam_state[5]) != 0.0:
            return
        omd, n1 = tick_values(float(ema_state[0]), float(ema_state[1]), float(ema_state[3]) != 0.0)
        ema_state[2], ema_state[0] = float(omd), float(n1)

    def ema_update(self, ema, p, ema_state):
        _state(ema_state, "ema_update")
        if ema.numel() != p.numel():
            raise ValueError("mmdyn_ema_update: ema must hold as many elements as p")
        if ema.data_ptr() == p.data_ptr() and ema.numel():
            raise ValueError("mmdyn_ema_update: ema must not alias p")
        ema.copy_(ema_reference(ema, p, float(ema_state[2])).view_as(ema))

    def adam_step_ema(self, p, g, m, v, ema, state, clip, ema_state, lr, beta1, beta2, eps, grad_scale, guarded=False):
        _state(ema_state, "adam_step_ema")
        if clip is None:
            self.adam_step(p, g, m, v, state, lr, beta1, beta2, eps, grad_scale, guarded=guarded)
        else:
            self.adam_step_clipped(p, g, m, v, state, clip, lr, beta1, beta2, eps, grad_scale, guarded=guarded)
        if guarded and float(state[5]) != 0.0:
            return
        self.ema_tick(ema_state)
        self.ema_update(ema, p, ema_state)
