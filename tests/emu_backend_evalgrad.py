"""CPU emulation of mmdyn_bn_eval_swish_bwd (the one-pass backward of eval-mode BatchNorm + Swish): :class:`EmuBackendWeighted` plus
that operation restated with torch, including its plane destination (the exact three-term bf16 split of ops.Planes) and the
``partial`` table in the layout of mmdyn_bn_swish_bwd_reduce.  Tests install it with ``ops.set_backend``; never imported by the
product."""
import torch

from emu_backend import _act_grad
from emu_backend_weighted import EmuBackendWeighted


def split_planes(x, planes):
    """x [rows][C] fp32 -> planes.t [rows][3][C] bf16: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round to nearest
    even (torch's fp32 -> bf16 conversion); hi + mid + lo == x bit for bit."""
    x = x.reshape(planes.rows, planes.C).float()
    hi = x.to(torch.bfloat16)
    r = x - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    planes.t.copy_(torch.stack((hi, mid, lo), dim=1))


class EmuBackendEvalGrad(EmuBackendWeighted):

    def bn_eval_swish_bwd(self, da, y, mean, rstd, gamma, beta, dy, partial, G, rpg, C, da_is_du=False, planes=None):
        self.calls.append("bn_eval_swish_bwd")
        if dy is None and planes is None:
            raise ValueError("mmdyn_hip: bn_eval_swish_bwd: one of dy / planes is required")
        need_y = (not da_is_du) or partial is not None
        if need_y and y is None:
            raise ValueError("mmdyn_hip: bn_eval_swish_bwd: y may be None only with da_is_du and without partial")
        du = da.reshape(G, rpg, C).float()
        if need_y:
            xh = self._xhat(y.float(), mean, rstd, G, rpg, C)
            if not da_is_du:
                du = du * _act_grad(xh * gamma + beta, 1)
        if partial is not None:
            T = self.colstats_tiles(rpg)
            assert partial.numel() == G * T * 2 * C, (tuple(partial.shape), G, T, C)
            p = partial.reshape(G, T, 2, C)
            p.zero_()
            # spread over the first and the last tile: whoever reads the table must sum every tile
            p[:, 0, 0] += 0.5 * du.sum(1)
            p[:, 0, 1] += 0.5 * (du * xh).sum(1)
            p[:, T - 1, 0] += 0.5 * du.sum(1)
            p[:, T - 1, 1] += 0.5 * (du * xh).sum(1)
        out = du * (gamma * rstd[:, None])
        if dy is not None:
            dy.reshape(-1).copy_(out.reshape(-1))
        if planes is not None:
            assert planes.rows == G * rpg and planes.C == C
            split_planes(out, planes)
