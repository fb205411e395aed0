"""CPU emulation of the operand join of the conditional models (mmdyn_concat_condition): :class:`EmuBackendRows` plus
``concat_condition`` restated with torch.cat / F.one_hot.  Tests install it with ``ops.set_backend``; never imported by the product."""
import torch
import torch.nn.functional as F

from emu_backend_rows import EmuBackendRows


class EmuBackendCond(EmuBackendRows):

    def concat_condition(self, x, cond, out, K, cd, bad_index=None):
        rows, width = out.shape
        assert width % 32 == 0 and K + cd <= width and x.shape[0] == rows
        if cond.dtype == torch.int64:
            assert tuple(cond.shape) == (rows,)
            ok = (cond >= 0) & (cond < cd)
            block = F.one_hot(torch.where(ok, cond, torch.zeros_like(cond)), cd).to(torch.float32) * ok.unsqueeze(1)
            if bad_index is not None and not bool(ok.all()):
                bad_index |= 1
        else:
            assert tuple(cond.shape) == (rows, cd) and cond.dtype == torch.float32
            block = cond
        out.copy_(torch.cat((x[:, :K], block, torch.zeros(rows, width - K - cd)), dim=-1))
