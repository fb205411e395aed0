"""CPU emulation of the image-grid op (mmdyn_image_grid_u8): :class:`EmuBackendEma` plus ``image_grid`` restated in numpy, on its
own -- none of the oracle's functions (tests/grid_cases.py) are used, so a test of one against the other is no circle.  Where the
oracle walks make_grid's loops over the tiles, this walks the OUTPUT: every pixel's tile and offset by index arithmetic, as the
kernel does.  The sigmoid is 1 / (1 + exp(-x)) in fp32, the bytes float32 * 255 -> clip -> truncate.  Every call is recorded in
``grid_calls`` (private copies of the sources) for the tests that look at what a problem handed to the op.  Tests install it with
``ops.set_backend``; never imported by the product."""
import numpy as np
import torch

from mmdyn_hip import ops
from emu_backend_ema import EmuBackendEma


def _bytes(v):
    with np.errstate(invalid="ignore", over="ignore"):
        t = v * np.float32(255.0)
    out = np.zeros(t.shape, np.uint8)
    top, mid = t >= 255, (t > 0) & (t < 255)
    out[top] = 255
    out[mid] = t[mid].astype(np.uint8)          # (0 < t < 255: the conversion truncates)
    return out


class EmuBackendGrid(EmuBackendEma):

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.grid_calls = []

    def image_grid(self, srcs, take, nrow, logits, padding=2, out=None):
        srcs = ops.check_grid_sources(srcs, take, nrow, padding)
        arrays = [s.detach().cpu().numpy().copy() for s in srcs]
        self.grid_calls.append(dict(srcs=arrays, take=int(take), nrow=int(nrow), logits=bool(logits), padding=int(padding)))
        C, H, W = arrays[0].shape[1:]
        counts = [min(a.shape[0], take) for a in arrays]
        N = sum(counts)
        Hg, Wg = ops.grid_shape(N, H, W, nrow, padding)
        pad = 0 if N == 1 else padding
        xmaps = min(nrow, N)
        y, x = np.arange(Hg)[:, None] - pad, np.arange(Wg)[None, :] - pad
        ty, iy, tx, ix = y // (H + pad), y % (H + pad), x // (W + pad), x % (W + pad)
        k = ty * xmaps + tx
        inside = (y >= 0) & (x >= 0) & (iy < H) & (ix < W) & (k < N)
        grid = np.zeros((Hg, Wg, 3), np.uint8)
        first = 0
        for a, n in zip(arrays, counts):             # the images [first, first + n) of the list come from this source
            mine = inside & (k >= first) & (k < first + n)
            yy, xx = np.nonzero(mine)
            kk = (k + 0 * x)[yy, xx] - first
            for ch in range(3):
                v = a[kk, ch if C == 3 else 0, (iy + 0 * x)[yy, xx], (ix + 0 * y)[yy, xx]].astype(np.float32)
                if logits:
                    with np.errstate(over="ignore"):
                        v = (np.float32(1.0) / (np.float32(1.0) + np.exp(-v, dtype=np.float32))).astype(np.float32)
                grid[yy, xx, ch] = _bytes(v)
            first += n
        grid = torch.from_numpy(grid)
        if out is None:
            return grid.to(srcs[0].device)
        ops.check_grid_out(out, (Hg, Wg, 3), srcs[0].device)
        out.copy_(grid)
        return out
