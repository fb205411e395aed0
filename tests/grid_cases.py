"""Oracle and case table of the image-grid kernel (mmdyn_image_grid_u8), shared by tests/test_image_grid_emu.py and
tests/test_image_grid_gpu.py.  A plain module, like tests/dirty.py.

Oracle (numpy): the layout by the loops of torchvision.utils.make_grid(img, nrow, padding, pad_value=0) on the image list
cat(src0[:take], src1[:take]); the bytes by the writer's rule float32 * 255 -> clip -> truncate.
  logits = 0: one fp32 multiply, deterministic -- a byte must EQUAL the oracle's.
  logits = 1: v = 255 * sigmoid(x) in fp64 from the fp32 logit; a byte must equal floor(v) clipped to 0..255, unless
              |v - round(v)| < BAND = 1e-3, where either neighbouring integer (round(v) - 1 or round(v), clipped) is accepted.  The band
              is in byte units: 4e-6 in the sigmoid, about 60 fp32 ulps at 1 -- far above expf plus one fp32 multiply, far below the
              whole bytes an indexing error produces.  A non-finite logit is exact: -inf and NaN give 0, +inf gives 255.  The bytes
              with two accepted values may be at most 1 % of a case's sigmoid bytes: asserted HERE, so that no test can hide a
              failure in the band.
"""
import functools

import numpy as np

BAND = 1e-3
BAND_CAP = 0.01
GUARD = 64            # bytes in front of and behind the output range inside the pre-filled buffer (a multiple of 4)
FILLS = (0xA5, 0x5A)  # tests/dirty.py's JUNK byte and its complement: a byte the launch left alone differs between the two runs

SPECIALS0 = (-0.5, 0.0, 0.999999, 1.0, 1.5, 7.0 / 255.0, float("nan"), float("inf"), float("-inf"))
SPECIALS1 = (float("-inf"), -100.0, 0.0, 100.0, float("inf"), float("nan"))


def _case(name, n0, n1, take, nrow, padding, C=3, H=3, W=5, logits=(0, 1), specials=None, what=""):
    return dict(name=name, n0=n0, n1=n1, take=take, nrow=nrow, padding=padding, C=C, H=H, W=W, logits=logits, specials=specials,
                what=what)


# every case names the smallest shape at which that part of the kernel can go wrong
CASES = [
    _case("rows_of_48_bytes_empty_cell", 5, 0, 5, 2, 2, what="3 * Wg = 48 and the total 816 are multiples of 4; ymaps = 3, last cell empty"),
    _case("dwords_straddle_rows", 3, 0, 3, 3, 1, H=2, W=3, what="3 * Wg = 39 bytes: dwords straddle rows and channels (4 x 13 x 3 = 156)"),
    _case("dwords_straddle_rows_and_tail", 3, 0, 3, 3, 1, H=3, W=3, what="3 * Wg = 39; the total 5 x 13 x 3 = 195 leaves a 3-byte tail"),
    _case("two_sources_take_between", 2, 5, 3, 4, 2, H=3, W=4, what="N = 5: src1 starts at image 2, its images 3 and 4 stay out"),
    _case("single_image_n0_1", 1, 0, 5, 4, 2, what="N = 1: no border"),
    _case("single_image_take_1", 4, 0, 1, 4, 2, what="N = 1 by take: no border"),
    _case("nrow_above_N", 3, 0, 3, 8, 2, what="xmaps = 3, one row"),
    _case("one_channel", 5, 0, 5, 2, 2, C=1, what="C = 1 replicated to RGB"),
    _case("no_padding", 4, 0, 4, 2, 0, what="tiles abut"),
    _case("specials_plain", 1, 0, 1, 1, 2, H=8, W=8, logits=(0,), specials=SPECIALS0, what="clip, truncation, NaN, +-inf"),
    _case("specials_logits", 1, 0, 1, 1, 2, H=8, W=8, logits=(1,), specials=SPECIALS1, what="saturated and non-finite logits"),
    _case("workload_shape", 256, 256, 120, 16, 2, H=64, W=64, logits=(1,), what="240 tiles of 64 x 64: a 15 x 16 grid"),
]
RUNS = [(c["name"], lg) for c in CASES for lg in c["logits"]]


def case(name):
    return next(c for c in CASES if c["name"] == name)


def grid_shape(N, H, W, nrow, padding):
    """(Hg, Wg) as the issue states the layout; the product's ops.grid_shape must agree."""
    if N == 1:
        return H, W
    xmaps = min(nrow, N)
    ymaps = (N + xmaps - 1) // xmaps
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def sources(name, logits):
    """The fp32 sources [n][C][H][W] of a run (numpy, seeded by the case's position): 3 * randn logits, or values in [-0.1, 1.1]
    so that both clips occur.  The specials sit at the start of an image of harmless values (logit 0 / value 0.5)."""
    c = case(name)
    rng = np.random.default_rng(1000 + 2 * [k["name"] for k in CASES].index(name) + logits)
    out = []
    for n in (c["n0"], c["n1"]):
        if n == 0:
            continue
        shape = (n, c["C"], c["H"], c["W"])
        if c["specials"] is not None:
            x = np.full(shape, 0.0 if logits else 0.5, np.float32)
            x.reshape(-1)[:len(c["specials"])] = np.array(c["specials"], np.float32)
        elif logits:
            x = (3.0 * rng.standard_normal(shape)).astype(np.float32)
            if x.size < 1000:
                # a case of a few dozen bytes has no room for a byte in the band under the 1 % cap: such a logit is drawn again
                # (decided by the oracle's fp64 value alone, before any code under test runs)
                lo, hi = sigmoid_bounds(x)
                while (lo != hi).any():
                    x = np.where(lo != hi, (3.0 * rng.standard_normal(shape)).astype(np.float32), x)
                    lo, hi = sigmoid_bounds(x)
        else:
            x = rng.uniform(-0.1, 1.1, shape).astype(np.float32)
        out.append(x)
    return out


def layout(srcs, take, nrow, padding):
    """make_grid's loops on cat(src[:take] for src in srcs): (values fp32 [Hg][Wg][3], inside bool [Hg][Wg][3])."""
    imgs = np.concatenate([s[:take] for s in srcs], 0)
    N, C, H, W = imgs.shape
    if C == 1:
        imgs = np.repeat(imgs, 3, 1)
    if N == 1:
        return np.ascontiguousarray(imgs[0].transpose(1, 2, 0)), np.ones((H, W, 3), bool)
    xmaps = min(nrow, N)
    ymaps = (N + xmaps - 1) // xmaps
    h, w = H + padding, W + padding
    grid = np.zeros((3, h * ymaps + padding, w * xmaps + padding), np.float32)
    inside = np.zeros(grid.shape, bool)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= N:
                break
            grid[:, y * h + padding:y * h + padding + H, x * w + padding:x * w + padding + W] = imgs[k]
            inside[:, y * h + padding:y * h + padding + H, x * w + padding:x * w + padding + W] = True
            k += 1
    return np.ascontiguousarray(grid.transpose(1, 2, 0)), np.ascontiguousarray(inside.transpose(1, 2, 0))


def plain_bytes(v):
    """float32 * 255, clip, truncate; NaN fails both comparisons and gives 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = v.astype(np.float32) * np.float32(255.0)
        low = np.where(t > 0, np.minimum(t, np.float32(254.0)), np.float32(0.0))      # (finite, NaN -> 0: safe to convert)
        return np.where(t >= 255, 255, np.trunc(low)).astype(np.uint8)


def sigmoid_bounds(x):
    """(lo, hi) uint8: the accepted bytes of logits x (fp32) -- lo == hi outside the band."""
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        v = 255.0 / (1.0 + np.exp(-x64))
    fin = np.isfinite(x64)
    v = np.where(fin, v, 0.0)
    r = np.round(v)
    near = fin & (np.abs(v - r) < BAND)
    lo = np.where(near, r - 1, np.floor(v))
    hi = np.where(near, r, np.floor(v))
    lo, hi = np.clip(lo, 0, 255), np.clip(hi, 0, 255)
    lo = np.where(np.isposinf(x64), 255, lo)
    hi = np.where(np.isposinf(x64), 255, hi)
    return lo.astype(np.uint8), hi.astype(np.uint8)


def bounds(srcs, take, nrow, padding, logits):
    """(lo, hi) uint8 [Hg][Wg][3] of any sources: what a grid of them must lie between (lo == hi: exactly)."""
    values, inside = layout(srcs, take, nrow, padding)
    if not logits:
        b = np.where(inside, plain_bytes(values), 0).astype(np.uint8)
        return b, b
    lo, hi = sigmoid_bounds(values)
    lo, hi = np.where(inside, lo, 0).astype(np.uint8), np.where(inside, hi, 0).astype(np.uint8)
    wide = int((lo != hi).sum())
    assert wide <= BAND_CAP * int(inside.sum()), f"the band covers {wide} of {int(inside.sum())} sigmoid bytes: above 1 %"
    return lo, hi


@functools.lru_cache(maxsize=None)
def expected(name, logits):
    """(lo, hi) of a run of the table, computed once and shared; read-only."""
    c = case(name)
    lo, hi = bounds(sources(name, logits), c["take"], c["nrow"], c["padding"], logits)
    N = min(c["n0"], c["take"]) + min(c["n1"], c["take"])
    assert lo.shape == grid_shape(N, c["H"], c["W"], c["nrow"], c["padding"]) + (3,)
    lo.setflags(write=False)
    hi.setflags(write=False)
    return lo, hi


def assert_within(got, lo, hi, what=""):
    """``got`` uint8 [Hg][Wg][3] (numpy) lies in [lo, hi] byte for byte; a failure names the first offending (row, column, channel)."""
    assert got.shape == lo.shape and got.dtype == np.uint8, (what, got.shape, lo.shape, got.dtype)
    bad = np.argwhere((got < lo) | (got > hi))
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} bytes outside the oracle's bounds, first at (row, column, channel) "
                           f"{tuple(bad[0])}: got {got[tuple(bad[0])]}, accepted {lo[tuple(bad[0])]}..{hi[tuple(bad[0])]}")


def check_specials(name, got):
    """The bytes the issue lists for the two specials cases, on top of the oracle's bounds (N = 1: the grid is the image, HWC, so
    special i of channel 0 sits at pixel i, channel 0)."""
    flat = got[:, :, 0].reshape(-1)
    if name == "specials_plain":
        want = [0, 0, 254, 255, 255, int(plain_bytes(np.array([7.0 / 255.0], np.float32))[0]), 0, 255, 0]
        assert flat[:9].tolist() == want, (flat[:9].tolist(), want)
    elif name == "specials_logits":
        f = flat[:6].tolist()
        assert f[:3] == [0, 0, 127] and f[3] in (254, 255) and f[4:] == [255, 0], f


def run_guarded(launch, shape, device):
    """The guard-byte check every run makes (the tests/dirty.py pattern): ``launch(out)`` writes an ``out`` of ``shape`` carved out
    of a larger uint8 buffer on ``device``, once per pre-fill of FILLS.  The GUARD bytes in front of and behind the range must
    still hold the fill, and the range must come out the same under both fills -- a byte the launch left alone would differ.
    Returns the range as numpy uint8 of ``shape``."""
    import torch
    total = int(np.prod(shape))
    got = []
    for fill in FILLS:
        buf = torch.full((2 * GUARD + total,), fill, dtype=torch.uint8, device=device)
        launch(buf[GUARD:GUARD + total].view(shape))
        flat = buf.cpu().numpy()
        for what, part in (("in front of", flat[:GUARD]), ("behind", flat[GUARD + total:])):
            touched = np.flatnonzero(part != fill)
            assert touched.size == 0, f"a byte {what} the output range was written (offset {int(touched[0])} of that guard)"
        got.append(flat[GUARD:GUARD + total].reshape(shape))
    left = np.flatnonzero(got[0].reshape(-1) != got[1].reshape(-1))
    assert left.size == 0, f"byte {int(left[0])} of the output range depends on what the buffer held: it was not written"
    return got[0]
