"""Inputs for which the multiply-accumulate kernels have ONE correct answer, shared by tests/test_exact_emu.py (EmuBackend, CPU) and
tests/test_exact_gpu.py (HipBackend, every route).  No tolerance appears here: every comparison is `==` on values or on bits.

Family A -- integer operands.  Small integers are exact in fp32, bf16 (|x| <= 256) and half (|x| <= 2048), their products are exact
    in the fp32 accumulator, and while sum |a||b| < 2^24 over the K range of an output element every partial sum is an exactly
    representable integer: any order, any route, any split over blocks, slabs or chunks gives the same number.  The reference is
    fp64 ATen (F.conv2d / F.conv_transpose2d / F.linear and their autograd), the precondition is asserted on the reference alone.
Family B -- selection weights.  One operand is arbitrary fp32 (24-bit mantissas, exponents over +-20 binades, no zero, no
    denormal), the other is one-hot per output column with value +-2^k, k in [-3, 3]: every output element is one input element
    scaled by a power of two, or exactly +0 where the tap falls into the padding.  The reference is index arithmetic; compared bit
    for bit (the 16-bit matrix-core modes against the RNE-rounded element: this pins the rounding mode per element).

16-bit stored operands (the `store` arguments; "bf16s" / "fp16s"): the integers and the +-2^k are exact in either type, so family A
    applies unchanged; family B's arbitrary operand is the RNE-rounded element, stored or rounded on its way into the matrix cores.

Every output of a launch is a slice in the middle of a larger buffer pre-filled with the JUNK pattern of tests/dirty.py (Guarded):
at least 64 rows in front and behind, and the columns N..ldc of the rows inside, must hold that pattern bit for bit afterwards.

A plain module, like tests/dirty.py and tests/iw_cases.py; no fixture, no pytest setting.
"""
import torch
import torch.nn.functional as F

from dirty import JUNK, bits, fill_
from mmdyn_hip.ops import DENSE, CONV, TCONV_S2P1, IM2COL3, TCONV_S1P0

GUARD_ROWS = 64
LIMIT = float(1 << 24)
INT_MAX_16 = {torch.bfloat16: 256.0, torch.float16: 2048.0}     # largest magnitude below which EVERY integer is exact
# exponent spread of the arbitrary operand: fp32 / bf16 share an exponent range; half is normal for 2^-14 .. 2^15, and the
# element is scaled by up to 2^3 afterwards
BINADES = {None: 20, torch.bfloat16: 20, torch.float16: 10}


# ---- guard rows -----------------------------------------------------------------------------------------------------------------
class Guarded:
    """A [rows][ld] output (the kernel writes columns 0..width) as a contiguous slice of a larger JUNK-filled buffer: >= 64 rows
    of the same stride in front and behind, the slice's start 256-byte aligned."""

    def __init__(self, rows, width, dtype=torch.float32, device="cpu", ld=None):
        self.rows, self.width, self.ld = rows, width, ld or width
        self.front = -(-GUARD_ROWS * self.ld // 128) * 128
        self.n = rows * self.ld
        self.buf = fill_(torch.empty(self.front + self.n + GUARD_ROWS * self.ld, dtype=dtype, device=device), JUNK)
        self.t = self.buf[self.front:self.front + self.n]
        assert self.t.is_contiguous() and (self.front * self.buf.element_size()) % 256 == 0
        assert self.buf.device.type == "cpu" or self.t.data_ptr() % 256 == 0

    def view(self, *shape):
        return self.t.view(*shape)

    def values(self):
        """What the launch wrote: [rows][width] on the CPU."""
        return self.t.detach().cpu().view(self.rows, self.ld)[:, :self.width].clone()

    def check(self, what):
        """Everything outside the declared extent still holds the sentinel bit for bit."""
        sentinel = bits(fill_(torch.empty(1, dtype=self.buf.dtype), JUNK))[0]
        guard = torch.ones(self.buf.numel(), dtype=torch.bool)
        guard[self.front:self.front + self.n].view(self.rows, self.ld)[:, :self.width] = False
        bad = ((bits(self.buf) != sentinel) & guard).nonzero()
        if bad.numel():
            i = int(bad[0]) - self.front
            where = f"row {i // self.ld}, column {i % self.ld} of the slice" if 0 <= i < self.n else \
                (f"{-i} elements in front of the slice" if i < 0 else f"{i - self.n} elements behind the slice")
            raise AssertionError(f"{what}: wrote outside its declared extent ({self.rows} rows x {self.width} columns, row stride "
                                 f"{self.ld}) at guard index {i} ({where}): found {self.buf.reshape(-1)[int(bad[0])].item()!r}")


def check_exact(got, want, what, bitwise=False):
    """got == want element for element ([rows][columns]); `bitwise`: the bit patterns (want is cast to got's type first, which is
    exact for every reference here).  A failure names the first differing flat index, its (row, column) and both values."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} against the reference's {tuple(want.shape)}"
    if bitwise:
        ne = bits(got) != bits(want.to(got.dtype))
    else:
        ne = ~(got.double().reshape(-1) == want.double().reshape(-1))        # (a NaN differs from everything)
    bad = ne.nonzero()
    if bad.numel():
        i = int(bad[0])
        cols = got.shape[-1] if got.dim() > 1 else got.numel()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, the first at flat index {i} (row {i // cols}, "
                             f"column {i % cols}): expected {want.reshape(-1)[i].item()!r}, found {got.reshape(-1)[i].item()!r}")


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed, mag=3, density=1.0):
    """Integers in [-mag, mag] as fp32; density < 1: that share of the entries is kept, the rest is zero."""
    g = _gen(seed)
    x = torch.randint(-mag, mag + 1, tuple(shape), generator=g).float()
    if density < 1.0:
        x = x * (torch.rand(tuple(shape), generator=g) < density)
    return x


def arbitrary(shape, seed, binades=20):
    """fp32 with full 24-bit mantissas (odd and even), exponents uniform over [-binades, binades], both signs; no zero, no denormal."""
    g = _gen(seed)
    shape = tuple(shape)
    mant = torch.randint(1 << 23, 1 << 24, shape, generator=g).float()
    e = torch.randint(-binades, binades + 1, shape, generator=g).float()
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * mant * torch.exp2(e - 23)


def pow2(n, seed):
    g = _gen(seed)
    return (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1) * torch.exp2(torch.randint(-3, 4, (n,), generator=g).float())


# ---- implicit GEMM --------------------------------------------------------------------------------------------------------------
class Geo:
    """(mode, G, Bg, Hi, Cin, Ho, N, stride, offset) as in IGEMM_CASES, or with both extents
    (mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, stride, offset)."""

    def __init__(self, case):
        if len(case) == 9:
            m, G, Bg, Hi, Cin, Ho, N, s, o = case
            case = (m, G, Bg, Hi, Hi, Cin, Ho, Ho, N, s, o)
        self.mode, self.G, self.Bg, self.Hi, self.Wi, self.Cin, self.Ho, self.Wo, self.N, self.stride, self.offset = case
        self.Bt = self.G * self.Bg
        self.taps = 1 if self.mode in (DENSE, IM2COL3) else 16
        self.rows = self.Bt * self.Ho * self.Wo
        self.K = 48 if self.mode == IM2COL3 else self.Cin            # real channels of the gathered operand
        self.a_shape = (self.Bt, 3, self.Hi, self.Wi) if self.mode == IM2COL3 else (self.Bt * self.Hi * self.Wi, self.Cin)
        self.dims = (self.mode, self.G, self.Bg, self.Hi, self.Wi, self.Cin, self.Ho, self.Wo, self.N)


def igemm_ref(g, A, Bp):
    """fp64 ATen: [rows][N] of A (NHWC rows, or the NCHW image of IM2COL3) and packed weights Bp [taps][N][Cin]."""
    A, Bp = A.double(), Bp.double().reshape(g.taps, g.N, g.Cin)
    if g.mode == DENSE:
        return F.linear(A.reshape(-1, g.Cin), Bp[0])
    if g.mode == IM2COL3:
        y = F.conv2d(A.reshape(g.Bt, 3, g.Hi, g.Wi), Bp[0][:, :48].reshape(g.N, 3, 4, 4), stride=2, padding=1)
    else:
        x = A.reshape(g.Bt, g.Hi, g.Wi, g.Cin).permute(0, 3, 1, 2)
        W = Bp.reshape(4, 4, g.N, g.Cin)
        if g.mode == CONV:             # Bp[kh*4+kw][n][ci] = W[n][ci][kh][kw]
            y = F.conv2d(x, W.permute(2, 3, 0, 1), stride=g.stride, padding=-g.offset)
        else:                          # Bp[kh*4+kw][n][ci] = W[ci][n][kh][kw] of the ConvTranspose2d
            s, p = (2, 1) if g.mode == TCONV_S2P1 else (1, 0)
            y = F.conv_transpose2d(x, W.permute(3, 2, 0, 1), stride=s, padding=p)
    assert tuple(y.shape[2:]) == (g.Ho, g.Wo), (tuple(y.shape), g.Ho, g.Wo)
    return y.permute(0, 2, 3, 1).reshape(-1, g.N)


def int_operands(g, seed, sparse):
    """(A, Bp): [-3, 3] everywhere, or {-1, 0, 1} thinned so that the BatchNorm sums of the case stay far below 2^24."""
    if not sparse:
        A, Bp = ints(g.a_shape, seed), ints((g.taps, g.N, g.Cin), seed + 1)
    else:
        rpg = g.rows // g.G
        d = min(0.25, (float(1 << 20) / (rpg * g.taps * g.K)) ** 0.5)        # rows * E[y^2] = rows * K * d^2 <= 2^20
        A, Bp = ints(g.a_shape, seed, 1, d), ints((g.taps, g.N, g.Cin), seed + 1, 1, d)
    if g.mode == IM2COL3:
        Bp[:, :, 48:] = 0
    return A, Bp


def assert_int_exact(g, A, Bp, bias=None, out16=None, stats=False):
    """The exactness preconditions, on the reference alone; returns the fp64 reference (+ bias)."""
    mag = igemm_ref(g, A.abs(), Bp.abs()) + (0 if bias is None else bias.abs().double())
    assert float(mag.max()) < LIMIT, f"broken case: sum |a||b| reaches {float(mag.max())} >= 2^24"
    ref = igemm_ref(g, A, Bp) + (0 if bias is None else bias.double())
    if out16 is not None:
        assert float(ref.abs().max()) <= INT_MAX_16[out16], f"broken case: |C| reaches {float(ref.abs().max())} in a {out16} output"
    if stats:
        r = ref.reshape(g.G, -1, g.N)
        assert float(r.abs().sum(1).max()) < LIMIT and float((r * r).sum(1).max()) < LIMIT, "broken case: BatchNorm sums reach 2^24"
    return ref


def stats_ref(g, ref):
    r = ref.reshape(g.G, -1, g.N)
    return torch.stack([r.sum(1), (r * r).sum(1)], 1)           # [G][2][N]


def onehot_weights(g, s):
    """Weight set s: column n is non-zero at exactly one (tap, ci), value +-2^k.  -> (Bp [taps][N][Cin], tap [N], ci [N], scale [N])"""
    n = torch.arange(g.N)
    ksteps = -(-g.K // 32)
    tap = (n + 5 * s) % g.taps
    kstep = (n // g.taps + (n if g.taps > 1 else 0) + 3 * s) % ksteps
    width = torch.full((g.N,), 32) if g.K % 32 == 0 else torch.where(kstep == ksteps - 1, g.K % 32, 32)
    ci = kstep * 32 + torch.randint(0, 1 << 16, (g.N,), generator=_gen(100 + s)) % width
    scale = pow2(g.N, 200 + s)
    Bp = torch.zeros(g.taps, g.N, g.Cin)
    Bp[tap, n, ci] = scale
    return Bp, tap, ci, scale


def assert_coverage(g, sets):
    """Over the weight sets of a case every tap and every 32-channel K-step is hit by at least one column."""
    taps = torch.cat([t for _, t, _, _ in sets]).unique()
    ksteps = (torch.cat([c for _, _, c, _ in sets]) // 32).unique()
    assert taps.numel() == g.taps and ksteps.numel() == -(-g.K // 32), (taps.tolist(), ksteps.tolist())


def select_ref(g, A, tap, ci, scale):
    """[rows][N] fp32: C[pixel][n] = scale[n] * A[pixel shifted by tap[n]][ci[n]], +0 where the tap falls into the padding."""
    A = A.float()
    if g.mode == DENSE:
        return A.reshape(-1, g.Cin)[:, ci] * scale
    oy, ox = torch.arange(g.Ho)[:, None], torch.arange(g.Wo)[:, None]
    if g.mode == IM2COL3:              # virtual channel k = c*16 + kh*4 + kw of the NCHW image, k4 s2 p1 window
        kh, kw, ch = (ci >> 2) & 3, ci & 3, ci >> 4
        A4 = A.reshape(g.Bt, 3, g.Hi, g.Wi).permute(0, 2, 3, 1)
        iy, ix, vy, vx = 2 * oy - 1 + kh, 2 * ox - 1 + kw, True, True
    else:
        kh, kw, ch = tap >> 2, tap & 3, ci
        A4 = A.reshape(g.Bt, g.Hi, g.Wi, g.Cin)
        if g.mode == CONV:
            iy, ix, vy, vx = oy * g.stride + g.offset + kh, ox * g.stride + g.offset + kw, True, True
        elif g.mode == TCONV_S2P1:     # oy = 2 iy - 1 + kh
            ty, tx = oy + 1 - kh, ox + 1 - kw
            iy, ix, vy, vx = ty // 2, tx // 2, ty % 2 == 0, tx % 2 == 0
        else:                          # TCONV_S1P0: oy = iy + kh
            iy, ix, vy, vx = oy - kh, ox - kw, True, True
    vy = vy & (iy >= 0) & (iy < g.Hi)
    vx = vx & (ix >= 0) & (ix < g.Wi)
    val = A4[:, iy.clamp(0, g.Hi - 1)[:, None, :], ix.clamp(0, g.Wi - 1)[None, :, :], ch[None, None, :]]     # [Bt][Ho][Wo][N]
    val = torch.where((vy[:, None, :] & vx[None, :, :])[None], val * scale, torch.zeros(()))
    return val.reshape(-1, g.N)


def operand_dtype(be):
    """The type the matrix cores round their operands to in the backend's precision mode (None: fp32)."""
    return {"fp32": None, "bf16": torch.bfloat16, "bf16s": torch.bfloat16}.get(be.precision, torch.float16)


def _dev(t, dev):
    return None if t is None else t.to(dev)


def run_igemm(be, dev, case, family, ld_extra=0, store=None, prep=None, planes=False, all16=False, mixed=False, what=""):
    """One case on one backend / route.  store: the 16-bit storage type of A and C (the "bf16s" / "fp16s" modes; the NCHW image of
    MMDYN_IM2COL3 stays fp32: the first layer of the storage modes); ld_extra: ldc - N (fp32 outputs); prep(A, Bp) -> operands as
    the launch takes them (planes: as ops.Planes); all16: the packed weights are stored in the 16-bit type as well; mixed (with
    store, family A): the mixed-output form only -- C stays fp32, C_act alone is 16-bit (storage flag bit 6), ReLU so that it
    stays exact.  Returns the number of launches."""
    g = Geo(case)
    h = operand_dtype(be)
    assert not mixed or (store is not None and family == "A")
    c_dtype = torch.float32 if mixed else store or torch.float32
    ca_dtype = store or torch.float32
    ldc = g.N + ld_extra
    what = f"{what}{case} family {family}"
    T = be.igemm_stat_tiles(*g.dims, **({"planes": True} if planes else {"all16": True} if all16 else {}))
    prep = prep or (lambda a, b: (a, b))

    def launch(A, Bp, bias, act, want_stats):
        a, b = prep(_dev(A.to(store) if store and g.mode != IM2COL3 else A, dev), _dev(Bp, dev))
        C = Guarded(g.rows, g.N, c_dtype, dev, ldc)
        Ca = Guarded(g.rows, g.N, ca_dtype, dev, ldc) if act else None
        st = Guarded(g.G * T * 2, g.N, torch.float32, dev) if want_stats else None
        be.igemm_nt(a, b, _dev(bias, dev), C.t, Ca.t if act else None, st.view(g.G, T, 2, g.N) if want_stats else None, None,
                    *g.dims, ldc, g.stride, g.offset, act, 1)
        if torch.device(dev).type == "cuda":
            torch.cuda.synchronize()
        for o, name in ((C, "C"), (Ca, "C_act"), (st, "stats")):
            if o is not None:
                o.check(f"{what}: {name}")
        return C, Ca, st

    key = (tuple(case), family, store, h)
    if key not in _JOBS:
        _JOBS[key] = igemm_jobs(g, family, store, h)
    jobs = _JOBS[key]
    if mixed:       # the job with a second output, with its bias and without (the specialised first-layer kernel declines a bias)
        jobs = [j for j in jobs if j[3]]
        jobs = jobs + [(A, Bp, None, act, ws_, ref - bias, label + ", bias dropped") for A, Bp, bias, act, ws_, ref, label in jobs]
        assert len(jobs) == 2 and float(jobs[1][5].abs().max()) <= INT_MAX_16[store]
    for A, Bp, bias, act, want_stats, ref, label in jobs:
        C, Ca, st = launch(A, Bp.to(store) if all16 else Bp, bias, act, want_stats)
        check_exact(C.values(), ref, f"{what}: C ({label})", bitwise=family == "B")
        if Ca is not None:
            check_exact(Ca.values(), ref.clamp_min(0), f"{what}: C_act (ReLU; {label})")
        if st is not None:
            check_exact(st.values().double().reshape(g.G, T, 2, g.N).sum(1).reshape(-1, g.N), stats_ref(g, ref.double()).reshape(-1, g.N),
                        f"{what}: stats summed over the {T} tiles, rows (group, sum | sum of squares)")
    return len(jobs)


_JOBS = {}      # (case, family, storage type, operand type) -> the launches of the case with their references, shared by the routes


def igemm_jobs(g, family, store, h):
    """[(A, Bp, bias, act, want_stats, reference [rows][N] fp32, label)]: built once per case, left unchanged."""
    if family == "A":
        # sparse {-1, 0, 1}: plain output + BatchNorm partial sums; then integer bias + ReLU second output
        A, Bp = int_operands(g, 11, sparse=True)
        jobs = [(A, Bp, None, 0, True, assert_int_exact(g, A, Bp, out16=store, stats=True).float(), "sparse integers")]
        A, Bp = int_operands(g, 13, sparse=store is not None)
        bias = ints((g.N,), 15, 1 if store else 5)
        return jobs + [(A, Bp, bias, 2, False, assert_int_exact(g, A, Bp, bias=bias, out16=store).float(), "integers + bias")]
    sets = [onehot_weights(g, s) for s in range(2 if g.N >= 64 or g.taps * g.K <= 64 else 3)]
    assert_coverage(g, sets)
    A = arbitrary(g.a_shape, 17, BINADES[h])
    assert bool((A != 0).all()) and float(A.abs().min()) >= 2.0 ** -126
    Ar = A.to(h).float() if h is not None and g.mode != IM2COL3 else A       # what the matrix cores multiply (RNE)
    return [(A, Bp, None, 0, False, select_ref(g, Ar, tap, ci, scale), f"weight set {s}") for s, (Bp, tap, ci, scale) in enumerate(sets)]


def run_dgrad_relu(be, dev, case, store=None, what=""):
    """mmdyn_igemm_nt_dgrad_act with ReLU on integers: C = acc * [u > 0], u an integer tensor that contains zeros.  store: A, u and
    C are stored in that 16-bit type (thinned {-1, 0, 1} operands, so that every |C| stays an exact integer of the type)."""
    g = Geo(case)
    A, Bp = int_operands(g, 21, sparse=store is not None)
    ref = assert_int_exact(g, A, Bp, out16=store)
    u = ints((g.rows, g.N), 23, 2)
    assert bool((u == 0).any())
    cast = (lambda t: t.to(store)) if store else (lambda t: t)
    C = Guarded(g.rows, g.N, store or torch.float32, dev)
    be.igemm_nt_dgrad_act(_dev(cast(A), dev), _dev(Bp, dev), C.t, _dev(cast(u), dev), 2, *g.dims, g.stride, g.offset)
    C.check(f"{what}{case}: dgrad_act C")
    check_exact(C.values(), ref * (u > 0), f"{what}{case}: dgrad_act (ReLU) C")


def run_splitk(be, dev, rows, K, N, splitk, family, what=""):
    """Split-K workspace + mmdyn_splitk_reduce (integer bias and ReLU second output in the reduce)."""
    g = Geo((DENSE, 1, rows, 1, K, 1, N, 1, 0))
    what = f"{what}split-K rows={rows} K={K} N={N} splitk={splitk} family {family}"
    bias = ints((N,), 35, 5)
    if family == "A":
        A, Bp = int_operands(g, 31, sparse=False)
        jobs = [(Bp, assert_int_exact(g, A, Bp, bias=bias))]
    else:
        A = arbitrary(g.a_shape, 33)
        sets = [onehot_weights(g, s) for s in range(2)]
        assert_coverage(g, sets)
        jobs = [(Bp, select_ref(g, A, tap, ci, scale)) for Bp, tap, ci, scale in sets]
    for Bp, want in jobs:
        ws, C, Ca = Guarded(splitk * rows, N, torch.float32, dev), Guarded(rows, N, torch.float32, dev), Guarded(rows, N, torch.float32, dev)
        be.igemm_nt(_dev(A, dev), _dev(Bp, dev), None, C.t, None, None, ws.view(splitk, rows, N), DENSE, 1, rows, 1, 1, K, 1, 1, N, N,
                    1, 0, 0, splitk)
        ws.check(f"{what}: ws")
        check_exact(ws.values().double().reshape(splitk, rows, N).sum(0).float(), want - (bias if family == "A" else 0),
                    f"{what}: ws summed over the {splitk} slices", bitwise=family == "B")
        be.splitk_reduce(ws.view(splitk, rows, N), _dev(bias, dev) if family == "A" else None, C.t, Ca.t, splitk, rows, N, 2)
        for o, name in ((C, "C"), (Ca, "C_act")):
            o.check(f"{what}: {name}")
        check_exact(C.values(), want, f"{what}: C", bitwise=family == "B")
        if family == "A":
            check_exact(Ca.values(), want.clamp_min(0), f"{what}: C_act (ReLU)")


def run_grouped(be, dev, G, rows, K, N, family, store=None, what=""):
    """mmdyn_igemm_nt_grouped: every group multiplies its OWN weights (a wrong b_group_stride shows) and adds its own bias.
    store: A, C and C_act are stored in that 16-bit type (family A then draws from {-1, 0, 1})."""
    what = f"{what}grouped G={G} rows={rows} K={K} N={N} family {family}" + (f" {store}" if store else "")
    g1 = Geo((DENSE, 1, rows, 1, K, 1, N, 1, 0))
    h = operand_dtype(be)
    cast = (lambda t: t.to(store)) if store else (lambda t: t)
    if family == "A":
        mag = 1 if store else 3
        A, Bp, bias = ints((G * rows, K), 41, mag), ints((G, N, K), 42, mag), ints((G, N), 43, 1 if store else 5)
        want = torch.cat([assert_int_exact(g1, A[i * rows:(i + 1) * rows], Bp[i], bias=bias[i], out16=store) for i in range(G)])
        assert G == 1 or not torch.equal(Bp[0], Bp[1])
        jobs = [(Bp, bias, want)]
    else:
        A = arbitrary((G * rows, K), 44, BINADES[h])
        Ar = A.to(h).float() if h is not None else A
        jobs = []
        for s in range(2):
            per = [onehot_weights(g1, s + 2 * i) for i in range(G)]
            jobs.append((torch.stack([p[0][0] for p in per]), None,
                         torch.cat([select_ref(g1, Ar[i * rows:(i + 1) * rows], *per[i][1:]) for i in range(G)])))
    for Bp, bias, want in jobs:
        C = Guarded(G * rows, N, store or torch.float32, dev)
        Ca = Guarded(G * rows, N, store or torch.float32, dev) if family == "A" else None
        be.igemm_nt_grouped(_dev(cast(A), dev), _dev(Bp, dev), _dev(bias, dev), C.t, Ca.t if Ca else None, None, G, rows, K, N, 2)
        C.check(f"{what}: C")
        check_exact(C.values(), want, f"{what}: C", bitwise=family == "B")
        if Ca:
            Ca.check(f"{what}: C_act")
            check_exact(Ca.values(), want.clamp_min(0), f"{what}: C_act (ReLU)")


# ---- weight gradient ------------------------------------------------------------------------------------------------------------
class WGeo:
    """(mode, Bt, Hr, Cd, Hi, Cg, stride, offset, cg_canon, perm) as in WGRAD_CASES, or with both extents
    (mode, Bt, Hr, Wr, Cd, Hi, Wi, Cg, stride, offset, cg_canon, perm)."""

    def __init__(self, case):
        if len(case) == 10:
            m, Bt, Hr, Cd, Hi, Cg, s, o, cgc, perm = case
            case = (m, Bt, Hr, Hr, Cd, Hi, Hi, Cg, s, o, cgc, perm)
        self.mode, self.Bt, self.Hr, self.Wr, self.Cd, self.Hi, self.Wi, self.Cg, self.stride, self.offset, cgc, self.perm = case
        self.cgc = self.Cg if cgc is None else cgc
        self.rows = self.Bt * self.Hr * self.Wr
        self.taps = 16 if self.mode == CONV else 1
        self.g_shape = (self.Bt, 3, self.Hi, self.Wi) if self.mode == IM2COL3 else (self.Bt * self.Hi * self.Wi, self.Cg)
        self.dims = (self.mode, self.Bt, self.Hr, self.Wr, self.Cd, self.Hi, self.Wi, self.Cg, self.stride, self.offset)


def wgrad_ref(w, D, Gt):
    """fp64 [taps][Cd][Cg]: sum over the rows of D[row][cd] * G_tap[row][cg] -- for the convolution modes the autograd weight
    gradient of F.conv2d (D = dL/dy of Conv2d(Cg -> Cd, k4, stride, pad = -offset), Gt its input)."""
    D, Gt = D.double(), Gt.double()
    if w.mode == DENSE:
        return (D.reshape(w.rows, w.Cd).t() @ Gt.reshape(w.rows, w.Cg))[None]
    dy = D.reshape(w.Bt, w.Hr, w.Wr, w.Cd).permute(0, 3, 1, 2)
    if w.mode == IM2COL3:
        x, cin, s, p = Gt.reshape(w.Bt, 3, w.Hi, w.Wi), 3, 2, 1
    else:
        x, cin, s, p = Gt.reshape(w.Bt, w.Hi, w.Wi, w.Cg).permute(0, 3, 1, 2), w.Cg, w.stride, -w.offset
    W = torch.zeros(w.Cd, cin, 4, 4, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, W, stride=s, padding=p)
    assert tuple(y.shape[2:]) == (w.Hr, w.Wr), (tuple(y.shape), w.Hr, w.Wr)
    (gW,) = torch.autograd.grad(y, W, dy)
    if w.mode == IM2COL3:              # column k = ci*16 + kh*4 + kw, columns 48..63 zero
        out = torch.zeros(1, w.Cd, 64, dtype=torch.float64)
        out[0, :, :48] = gW.reshape(w.Cd, 48)
        return out
    return gW.reshape(w.Cd, w.Cg, 16).permute(2, 0, 1)


def canon_ref(w, s):
    """The canonical layout mmdyn_wgrad_reduce writes, of s [taps][Cd][Cg] (index arithmetic of include/mmdyn_hip.h)."""
    s = s[:, :, :w.cgc]
    if w.perm == 0:                    # canon[cd][cg][tap]
        return s.permute(1, 2, 0).reshape(-1)
    if w.perm == 1:                    # cg = hw*256 + c -> canon[cd][c*25 + hw]
        return s[0].reshape(w.Cd, 25, 256).permute(0, 2, 1).reshape(-1)
    return s[0].reshape(25, 256, w.cgc).permute(1, 0, 2).reshape(-1)        # cd = hw*256 + c -> canon[c*25 + hw][cg]


def onehot_rows(w, s):
    """Dense operand D, one-hot per output row cd: D[row(cd)][cd] = +-2^k, the rows spread over the whole row range (every chunk)."""
    cd = torch.arange(w.Cd)
    row = (cd * w.rows // w.Cd + 17 * s + cd % 3) % w.rows
    scale = pow2(w.Cd, 300 + s)
    D = torch.zeros(w.rows, w.Cd)
    D[row, cd] = scale
    return D, row, scale


def onehot_pixels(w, s):
    """Gathered operand Gt, one-hot per output column cg: Gt[pixel(cg)][cg] = +-2^k (DENSE / CONV)."""
    cg = torch.arange(w.Cg)
    npix = w.Bt * w.Hi * w.Wi
    pix = (cg * npix // w.Cg + 29 * s + cg % 5) % npix
    scale = pow2(w.Cg, 400 + s)
    Gt = torch.zeros(npix, w.Cg)
    Gt[pix, cg] = scale
    return Gt, pix, scale


def wgrad_select_ref(w, D=None, row=None, Gt=None, pix=None, scale=None):
    """[taps][Cd][Cg] fp32 of a one-hot D (row, scale per cd) against an arbitrary Gt, or of an arbitrary D against a one-hot Gt
    (pix, scale per cg): one element of the other operand times a power of two, +0 where the tap falls into the padding."""
    kh, kw = torch.arange(w.taps) >> 2, torch.arange(w.taps) & 3
    if row is not None:                # out[t][cd][:] = scale[cd] * G_tap[row[cd]][:]
        if w.mode == DENSE:
            return (Gt.reshape(w.rows, w.Cg)[row] * scale[:, None])[None]
        b, p = row // (w.Hr * w.Wr), row % (w.Hr * w.Wr)
        if w.mode == IM2COL3:          # column k = c*16 + kh*4 + kw of the k4 s2 p1 window of the NCHW image, k >= 48 zero
            k = torch.arange(48)
            y = (2 * (p // w.Wr) - 1)[:, None] + ((k >> 2) & 3)[None, :]        # [Cd][48]
            x = (2 * (p % w.Wr) - 1)[:, None] + (k & 3)[None, :]
            ok = (y >= 0) & (y < w.Hi) & (x >= 0) & (x < w.Wi)
            v = Gt.reshape(w.Bt, 3, w.Hi, w.Wi)[b[:, None], (k >> 4)[None, :], y.clamp(0, w.Hi - 1), x.clamp(0, w.Wi - 1)]
            out = torch.zeros(1, w.Cd, 64)
            out[0, :, :48] = torch.where(ok, v * scale[:, None], torch.zeros(()))
            return out
        y = (p // w.Wr * w.stride + w.offset)[None, :] + kh[:, None]            # [taps][Cd]
        x = (p % w.Wr * w.stride + w.offset)[None, :] + kw[:, None]
        ok = (y >= 0) & (y < w.Hi) & (x >= 0) & (x < w.Wi)
        v = Gt.reshape(w.Bt, w.Hi, w.Wi, w.Cg)[b[None, :], y.clamp(0, w.Hi - 1), x.clamp(0, w.Wi - 1)]      # [taps][Cd][Cg]
        return torch.where(ok[:, :, None], v * scale[None, :, None], torch.zeros(()))
    if w.mode == DENSE:                # out[0][:][cg] = scale[cg] * D[pix[cg]][:]
        return (D.reshape(w.rows, w.Cd)[pix] * scale[:, None]).t()[None]
    b, p = pix // (w.Hi * w.Wi), pix % (w.Hi * w.Wi)
    ty = (p // w.Wi - w.offset)[None, :] - kh[:, None]                          # iy = r*stride + offset + kh
    tx = (p % w.Wi - w.offset)[None, :] - kw[:, None]
    r, c = ty // w.stride, tx // w.stride
    ok = (ty % w.stride == 0) & (tx % w.stride == 0) & (r >= 0) & (r < w.Hr) & (c >= 0) & (c < w.Wr)
    v = D.reshape(w.Bt, w.Hr, w.Wr, w.Cd)[b[None, :], r.clamp(0, w.Hr - 1), c.clamp(0, w.Wr - 1)]            # [taps][Cg][Cd]
    return torch.where(ok[:, :, None], v * scale[None, :, None], torch.zeros(())).permute(0, 2, 1)


_WJOBS = {}     # (case, family, operand type) -> the launches of a weight-gradient case with their references, built once


def wgrad_jobs(w, family, h):
    """[(D, Gt, reference [taps][Cd][Cg])] of one case; h: the type the arbitrary operand of family B is rounded to."""
    if family == "A":
        D, Gt = ints((w.rows, w.Cd), 51), ints(w.g_shape, 52)
        mag = wgrad_ref(w, D.abs(), Gt.abs())
        assert float(mag.max()) < LIMIT, f"broken case: sum |d||g| reaches {float(mag.max())} >= 2^24"
        jobs = [(D, Gt, wgrad_ref(w, D, Gt))]
    else:
        jobs = []
        Gt, D = arbitrary(w.g_shape, 53, BINADES[h]), arbitrary((w.rows, w.Cd), 54, BINADES[h])
        r16 = (lambda t: t.to(h).float()) if h is not None else (lambda t: t)
        if w.mode == IM2COL3:
            Gt = r16(Gt)
        for s in range(2):
            Ds, row, sc = onehot_rows(w, s)
            jobs.append((Ds, Gt, wgrad_select_ref(w, Gt=r16(Gt), row=row, scale=sc)))
            if w.mode == IM2COL3:      # (the gathered operand is the NCHW image: the one-hot D direction only)
                continue
            Gs, pix, sc = onehot_pixels(w, s)
            jobs.append((D, Gs, wgrad_select_ref(w, D=r16(D), pix=pix, scale=sc)))
        hit = torch.cat([j[0].nonzero()[:, 0] for j in jobs if j[1] is Gt])     # the one-hot rows reach both ends of the row range
        assert int(hit.min()) <= w.rows // 4 and int(hit.max()) >= 3 * (w.rows - 1) // 4
    return jobs


def run_wgrad(be, dev, case, family, prep=None, planes=(False, False), store=(None, None), what=""):
    """mmdyn_wgrad_tn (partial summed over the chunks on the host in fp64), then mmdyn_wgrad_reduce with the case's permutation and
    cg_canon, beta = 0 and the accumulate form.  store = (type of D, type of Gt) in HBM, None: fp32 -- both 16-bit, D only or Gt
    only (under "bf16s" / "fp16s" the six storage instances of wgrad_tn.hip; MMDYN_IM2COL3 takes a 16-bit D only, its gathered
    operand is the fp32 image).  Integers up to 3 and +-2^k are exact in either type; the arbitrary operand of family B is the
    RNE-rounded one whichever operand is stored in 16 bits, as in the 16-bit matrix-core modes."""
    w = WGeo(case)
    assert store[1] is None or w.mode != IM2COL3
    h = operand_dtype(be) if w.mode != IM2COL3 else store[0]        # (a 16-bit D: the image may or may not be rounded on the way
    what = f"{what}{case} family {family}" + (f" store {store}" if any(store) else "")     # into the matrix cores -- it is given rounded)
    assert all(s in (None, operand_dtype(be)) for s in store)
    to_store = lambda d, g: (d.to(store[0]) if store[0] else d, g.to(store[1]) if store[1] else g)
    prep = prep or to_store
    chunks = be.wgrad_chunks(w.mode, w.rows, w.Cd, w.Cg, planes) if any(planes) else be.wgrad_chunks(w.mode, w.rows, w.Cd, w.Cg)
    assert chunks % 4 == 0
    key = (tuple(case), family, h if family == "B" else None)
    if key not in _WJOBS:
        _WJOBS[key] = wgrad_jobs(w, family, h)
    jobs = _WJOBS[key]
    bitwise = family == "B"
    for k, (D, Gt, want) in enumerate(jobs):
        d, gt = prep(_dev(D, dev), _dev(Gt, dev))
        P = Guarded(chunks * w.taps * w.Cd, w.Cg, torch.float32, dev)
        be.wgrad_tn(d, gt, P.view(chunks, w.taps, w.Cd, w.Cg), *w.dims, chunks)
        P.check(f"{what}: partial")
        got = P.values().double().reshape(chunks, w.taps, w.Cd, w.Cg).sum(0)
        check_exact(got.float().reshape(-1, w.Cg), want.reshape(-1, w.Cg), f"{what}: partial summed over {chunks} chunks (job {k}), "
                    f"rows (tap, cd)", bitwise=bitwise)
        canon = Guarded(w.Cd * w.taps, w.cgc, torch.float32, dev)
        be.wgrad_reduce(P.view(chunks, w.taps, w.Cd, w.Cg), canon.t, chunks, w.taps, w.Cd, w.Cg, w.cgc, w.perm, 0.0)
        canon.check(f"{what}: canon")
        cref = canon_ref(w, want)
        check_exact(canon.values().reshape(-1), cref, f"{what}: canon (perm {w.perm}, cg_canon {w.cgc}, job {k})", bitwise=bitwise)
        be.wgrad_reduce(P.view(chunks, w.taps, w.Cd, w.Cg), canon.t, chunks, w.taps, w.Cd, w.Cg, w.cgc, w.perm, 1.0)
        canon.check(f"{what}: canon (beta = 1)")
        check_exact(canon.values().reshape(-1), 2 * cref, f"{what}: canon accumulated (beta = 1, job {k})", bitwise=bitwise)


def wgrad_pairs(cases):
    """(case, family) pairs."""
    return [(c, f) for c in cases for f in ("A", "B")]


def run_wgrad_grouped(be, dev, G, rows, Cd, Cg, family, store=(None, None), what=""):
    """mmdyn_wgrad_tn_grouped: partial [chunks][G][Cd][Cg], one reduce over Cd' = G * Cd.  store = (type of D, type of Gt) in HBM
    as in run_wgrad; the grouped launch takes ONE 16-bit operand (both: MMDYN_ERR_SHAPE, include/mmdyn_hip.h)."""
    what = f"{what}grouped wgrad G={G} rows={rows} Cd={Cd} Cg={Cg} family {family}" + (f" store {store}" if any(store) else "")
    assert all(s in (None, operand_dtype(be)) for s in store) and not all(store)
    w = WGeo((DENSE, rows, 1, Cd, 1, Cg, 1, 0, None, 0))
    h = operand_dtype(be)
    chunks = be.wgrad_chunks(DENSE, rows, Cd, Cg)
    if family == "A":
        D, Gt = ints((G * rows, Cd), 61), ints((G * rows, Cg), 62)
        want = torch.cat([wgrad_ref(w, D[i * rows:(i + 1) * rows], Gt[i * rows:(i + 1) * rows]) for i in range(G)])
        assert float(torch.cat([wgrad_ref(w, D[i * rows:(i + 1) * rows].abs(), Gt[i * rows:(i + 1) * rows].abs()) for i in range(G)]).max()) < LIMIT
    else:
        Gt = arbitrary((G * rows, Cg), 63, BINADES[h])
        Gr = Gt.to(h).float() if h is not None else Gt
        per = [onehot_rows(w, i) for i in range(G)]
        D = torch.cat([p[0] for p in per])
        want = torch.cat([wgrad_select_ref(w, Gt=Gr[i * rows:(i + 1) * rows], row=per[i][1], scale=per[i][2]) for i in range(G)])
    P = Guarded(chunks * G * Cd, Cg, torch.float32, dev)
    be.wgrad_tn_grouped(_dev(D.to(store[0]) if store[0] else D, dev), _dev(Gt.to(store[1]) if store[1] else Gt, dev),
                        P.view(chunks, G, Cd, Cg), G, rows, Cd, Cg, chunks)
    P.check(f"{what}: partial")
    check_exact(P.values().double().reshape(chunks, G * Cd, Cg).sum(0).float(), want.reshape(G * Cd, Cg), f"{what}: partial summed",
                bitwise=family == "B")
    canon = Guarded(G * Cd, Cg, torch.float32, dev)
    be.wgrad_reduce(P.view(chunks, 1, G * Cd, Cg), canon.t, chunks, 1, G * Cd, Cg, Cg, 0, 0.0)
    canon.check(f"{what}: canon")
    check_exact(canon.values(), want.reshape(G * Cd, Cg), f"{what}: canon [G][Cd][Cg]", bitwise=family == "B")


# ---- direct kernels -------------------------------------------------------------------------------------------------------------
def out3_weight_sets():
    """The six selection weight sets of the last decoder layer, [(w [32][3][4][4], tap [3], ci [3], scale [3])]: output channel co
    of set s selects one (ci, kh, kw) with value +-2^k; co + 3 s covers the 16 taps in 6 sets."""
    sets, taps = [], set()
    for s in range(6):
        tap, ci, scale = (torch.arange(3) + 3 * s) % 16, (torch.arange(3) * 11 + 5 * s) % 32, pow2(3, 500 + s)
        w = torch.zeros(32, 3, 4, 4)
        w[ci, torch.arange(3), tap >> 2, tap & 3] = scale
        sets.append((w, tap, ci, scale))
        taps |= set(tap.tolist())
    assert len(taps) == 16
    return sets


def run_tconv_out3(be, dev, Bt, Hi, Wi, family, store=None, what=""):
    """mmdyn_tconv_out3_fwd: ConvTranspose2d(32, 3, 4, 2, 1) of an NHWC activation, NCHW logits.  store: the activation is stored
    in that 16-bit type (mmdyn_tconv_out3_fwd_b16; the arbitrary activation of family B is then one of its values); weights and
    logits stay fp32."""
    what = f"{what}tconv_out3_fwd Bt={Bt} {Hi}x{Wi} family {family}" + (f" {store}" if store else "")
    if family == "A":
        a, ws = ints((Bt * Hi * Wi, 32), 71), [ints((32, 3, 4, 4), 72)]
        x = a.double().reshape(Bt, Hi, Wi, 32).permute(0, 3, 1, 2)
        assert float(F.conv_transpose2d(x.abs(), ws[0].double().abs(), stride=2, padding=1).max()) < LIMIT
        wants = [F.conv_transpose2d(x, ws[0].double(), stride=2, padding=1)]
    else:                              # the six selection sets: every logit is one activation times +-2^k, or +0 in the padding
        a, ws, wants = arbitrary((Bt * Hi * Wi, 32), 73, BINADES[store]), [], []
        a = a.to(store).float() if store else a
        g = Geo((TCONV_S2P1, 1, Bt, Hi, Wi, 32, 2 * Hi, 2 * Wi, 3, 1, 0))
        for w, tap, ci, scale in out3_weight_sets():
            ws.append(w)
            wants.append(select_ref(g, a, tap, ci, scale).reshape(Bt, 2 * Hi, 2 * Wi, 3).permute(0, 3, 1, 2))
    for w, want in zip(ws, wants):
        out = Guarded(Bt * 3 * 2 * Hi, 2 * Wi, torch.float32, dev)
        be.tconv_out3_fwd(_dev(a.to(store) if store else a, dev), _dev(w, dev), out.t, Bt, Hi, Wi)
        out.check(f"{what}: out")
        check_exact(out.values(), want.reshape(-1, 2 * Wi), f"{what}: logits, rows (sample, channel, y)", bitwise=family == "B")


def run_col2im(be, dev, Bt, Hi, Wi, C, stride, pad, tap_major, ld_extra, family, what=""):
    """mmdyn_col2im_k4: every output pixel is the sum of the (up to 16) column entries that scatter onto it.  Family B: one
    non-zero tap per column-matrix row, so every output element is one input element or +0."""
    what = f"{what}col2im_k4 Bt={Bt} {Hi}x{Wi} C={C} s={stride} p={pad} tap_major={tap_major} family {family}"
    Ho, Wo = (Hi - 1) * stride - 2 * pad + 4, (Wi - 1) * stride - 2 * pad + 4
    ld = 16 * C + ld_extra
    if family == "A":
        cols = [ints((Bt * Hi * Wi, ld), 81)]
    else:                              # set s keeps ONE tap per channel, (c + C s) % 16, in every row: an output element of channel c
        cols, seen = [], set()         # then has at most one term, the input pixel that this tap scatters onto it
        for s in range(-(-16 // C)):
            tap = (torch.arange(C) + C * s) % 16
            seen |= set(tap.tolist())
            keep = torch.zeros(16, C, dtype=torch.bool)
            keep[tap, torch.arange(C)] = True
            col = arbitrary((Bt * Hi * Wi, ld), 82 + s)
            col[:, :16 * C] = torch.where((keep if tap_major else keep.t()).reshape(-1)[None], col[:, :16 * C], torch.zeros(()))
            cols.append(col)
        assert len(seen) == 16
    for col in cols:
        c = col[:, :16 * C].double()
        c = c.reshape(Bt, Hi * Wi, 16, C) if tap_major else c.reshape(Bt, Hi * Wi, C, 16).permute(0, 1, 3, 2)
        img = F.fold(c.permute(0, 3, 2, 1).reshape(Bt, C * 16, Hi * Wi), (Ho, Wo), kernel_size=4, stride=stride, padding=pad)
        want = img.permute(0, 2, 3, 1).reshape(-1, C) if tap_major else img.reshape(-1, Wo)          # img: [Bt][C][Ho][Wo]
        out = Guarded(want.shape[0], want.shape[1], torch.float32, dev)
        be.col2im_k4(_dev(col, dev), out.t, Bt, Hi, Wi, Ho, Wo, C, ld, stride, pad, tap_major)
        out.check(f"{what}: out")
        check_exact(out.values(), want, f"{what}: out", bitwise=family == "B")


# ---- pure sums (family A only) ---------------------------------------------------------------------------------------------------
# G, rows per group, C.  The first four reach the 32-row tile of the column reductions only (csrc/bn.hip, tile_rows_for); the others:
# 64-row tiles with T = 257 and a last tile of one row; 64-row tiles with 4 row lanes, a last tile of 63 rows and a group boundary;
# 96-row tiles; 512-row tiles (four trips of the 4-row unrolled loop with 32 row lanes) with a last tile of one row; 32-row tiles
# with T = 257.  T = 257 takes two slices of the tile sums later.
COLSTATS_SHAPES = [(1, 1, 32), (4, 700, 128), (2, 4097, 64), (3, 255, 256),
                   (1, 16385, 32), (2, 16447, 256), (1, 24576 + 33, 128), (1, 131073, 32), (3, 8224, 64)]
EVAL_TABLE_SHAPES = [(2, 16447, 256), (1, 131073, 32), (3, 8224, 64)]


def _no_junk(P, what):
    """Every element of the declared extent was written: none keeps the sentinel."""
    sentinel = bits(fill_(torch.empty(1, dtype=P.buf.dtype), JUNK))[0]
    left = (bits(P.values()) == sentinel).nonzero()
    assert left.numel() == 0, (f"{what}: {left.numel()} elements of the output were never written, the first at row "
                               f"{int(left[0]) // P.width}, column {int(left[0]) % P.width}")


def run_colstats(be, dev, shape, what=""):
    """mmdyn_colstats on integers: the table summed over its T tiles is the exact column sum of y and of y * y."""
    G, rpg, C = shape
    y = ints((G * rpg, C), 91, 3)
    r = y.double().reshape(G, rpg, C)
    assert float(r.abs().sum(1).max()) < LIMIT and float((r * r).sum(1).max()) < LIMIT
    T = be.colstats_tiles(rpg)
    P = Guarded(G * T * 2, C, torch.float32, dev)
    be.colstats(_dev(y, dev), P.view(G, T, 2, C), G, rpg, C)
    P.check(f"{what}colstats {G, rpg, C}: partial")
    _no_junk(P, f"{what}colstats {G, rpg, C}: partial")
    check_exact(P.values().double().reshape(G, T, 2, C).sum(1).reshape(-1, C), torch.stack([r.sum(1), (r * r).sum(1)], 1).reshape(-1, C),
                f"{what}colstats {G, rpg, C}: partial summed over {T} tiles")


def run_eval_table(be, dev, shape, what=""):
    """The `partial` table of mmdyn_bn_eval_swish_bwd on integers: da_is_du = 1 with integer da, mean = 0 and rstd = 1, so xhat = y
    is an integer and the table summed over its tiles is the exact (sum du, sum du * y); gamma = +-2^k, so dy = du * gamma is exact
    as well."""
    G, rpg, C = shape
    y, da = ints((G * rpg, C), 101, 3), ints((G * rpg, C), 102, 3)
    r, d = y.double().reshape(G, rpg, C), da.double().reshape(G, rpg, C)
    assert float(d.abs().sum(1).max()) < LIMIT and float((d * r).abs().sum(1).max()) < LIMIT
    gamma, beta = pow2(C, 103), ints((C,), 104, 3)
    mean, rstd = torch.zeros(G, C), torch.ones(G, C)
    T = be.colstats_tiles(rpg)
    P, dy = Guarded(G * T * 2, C, torch.float32, dev), Guarded(G * rpg, C, torch.float32, dev)
    be.bn_eval_swish_bwd(_dev(da, dev), _dev(y, dev), _dev(mean, dev), _dev(rstd, dev), _dev(gamma, dev), _dev(beta, dev),
                         dy.view(G * rpg, C), P.view(G, T, 2, C), G, rpg, C, True)
    what = f"{what}bn_eval_swish_bwd {G, rpg, C}"
    P.check(f"{what}: partial")
    dy.check(f"{what}: dy")
    _no_junk(P, f"{what}: partial")
    check_exact(P.values().double().reshape(G, T, 2, C).sum(1).reshape(-1, C), torch.stack([d.sum(1), (d * r).sum(1)], 1).reshape(-1, C),
                f"{what}: partial summed over {T} tiles")
    check_exact(dy.values(), (d * gamma.double()).reshape(-1, C), f"{what}: dy")


def run_sums(be, dev, what=""):
    """mmdyn_colstats, mmdyn_colsum (perm 0 / 2, beta 0 / 1), mmdyn_sum_blocks, mmdyn_dropout_expand / _reduce with p_drop = 0.5
    (the scale 2 is exact), mmdyn_linear_small_fwd / _bwd on integers; the `partial` table of mmdyn_bn_eval_swish_bwd on three of
    the column-statistics shapes."""
    for shape in COLSTATS_SHAPES:
        run_colstats(be, dev, shape, what)
    for shape in EVAL_TABLE_SHAPES:
        run_eval_table(be, dev, shape, what)
    for rows, C, perm in ((1, 32, 0), (300, 512, 0), (1025, 100, 0), (5000, 64, 0), (64, 6400, 2), (7, 6400, 2)):
        x = ints((rows, C), 92, 3)
        s = x.double().sum(0)
        want = s.reshape(25, 256).t().reshape(-1) if perm == 2 else s
        out = Guarded(1, C, torch.float32, dev)
        be.colsum(_dev(x, dev), out.t, rows, C, perm, 0.0)
        out.check(f"{what}colsum {rows, C, perm}: out")
        check_exact(out.values(), want[None], f"{what}colsum rows={rows} C={C} perm={perm} beta=0")
        be.colsum(_dev(x, dev), out.t, rows, C, perm, 1.0)
        out.check(f"{what}colsum {rows, C, perm}: out (beta = 1)")
        check_exact(out.values(), 2 * want[None], f"{what}colsum rows={rows} C={C} perm={perm} beta=1")
    for P_, n in ((1, 4), (4, 999), (7, 4100)):
        x = ints((P_, n), 93, 3)
        out = Guarded(1, n, torch.float32, dev)
        be.sum_blocks(_dev(x, dev), out.t, P_, n)
        out.check(f"{what}sum_blocks {P_, n}: out")
        check_exact(out.values(), x.double().sum(0)[None], f"{what}sum_blocks P={P_} n={n}")
    for P_, B, H in ((4, 37, 512), (1, 1, 512), (3, 5, 260)):
        h, dout = ints((B, H), 94, 3), ints((P_, B, H), 95, 3)
        masks = (torch.rand(P_, B, H, generator=_gen(96)) > 0.5).to(torch.uint8)
        out = Guarded(P_ * B, H, torch.float32, dev)
        be.dropout_expand(_dev(h, dev), _dev(masks, dev), out.view(P_, B, H), P_, B, H, 0.5)
        out.check(f"{what}dropout_expand {P_, B, H}: out")
        check_exact(out.values(), (h.double()[None] * masks.double() * 2).reshape(-1, H), f"{what}dropout_expand P={P_} B={B} H={H}")
        dh = Guarded(B, H, torch.float32, dev)
        be.dropout_reduce(_dev(dout, dev), _dev(masks, dev), dh.view(B, H), P_, B, H, 0.5)
        dh.check(f"{what}dropout_reduce {P_, B, H}: dh")
        check_exact(dh.values(), (dout.double() * masks.double() * 2).sum(0), f"{what}dropout_reduce P={P_} B={B} H={H}")
    for rows, K, N, act in ((33, 7, 512, 2), (33, 512, 7, 0), (1, 7, 32, 2), (130, 64, 7, 0)):
        x, W, b, dy = ints((rows, K), 97), ints((N, K), 98), ints((N,), 99, 5), ints((rows, N), 100)
        assert K * 9 + 5 < LIMIT and rows * 9 < LIMIT and N * 9 < LIMIT
        y = Guarded(rows, N, torch.float32, dev)
        be.linear_small_fwd(_dev(x, dev), _dev(W, dev), _dev(b, dev), y.view(rows, N), rows, K, N, act)
        y.check(f"{what}linear_small_fwd {rows, K, N}: y")
        ref = F.linear(x.double(), W.double(), b.double())
        check_exact(y.values(), ref.clamp_min(0) if act == 2 else ref, f"{what}linear_small_fwd rows={rows} K={K} N={N} act={act}")
        dx, dW, db = Guarded(rows, K, torch.float32, dev), Guarded(N, K, torch.float32, dev), Guarded(1, N, torch.float32, dev)
        be.linear_small_bwd(_dev(dy, dev), _dev(x, dev), _dev(W, dev), dx.view(rows, K), dW.view(N, K), db.view(N), rows, K, N, 0.0)
        for o, name, want in ((dx, "dx", dy.double() @ W.double()), (dW, "dW", dy.double().t() @ x.double()), (db, "db", dy.double().sum(0)[None])):
            o.check(f"{what}linear_small_bwd {rows, K, N}: {name}")
            check_exact(o.values(), want, f"{what}linear_small_bwd rows={rows} K={K} N={N}: {name}")


# ---- case lists -----------------------------------------------------------------------------------------------------------------
# Edges of the routes' tiles (heights 32 / 64 / 128): one row per group, one less than / exactly / one more than a tile multiple, and
# four groups whose boundaries fall inside tiles.
EDGE_CASES = [
    (DENSE, 1, 1, 1, 64, 1, 64, 1, 0),
    (DENSE, 4, 1, 1, 32, 1, 32, 1, 0),
    (DENSE, 1, 127, 1, 64, 1, 128, 1, 0),
    (DENSE, 1, 128, 1, 64, 1, 128, 1, 0),
    (DENSE, 1, 129, 1, 64, 1, 128, 1, 0),
    (DENSE, 4, 33, 1, 96, 1, 64, 1, 0),
    (DENSE, 4, 63, 1, 32, 1, 32, 1, 0),
    (DENSE, 1, 31, 1, 32, 1, 32, 1, 0),
    (DENSE, 1, 65, 1, 64, 1, 64, 1, 0),
    (DENSE, 1, 257, 1, 32, 1, 32, 1, 0),
    (CONV, 4, 1, 8, 128, 5, 128, 1, 0),            # 25 rows per group
    (CONV, 1, 2, 16, 64, 8, 64, 2, -1),            # exactly 128 rows
    (TCONV_S2P1, 4, 1, 8, 128, 16, 64, 1, 0),      # 64 rows per class and group
    (TCONV_S1P0, 4, 1, 5, 256, 8, 128, 1, 0),      # one sample per (pixel, group) tile
    (TCONV_S1P0, 1, 129, 5, 256, 8, 128, 1, 0),
]
# Non-square geometry: mode, G, Bg, Hi, Wi, Cin, Ho, Wo, N, stride, offset
NONSQUARE_CASES = [
    (CONV, 1, 3, 16, 24, 64, 8, 12, 128, 2, -1),
    (CONV, 2, 2, 24, 16, 64, 12, 8, 64, 2, -1),
    (CONV, 1, 3, 8, 11, 128, 5, 8, 128, 1, 0),
    (TCONV_S2P1, 1, 3, 8, 12, 128, 16, 24, 64, 1, 0),
    (TCONV_S2P1, 2, 2, 12, 8, 64, 24, 16, 64, 1, 0),
    (TCONV_S2P1, 1, 2, 16, 32, 64, 32, 64, 32, 1, 0),       # N = 32: the patch-resident kernel declines Hi != Wi
    (DENSE, 1, 2, 3, 5, 64, 3, 5, 64, 1, 0),
    (IM2COL3, 1, 2, 32, 48, 64, 16, 24, 32, 1, 0),
    (IM2COL3, 1, 1, 64, 128, 64, 32, 64, 32, 1, 0),         # the first-layer kernel (conv3.hip) declines Hi != Wi
]
IM2COL3_CASES = [
    (IM2COL3, 1, 3, 32, 64, 16, 32, 1, 0),                  # generic route
    (IM2COL3, 2, 2, 64, 64, 32, 32, 1, 0),                  # the first / last-layer kernels of conv3.hip
]
# mode, Bt, Hr, Wr, Cd, Hi, Wi, Cg, stride, offset, cg_canon, perm
WGRAD_EXTRA = [
    (CONV, 3, 8, 12, 128, 16, 24, 64, 2, -1, None, 0),
    (CONV, 2, 12, 8, 64, 24, 16, 32, 2, -1, None, 0),
    (CONV, 3, 5, 8, 64, 8, 11, 128, 1, 0, None, 0),
    (IM2COL3, 2, 16, 24, 32, 32, 48, 64, 1, 0, 48, 0),
    (IM2COL3, 2, 32, 32, 32, 64, 64, 64, 1, 0, 48, 0),      # conv3.hip
    (IM2COL3, 1, 32, 64, 32, 64, 128, 64, 1, 0, 48, 0),     # conv3.hip declines Hi != Wi
    (DENSE, 1, 1, 1, 32, 1, 1, 32, 1, 0, None, 0),
    (DENSE, 31, 1, 1, 64, 1, 1, 32, 1, 0, None, 0),
    (DENSE, 33, 1, 1, 32, 1, 1, 96, 1, 0, 80, 0),
]
# ---- 16-bit stored operands ("bf16s" / "fp16s") -----------------------------------------------------------------------------------
# weight gradient next to WGRAD_CASES[:7] of tests/test_kernels_gpu.py (channel tiles 128x128, 64x64, 64x32, 32x64, 32x32): the DENSE
# cases of 1 / 31 / 33 rows, the non-square CONV cases and the MMDYN_IM2COL3 cases (16-bit D only; conv3.hip and the generic route)
WGRAD_16 = WGRAD_EXTRA
# G, rows, Cd, Cg / G, rows, K, N: the two smallest shapes of the fp32 tests and a ragged one
WGRAD_GROUPED_16 = [(2, 1, 32, 32), (3, 100, 64, 32), (4, 33, 32, 96)]
GROUPED_16 = [(2, 1, 32, 32), (3, 37, 64, 64), (4, 129, 512, 128)]
TCONV_OUT3_16 = [(2, 16, 16), (1, 16, 32)]
# one case per mode for the mixed-output form (fp32 C, 16-bit C_act)
MIXED_OUT_CASES = [
    (DENSE, 2, 50, 1, 32, 1, 64, 1, 0),
    (CONV, 2, 3, 16, 64, 8, 128, 2, -1),
    (TCONV_S2P1, 2, 3, 16, 64, 32, 32, 1, 0),
    (TCONV_S1P0, 1, 5, 5, 256, 8, 128, 1, 0),
] + IM2COL3_CASES


def wgrad_store(which, t):
    """(type of D, type of Gt) in HBM for `which` in "both" / "D" / "Gt"."""
    return {"both": (t, t), "D": (t, None), "Gt": (None, t)}[which]


def wgrad_store_triples(cases):
    """(case, family, which): every storage combination the entry point takes -- MMDYN_IM2COL3 a 16-bit D only."""
    return [(c, f, wh) for c in cases for f in ("A", "B") for wh in ("both", "D", "Gt") if c[0] != IM2COL3 or wh == "D"]
