"""Plain numpy reference of the on-device noise kernels (csrc/elementwise.hip: random_masks_kernel,
random_normal_kernel) and of the counter accounting of models/vae.py::NoiseSource.

Philox-4x32-10 (Salmon et al., SC'11) on the counter {lo, hi, 0, 0} with the 64-bit seed as the key {lo, hi}.
Element j of a launch at stream position ``offset`` uses counter ``offset + j // 4``, word ``j % 4``.
All integer arithmetic is done in uint64 arrays with 32-bit masking; the uniforms are computed in float32 with the
kernel's three operations in the kernel's order (convert, add 0.5, multiply by 2^-24: an add followed by a multiply
cannot contract to an FMA, so they are bit-exact); Box-Muller is done in float64 on those exact float32 uniforms."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0 = np.uint64(0xD2511F53)
PHILOX_M1 = np.uint64(0xCD9E8D57)
PHILOX_W0 = 0x9E3779B9
PHILOX_W1 = 0xBB67AE85
MASK_SEED_XOR = 0x5DEECE66D          # NoiseSource.keep_mask draws from the stream of seed ^ this
U01_MIN = 2.0 ** -25                 # u01(0)
RADIUS_MAX = 5.8871                  # sqrt(-2 ln 2^-25) = sqrt(50 ln 2) = 5.88705..., rounded up


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def philox4x32_10_full(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on four counter words and two key words (uint64 arrays holding 32-bit values).
    Returns the four output words as uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = (_u64(v) & M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = PHILOX_M0 * c0              # 32 x 32 -> 64 bit products: no overflow in uint64
        p1 = PHILOX_M1 * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(PHILOX_W0)) & M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & M32
    return c0, c1, c2, c3


def philox4x32_10(ctr_lo, ctr_hi, key_lo, key_hi):
    """The kernel's layout: counter {lo, hi, 0, 0}."""
    return philox4x32_10_full(ctr_lo, ctr_hi, 0, 0, key_lo, key_hi)


def words_ref(n4, seed, offset):
    """[n4, 4] uint64: the four words of counters offset .. offset + n4 - 1 (the sum wraps at 2^64 like the kernel's)."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    ctr = np.uint64(offset) + np.arange(n4, dtype=np.uint64)      # uint64 addition wraps
    w = philox4x32_10(ctr & M32, ctr >> np.uint64(32), np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    return np.stack(w, axis=1)


def u01(words):
    """float32 ((float)(x >> 8) + 0.5f) * 2^-24: in (0, 1]; u01(0) = 2^-25, u01(x) = 1.0 for x >> 8 = 2^24 - 1
    (2^24 - 0.5 is not a float32 and rounds to even)."""
    x = (_u64(words) >> np.uint64(8)).astype(np.float32)          # < 2^24: exact
    return (x + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def uniforms_ref(n, seed, offset):
    """float32 [n]: the uniform of every element."""
    return u01(words_ref((n + 3) // 4, seed, offset)).reshape(-1)[:n]


def masks_ref(n, p_drop, seed, offset, uniforms=None):
    """uint8 [n]: 1 where u01 >= p_drop, compared in float32.  ``uniforms``: uniforms_ref(n, seed, offset) if the
    caller already has it (several p_drop on one stream)."""
    u = uniforms_ref(n, seed, offset) if uniforms is None else uniforms
    assert u.dtype == np.float32 and u.shape == (n,)
    return (u >= np.float32(p_drop)).astype(np.uint8)


def normal_ref(n, seed, offset):
    """(z, radius): float64 [n] each.  Words 0, 1 of a counter give z0 = r cos(a), z1 = r sin(a) with
    r = sqrt(-2 ln u01(w0)), a = 2 pi u01(w1); words 2, 3 give z2, z3 the same way."""
    n4 = (n + 3) // 4
    u = u01(words_ref(n4, seed, offset)).astype(np.float64).reshape(n4, 2, 2)     # [counter, pair, (radius, angle)]
    rad = np.sqrt(-2.0 * np.log(u[:, :, 0]))
    ang = 2.0 * np.pi * u[:, :, 1]
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=2).reshape(-1)[:n]
    radius = np.repeat(rad, 2, axis=1).reshape(-1)[:n]
    return z, radius


def counters_of(numel):
    """Counters one draw of ``numel`` elements occupies."""
    return (numel + 3) // 4


# The NoiseSource script shared by the CPU accounting test and the device test: (method, args) in call order,
# with element counts that are no multiple of 4.  "commit" moves the host offset into the device counter.
NOISE_SCRIPT_SEED = 11
NOISE_SCRIPT = [
    ("eps", ((3, 5, 7),)),
    ("keep_mask", ((2, 5, 9),)),
    ("eps_block", (2, 5, 6)),
    ("commit", ()),
    ("eps", ((5,),)),
]


def noise_script_plan(script=NOISE_SCRIPT, seed=NOISE_SCRIPT_SEED):
    """What the accounting rules say each draw of ``script`` uses: a list of (kind, seed, position, numel) with
    position the absolute stream position base + offset.  Every draw starts where the previous one ended."""
    plan, pos = [], 0
    for name, args in script:
        if name == "commit":
            continue
        shape = args[0] if name in ("eps", "keep_mask") else args
        numel = int(np.prod(shape))
        is_mask = name in ("keep_mask", "mask_block")
        plan.append(("mask" if is_mask else "normal", seed ^ MASK_SEED_XOR if is_mask else seed, pos, numel))
        pos += counters_of(numel)
    return plan
