"""Exact answers on a real MI355X: the cases of tests/exact_cases.py (validated against the CPU emulation by
tests/test_exact_emu.py) on HipBackend, on the default route and on every forced route that serves the mode.  Family A: integer
operands, every partial sum an exact fp32 integer, compared with `==` against fp64 ATen; family B: one-hot +-2^k weights against
arbitrary fp32, every output element one input element, compared bit for bit against index arithmetic (the 16-bit matrix-core modes
against the RNE-rounded element).  There is no tolerance in this file.  Every output is a slice in the middle of a JUNK-filled
buffer (exact_cases.Guarded): 64 rows in front and behind, and the columns N..ldc of the rows inside, must keep the sentinel.

The only pytest.skip is the one tests/test_kernels_gpu.py already has: a forced persistent tile whose width does not divide N.
It hits the N = 64 cases under the forced 128 x 128 tile (they run under the forced 128 x 64 tile):
  test_igemm_nt_persistent (both families): (DENSE, 2, 50, 1, 32, 1, 64, 1, 0), (CONV, 1, 4, 32, 32, 16, 64, 2, -1),
      (CONV, 1, 3, 32, 32, 16, 64, 2, -1), (TCONV_S2P1, 1, 4, 8, 128, 16, 64, 1, 0), (TCONV_S2P1, 4, 33, 8, 128, 16, 64, 1, 0),
      (DENSE, 1, 1, 1, 64, 1, 64, 1, 0), (DENSE, 4, 33, 1, 96, 1, 64, 1, 0), (DENSE, 1, 65, 1, 64, 1, 64, 1, 0),
      (CONV, 1, 2, 16, 64, 8, 64, 2, -1),
      (TCONV_S2P1, 4, 1, 8, 128, 16, 64, 1, 0), and the non-square (CONV, 2, 2, 24, 16, 64, 12, 8, 64, 2, -1),
      (TCONV_S2P1, 1, 3, 8, 12, 128, 16, 24, 64, 1, 0), (TCONV_S2P1, 2, 2, 12, 8, 64, 24, 16, 64, 1, 0),
      (DENSE, 1, 2, 3, 5, 64, 3, 5, 64, 1, 0);
  test_igemm_nt_persistent_wide_rows (both families): (TCONV_S2P1, 1, 3, 8, 12, 128, 16, 24, 64, 1, 0);
  test_igemm_all16_persistent (both families, both storage types): (TCONV_S2P1, 2, 5, 8, 128, 16, 64, 1, 0);
  test_dgrad_relu_persistent: (DENSE, 2, 50, 1, 32, 1, 64, 1, 0), (TCONV_S2P1, 4, 33, 8, 128, 16, 64, 1, 0),
      (TCONV_S2P1, 1, 3, 8, 12, 128, 16, 24, 64, 1, 0).

16-bit stored operands ("bf16s" / "fp16s", the *_16bit_* tests below): integers up to 256 (bf16) / 2048 (half) and +-2^k are exact
in storage, so both families apply unchanged -- the weight gradient with both operands, D only or Gt only read as 16-bit values
(the six storage instances of wgrad_tn.hip, wgrad_b16_kernel / wgrad_b16_tn4_kernel, conv3.hip's weight-gradient instances with
a 16-bit D) on every channel tile, on 1 / 31 / 33 rows and on non-square extents; mmdyn_igemm_nt_grouped, mmdyn_wgrad_tn_grouped
(one 16-bit operand: both is MMDYN_ERR_SHAPE, asserted), mmdyn_igemm_nt_dgrad_act (ReLU) and mmdyn_tconv_out3_fwd_b16; the
MMDYN_IM2COL3 launch with a 16-bit C and the mixed-output form (fp32 C, 16-bit C_act) in every mode.

Not exact, because they multiply by a sigmoid: the Swish epilogues (act = MMDYN_ACT_SWISH second output, mmdyn_igemm_nt_dgrad_act
with Swish) and the BatchNorm-backward epilogue of mmdyn_igemm_nt_dgrad_bn.  They are held per element by
tests/test_store16_gpu.py (rule of tests/store16_cases.py: half an ulp of the output type plus a measured multiple of 2^-24 of the
largest intermediate, against the documented formula in fp64, on the integer operands of family A), with 16-bit and with fp32
outputs, next to the 16-bit element-wise kernels (bn_swish_fwd / _bwd_reduce / _bwd_apply, act_bwd).  The fused last
decoder layer -- mmdyn_tconv_out3_bn_fwd, mmdyn_wgrad_out3_bn and the loss kernels mmdyn_tconv_out3_bn_bce, _bce_rows,
_bce_rows_grad, which evaluate log / exp per element and add into fp64 atomics -- is held by the same rule, with the selection
weights of family B, in tests/test_out3_gpu.py (cases and references: tests/out3_cases.py).  The weight-gradient selection
family runs both ways round (one-hot D, one-hot Gt) for the DENSE and CONV gathers; for MMDYN_IM2COL3, whose gathered operand is
the NCHW image, with the one-hot D only.

What reading the routes' address arithmetic for Hi != Wi found (before anything was launched):
  - the register-staged (igemm_nt.hip), wave-specialised (igemm_ws.hip), persistent (igemm_wsp.hip) and direct-fragment
    (igemm_d16.hip) kernels, the weight-gradient kernels (wgrad_tn.hip, wgrad_p3.hip), mmdyn_col2im_k4 and mmdyn_tconv_out3_fwd
    index rows with Hi / Ho / Hr and columns with Wi / Wo / Wr consistently, bound every gather with both extents and compute
    output offsets from (Ho, Wo, ldc): non-square shapes stay in bounds, and the tests below hold them to exact results;
  - MMDYN_TCONV_S1P0 is refused unless Ho == Wo == 8 (so Hi == Wi == 5): MMDYN_ERR_SHAPE, asserted below; the header said only
    "Ho = Hi+3" and now states the refusal;
  - the patch-resident k4 s2 p1 kernel (tconv_patch.hip) and the 3-channel first / last-layer kernels (conv3.hip) decline
    Hi != Wi (return 1) and the launch falls back to the generic kernels: results exact through the fallback, asserted below.
No kernel defect was found by these inputs.  Writing the mixed-output cases found one in the dispatch: an MMDYN_IM2COL3 launch of
the mixed-output form without a bias was handed to the first-layer kernel of conv3.hip, which stores C and C_act in one type and
would have written fp32 elements into the 16-bit C_act buffer (twice its size); the entry point now keeps that form on the
generic kernels (test_igemm_mixed_output, with a bias and without).
"""
import pytest
import torch

import exact_cases as X
import test_kernels_gpu as K
from test_kernels_gpu import (IGEMM_CASES, WGRAD_CASES, WSP_CASES, D16_TILES, DEV,                              # noqa: F401
                              lab, regstage, mfma16, wsp, d16_tile, store16, bf16_mode)                         # noqa: F401
from test_kernels_aten_gpu import x3                                                                            # noqa: F401
from mmdyn_hip import ops
from mmdyn_hip._lib import MmdynError
from mmdyn_hip.ops import DENSE, CONV, TCONV_S2P1, IM2COL3, TCONV_S1P0

pytestmark = pytest.mark.gpu

FAMILIES = ["A", "B"]
ALL_IGEMM = list(dict.fromkeys(IGEMM_CASES + WSP_CASES)) + X.EDGE_CASES + X.NONSQUARE_CASES + X.IM2COL3_CASES
NOT_IM2COL3 = [c for c in X.NONSQUARE_CASES if c[0] != IM2COL3]
# one case per mode, ragged row counts and four groups included, + the non-square ones: the forced routes that repeat a (route, mode)
# pair of another test
PER_MODE = [IGEMM_CASES[2], IGEMM_CASES[3], IGEMM_CASES[5], IGEMM_CASES[6], IGEMM_CASES[9], IGEMM_CASES[11], IGEMM_CASES[13]]


def igemm(case, family, **kw):
    X.run_igemm(K.HIP, DEV, case, family, **kw)


# ---- mmdyn_igemm_nt, fp32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", ALL_IGEMM)
def test_igemm_nt(case, family):
    igemm(case, family)


WIDE = [IGEMM_CASES[0], IGEMM_CASES[5], IGEMM_CASES[8], IGEMM_CASES[12], IGEMM_CASES[13], X.IM2COL3_CASES[0]] + NOT_IM2COL3[:4]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", WIDE)
def test_igemm_nt_wide_rows(case, family):
    """ldc = N + 32: the columns N..ldc of every row keep the sentinel."""
    igemm(case, family, ld_extra=32)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", IGEMM_CASES + X.EDGE_CASES + NOT_IM2COL3)
def test_igemm_nt_regstage(case, family, regstage):
    igemm(case, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [IGEMM_CASES[5], IGEMM_CASES[8]] + NOT_IM2COL3[:4])
def test_igemm_nt_regstage_wide_rows(case, family, regstage):
    igemm(case, family, ld_extra=32)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", PER_MODE + X.EDGE_CASES[2:5] + NOT_IM2COL3)
def test_igemm_nt_mfma16(case, family, mfma16):
    igemm(case, family)


WSP_EXACT = WSP_CASES + [c for c in X.EDGE_CASES if c[0] != TCONV_S1P0 and c[6] % 64 == 0] + [c for c in NOT_IM2COL3 if c[8] % 64 == 0]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", WSP_EXACT)
def test_igemm_nt_persistent(case, family, wsp):
    """Every tile split between blocks (stream-K): the K-step where a tile is handed from one block to the next, slabs + fix-up."""
    if X.Geo(case).N % int(wsp.split(",")[1]):
        pytest.skip("N is not a multiple of the forced tile width")
    igemm(case, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [WSP_CASES[4], NOT_IM2COL3[0], NOT_IM2COL3[3]])
def test_igemm_nt_persistent_wide_rows(case, family, wsp):
    if X.Geo(case).N % int(wsp.split(",")[1]):
        pytest.skip("N is not a multiple of the forced tile width")
    igemm(case, family, ld_extra=32)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [(TCONV_S1P0, 4, 70, 5, 256, 8, 128, 1, 0), (TCONV_S1P0, 1, 5, 5, 256, 8, 128, 1, 0),
                                  (TCONV_S1P0, 1, 129, 5, 256, 8, 128, 1, 0)])
def test_s1p0_persistent(case, family, lab, monkeypatch):
    monkeypatch.setenv("MMDYN_WSP_MIN_UNITS", "0")
    igemm(case, family)


@pytest.mark.parametrize("d16_tile", D16_TILES, indirect=True)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", PER_MODE + NOT_IM2COL3[:5])
def test_igemm_d16(case, family, d16_tile):
    igemm(case, family)


# ---- fp32x3 (flags 128) and plane operands (flags 384) ---------------------------------------------------------------------------
# (the split serves launches of >= 512 tiles: the first two cases are the smallest such; the others take the native kernels under
#  the same flag)
X3_CASES = [(CONV, 4, 64, 16, 64, 8, 128, 2, -1), (TCONV_S2P1, 4, 33, 16, 64, 32, 64, 1, 0), (DENSE, 1, 6400, 1, 256, 1, 2048, 1, 0)] + \
    PER_MODE + NOT_IM2COL3[:4]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", X3_CASES)
def test_igemm_x3(case, family, x3):
    """Integers have mid = lo = 0; the selection family populates all three planes of the arbitrary operand: hi b + mid b + lo b
    is exact in any order, so the result is the fp32 element bit for bit."""
    X.run_igemm(ops.B, DEV, case, family)


def _planes(x):
    p = ops.Planes(x.shape[0], x.shape[1], x.device)
    ops.B.split_planes(x.contiguous(), p)
    return p


PLANE_CASES = [(CONV, 4, 75, 16, 64, 8, 128, 2, -1), (TCONV_S2P1, 2, 77, 8, 128, 16, 64, 1, 0), (TCONV_S1P0, 4, 70, 5, 256, 8, 128, 1, 0),
               # the patch-resident P3 up-sampling layers (csrc/tconv_patch.hip)
               (TCONV_S2P1, 2, 3, 32, 32, 64, 32, 1, 0), (TCONV_S2P1, 4, 6, 16, 64, 32, 32, 1, 0), (TCONV_S2P1, 1, 150, 32, 32, 64, 32, 1, 0)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", PLANE_CASES)
def test_igemm_planes(case, family, x3):
    g = X.Geo(case)
    assert ops.B.igemm_planes_served(*g.dims)
    X.run_igemm(ops.B, DEV, case, family, planes=True, prep=lambda a, b: (_planes(a), _planes(b.view(-1, g.Cin))))


# ---- 16-bit matrix cores and 16-bit storage --------------------------------------------------------------------------------------
B16_CASES = [IGEMM_CASES[1], IGEMM_CASES[3], IGEMM_CASES[5], IGEMM_CASES[6], IGEMM_CASES[9], IGEMM_CASES[13]] + NOT_IM2COL3[:4]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", B16_CASES)
def test_igemm_nt_bf16(case, family, bf16_mode):
    igemm(case, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", B16_CASES)
def test_igemm_nt_f16(case, family):
    K.HIP.precision = "fp16"
    try:
        igemm(case, family)
    finally:
        K.HIP.precision = "fp32"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [IGEMM_CASES[1], IGEMM_CASES[4], IGEMM_CASES[6], IGEMM_CASES[9], IGEMM_CASES[13], NOT_IM2COL3[0], NOT_IM2COL3[3]])
def test_igemm_16bit_storage(case, family, store16):
    igemm(case, family, store=K.S16)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [(CONV, 2, 3, 16, 64, 8, 128, 2, -1), (TCONV_S2P1, 2, 5, 8, 128, 16, 64, 1, 0), (TCONV_S1P0, 2, 70, 5, 256, 8, 128, 1, 0)])
def test_igemm_all16_persistent(case, family, wsp, store16, monkeypatch):
    """Both operands 16-bit in HBM on the persistent kernel (forced onto the small shapes), 16-bit outputs."""
    if X.Geo(case).N % int(wsp.split(",")[1]):
        pytest.skip("N is not a multiple of the forced tile width")
    monkeypatch.setenv("MMDYN_WSP_MIN_UNITS", "0")
    monkeypatch.setenv("MMDYN_WSP_B16", "1")
    igemm(case, family, store=K.S16, all16=True)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", X.IM2COL3_CASES)
def test_igemm_im2col3_16bit_output(case, family, store16):
    """The first layer of the storage modes: fp32 NCHW image, 16-bit C (conv3.hip and the generic route)."""
    igemm(case, family, store=K.S16)


@pytest.mark.parametrize("case", X.MIXED_OUT_CASES)
def test_igemm_mixed_output(case, store16):
    """fp32 C + 16-bit C_act (storage flag bit 6), ReLU, with a bias and without.  The 3-channel first-layer kernel stores both
    outputs in one type: the entry point keeps this form away from it (without a bias it used to be taken there)."""
    igemm(case, "A", store=K.S16, mixed=True)


# ---- epilogues, split-K, grouped -------------------------------------------------------------------------------------------------
DGRAD = [IGEMM_CASES[2], IGEMM_CASES[3], IGEMM_CASES[5], IGEMM_CASES[6], IGEMM_CASES[8], (TCONV_S2P1, 1, 3, 16, 64, 32, 32, 1, 0)] + NOT_IM2COL3[:4]


@pytest.mark.parametrize("case", DGRAD)
def test_dgrad_relu(case):
    X.run_dgrad_relu(K.HIP, DEV, case)


@pytest.mark.parametrize("case", DGRAD)
def test_dgrad_relu_regstage(case, regstage):
    X.run_dgrad_relu(K.HIP, DEV, case)


@pytest.mark.parametrize("case", [WSP_CASES[2], WSP_CASES[4], WSP_CASES[-1], WSP_CASES[-2], NOT_IM2COL3[0], NOT_IM2COL3[3]])
def test_dgrad_relu_persistent(case, wsp):
    if X.Geo(case).N % int(wsp.split(",")[1]):
        pytest.skip("N is not a multiple of the forced tile width")
    X.run_dgrad_relu(K.HIP, DEV, case)


@pytest.mark.parametrize("case", [DGRAD[0], DGRAD[2], DGRAD[4]])
def test_dgrad_relu_16bit_storage(case, store16):
    """A, u and C 16-bit in HBM, one case per mode."""
    X.run_dgrad_relu(K.HIP, DEV, case, store=K.S16)


SPLITK = [(256, 6400, 512, 25), (64, 512, 256, 3), (5, 64, 32, 2), (129, 6400, 256, 8)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows,K_,N,splitk", SPLITK)
def test_splitk(rows, K_, N, splitk, family):
    X.run_splitk(K.HIP, DEV, rows, K_, N, splitk, family)


@pytest.mark.parametrize("d16_tile", D16_TILES[:2], indirect=True)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows,K_,N,splitk", SPLITK[1:])
def test_splitk_d16(rows, K_, N, splitk, family, d16_tile):
    X.run_splitk(K.HIP, DEV, rows, K_, N, splitk, family)


GROUPED = [(3, 37, 64, 64), (4, 129, 512, 128), (2, 1, 32, 32), (3, 1024, 512, 512)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("G,rows,K_,N", GROUPED)
def test_grouped(G, rows, K_, N, family):
    X.run_grouped(K.HIP, DEV, G, rows, K_, N, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("G,rows,K_,N", GROUPED[:2])
def test_grouped_bf16(G, rows, K_, N, family, bf16_mode):
    X.run_grouped(K.HIP, DEV, G, rows, K_, N, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("G,rows,K_,N", X.GROUPED_16)
def test_grouped_16bit_storage(G, rows, K_, N, family, store16):
    X.run_grouped(K.HIP, DEV, G, rows, K_, N, family, store=K.S16)


# ---- weight gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,family", X.wgrad_pairs(WGRAD_CASES[:7] + X.WGRAD_EXTRA))
def test_wgrad(case, family):
    X.run_wgrad(K.HIP, DEV, case, family)


@pytest.mark.parametrize("case,family", X.wgrad_pairs([WGRAD_CASES[0], WGRAD_CASES[4], WGRAD_CASES[6]] + X.WGRAD_EXTRA[:3]))
def test_wgrad_bf16(case, family, bf16_mode):
    X.run_wgrad(K.HIP, DEV, case, family)


@pytest.mark.parametrize("case,family,which", X.wgrad_store_triples(WGRAD_CASES[:7] + X.WGRAD_16))
def test_wgrad_16bit_storage(case, family, which, store16):
    """Operands read as 16-bit values from HBM: both (wgrad_b16_kernel / wgrad_b16_tn4_kernel and their transposing LDS reads), D
    only or Gt only (the storage instances of wgrad_tn.hip), in both formats; MMDYN_IM2COL3 with a 16-bit D (conv3.hip's
    weight-gradient instances and, for Hi != Wi or other extents, the generic route)."""
    X.run_wgrad(K.HIP, DEV, case, family, store=X.wgrad_store(which, K.S16))


@pytest.mark.parametrize("which", ["D", "Gt"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("G,rows,Cd,Cg", X.WGRAD_GROUPED_16)
def test_wgrad_grouped_16bit_storage(G, rows, Cd, Cg, family, which, store16):
    X.run_wgrad_grouped(K.HIP, DEV, G, rows, Cd, Cg, family, store=X.wgrad_store(which, K.S16))


def test_wgrad_grouped_refuses_two_16bit_operands(store16):
    """The grouped launch runs the register-staged kernel only: both operands 16-bit is MMDYN_ERR_SHAPE, nothing is launched."""
    G, rows, Cd, Cg = X.WGRAD_GROUPED_16[0]
    chunks = K.HIP.wgrad_chunks(DENSE, rows, Cd, Cg)
    P = X.Guarded(chunks * G * Cd, Cg, torch.float32, DEV)
    D, Gt = torch.zeros(G * rows, Cd, dtype=K.S16, device=DEV), torch.zeros(G * rows, Cg, dtype=K.S16, device=DEV)
    with pytest.raises(MmdynError, match="MMDYN_ERR_SHAPE"):
        K.HIP.wgrad_tn_grouped(D, Gt, P.view(chunks, G, Cd, Cg), G, rows, Cd, Cg, chunks)
    torch.cuda.synchronize()
    assert torch.equal(P.buf.cpu(), X.Guarded(chunks * G * Cd, Cg).buf)


# mode, Bt, Hr, Wr, Cd, Hi, Wi, Cg, stride, offset: the tiles of test_weight_gradient_on_operands_that_arrive_split + a non-square one
SPLIT_WGRAD = [(CONV, 64, 5, 5, 256, 8, 8, 128, 1, 0, None, 0), (CONV, 64, 8, 8, 128, 16, 16, 64, 2, -1, None, 0),
               (CONV, 64, 8, 8, 64, 16, 16, 64, 2, -1, None, 0), (CONV, 64, 16, 16, 64, 32, 32, 32, 2, -1, None, 0),
               (CONV, 64, 16, 16, 32, 32, 32, 64, 2, -1, None, 0), (CONV, 48, 8, 12, 128, 16, 24, 64, 2, -1, None, 0)]


@pytest.mark.parametrize("planes", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("case,family", X.wgrad_pairs(SPLIT_WGRAD))
def test_wgrad_x3_and_planes(case, family, planes, x3):
    """The fp32x3 weight gradient with either operand (or both) arriving split: both split takes the plane-ring kernel where it
    serves the shape."""
    prep = lambda d, g: (_planes(d) if planes[0] else d, _planes(g) if planes[1] else g)
    X.run_wgrad(ops.B, DEV, case, family, prep=prep, planes=planes)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("G,rows,Cd,Cg", [(3, 100, 64, 32), (2, 1, 32, 32), (4, 33, 32, 96), (3, 1024, 512, 512)])
def test_wgrad_grouped(G, rows, Cd, Cg, family):
    X.run_wgrad_grouped(K.HIP, DEV, G, rows, Cd, Cg, family)


# ---- direct kernels and pure sums ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Bt,Hi,Wi", [(2, 16, 16), (1, 16, 32), (1, 32, 16), (3, 32, 32), (1, 48, 16)])
def test_tconv_out3_fwd(Bt, Hi, Wi, family):
    X.run_tconv_out3(K.HIP, DEV, Bt, Hi, Wi, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Bt,Hi,Wi", X.TCONV_OUT3_16)
def test_tconv_out3_fwd_16bit_activation(Bt, Hi, Wi, family, store16):
    """mmdyn_tconv_out3_fwd_b16: the activation 16-bit in HBM, fp32 weights and logits."""
    X.run_tconv_out3(K.HIP, DEV, Bt, Hi, Wi, family, store=K.S16)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Bt,Hi,Wi,C,stride,pad,tap_major,ld_extra", [(3, 5, 5, 128, 1, 0, 1, 0), (2, 5, 7, 8, 1, 0, 1, 32), (2, 7, 5, 6, 1, 0, 1, 0),
                                                                      (2, 32, 32, 3, 2, 1, 0, 16), (2, 8, 12, 3, 2, 1, 0, 16),
                                                                      (1, 12, 8, 3, 2, 1, 0, 0), (2, 8, 12, 4, 2, 1, 1, 0)])
def test_col2im_k4(Bt, Hi, Wi, C, stride, pad, tap_major, ld_extra, family):
    X.run_col2im(K.HIP, DEV, Bt, Hi, Wi, C, stride, pad, tap_major, ld_extra, family)


def test_pure_sums():
    X.run_sums(K.HIP, DEV)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hi,Wi", [(5, 6), (6, 5), (4, 5), (6, 6)])
def test_s1p0_refuses_everything_but_5x5_to_8x8(Hi, Wi):
    """MMDYN_TCONV_S1P0 walks the four-pixel quads of an 8 x 8 output: any other extent is MMDYN_ERR_SHAPE on the host, and nothing
    is launched (the output keeps the sentinel everywhere)."""
    g = X.Geo((TCONV_S1P0, 1, 2, Hi, Wi, 256, Hi + 3, Wi + 3, 128, 1, 0))
    A, Bp = X.int_operands(g, 11, sparse=False)
    C = X.Guarded(g.rows, g.N, torch.float32, DEV)
    with pytest.raises(MmdynError, match="MMDYN_ERR_SHAPE"):
        K.HIP.igemm_nt(A.to(DEV), Bp.to(DEV), None, C.t, None, None, None, *g.dims, g.N, 1, 0, 0, 1)
    torch.cuda.synchronize()
    assert torch.equal(C.buf.cpu(), X.Guarded(g.rows, g.N).buf)


def test_specialised_routes_decline_non_square_shapes():
    """Host queries: the patch-resident kernel and its plane form serve 16x16 / 32x32 inputs and decline 16x32; the launch of the
    declined shape (NONSQUARE_CASES, test_igemm_nt) is exact through the generic kernels."""
    lib = K.HIP.lib
    sq = lib.mmdyn_igemm_stat_tiles(TCONV_S2P1, 1, 2, 16, 16, 64, 32, 32, 32)
    assert sq == 2 * 1 and lib.mmdyn_igemm_stat_tiles(TCONV_S2P1, 1, 2, 16, 32, 64, 32, 64, 32) != 2 * 2
    assert lib.mmdyn_igemm_planes_served(TCONV_S2P1, 1, 2, 16, 16, 64, 32, 32, 32) == 1
    assert lib.mmdyn_igemm_planes_served(TCONV_S2P1, 1, 2, 16, 32, 64, 32, 64, 32) == 0
