"""The per-element rule of tests/store16_cases.py on a real MI355X: the 16-bit element-wise kernels (bn_swish_fwd_b16,
bn_swish_bwd_reduce_b16, bn_swish_bwd_apply_b16, act_bwd_b16) and the Swish / BatchNorm-backward epilogues of the GEMMs, in both
storage types and with fp32 outputs, against the documented formulas evaluated in fp64 on the widened inputs.  The constants of
the bound and the cap of rule 2 are validated on the CPU by tests/test_store16_emu.py; every test prints its figures (largest
|got - ref| / bound, share of the elements that differ from RNE(ref)) before it asserts.

The only pytest.skip is the one tests/test_kernels_gpu.py::test_igemm_all16_persistent already has (a forced persistent tile whose
width does not divide N: (TCONV_S2P1, 2, 5, 8, 128, 16, 64, 1, 0) under the forced 128 x 128 tile)."""
import pytest

import store16_cases as S
import test_kernels_gpu as K
from test_kernels_gpu import DEV, lab, wsp, store16                                                             # noqa: F401
from mmdyn_hip.ops import TCONV_S1P0

pytestmark = pytest.mark.gpu


# ---- element-wise kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.BN_SHAPES)
def test_bn_swish_fwd(shape, store16):
    S.run_fwd(K.HIP, DEV, shape, K.S16)


@pytest.mark.parametrize("shape", S.BN_SHAPES)
def test_bn_swish_fwd_half_subnormals_and_overflow(shape):
    """Inputs scaled so that part of the output is subnormal in half and part lies beyond 65504: RNE into subnormals and +-inf."""
    S.run_fwd(K.HIP, DEV, shape, S.F16, scaled=True)


@pytest.mark.parametrize("da_is_du", [False, True])
@pytest.mark.parametrize("shape", S.BN_SHAPES)
def test_bn_swish_bwd_apply(shape, da_is_du, store16):
    S.run_apply(K.HIP, DEV, shape, K.S16, da_is_du)


@pytest.mark.parametrize("shape", S.BN_SHAPES)
def test_bn_swish_bwd_reduce(shape, store16):
    S.run_reduce(K.HIP, DEV, shape, K.S16)


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("shape", S.BN_SHAPES)
def test_act_bwd(shape, act, store16):
    S.run_act_bwd(K.HIP, DEV, shape, K.S16, act)


# ---- GEMM epilogues --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", S.EPI_CASES)
def test_swish_output_16bit(case, mixed, store16):
    S.run_swish_out(K.HIP, DEV, case, K.S16, mixed=mixed)


@pytest.mark.parametrize("case", S.EPI_CASES[:3])
def test_dgrad_act_swish_16bit(case, store16):
    S.run_dgrad_act(K.HIP, DEV, case, K.S16)


@pytest.mark.parametrize("case", S.EPI_CASES)
def test_dgrad_bn_16bit(case, store16):
    S.run_dgrad_bn(K.HIP, DEV, case, K.S16)


@pytest.mark.parametrize("case", S.EPI_CASES)
def test_swish_output_fp32(case):
    S.run_swish_out(K.HIP, DEV, case, None)


@pytest.mark.parametrize("case", S.EPI_CASES[:3])
def test_dgrad_epilogues_fp32(case):
    S.run_dgrad_act(K.HIP, DEV, case, None)
    S.run_dgrad_bn(K.HIP, DEV, case, None)


@pytest.mark.parametrize("case", S.ALL16_CASES)
def test_epilogues_all16_persistent(case, wsp, store16, monkeypatch):
    """Both operands 16-bit in HBM on the persistent kernel (forced onto the small shapes), 16-bit outputs."""
    if case[6] % int(wsp.split(",")[1]):
        pytest.skip("N is not a multiple of the forced tile width")
    monkeypatch.setenv("MMDYN_WSP_MIN_UNITS", "0")
    monkeypatch.setenv("MMDYN_WSP_B16", "1")
    S.run_swish_out(K.HIP, DEV, case, K.S16, all16=True)
    if case[0] != TCONV_S1P0:
        S.run_dgrad_bn(K.HIP, DEV, case, K.S16, all16=True)
        S.run_dgrad_act(K.HIP, DEV, case, K.S16, all16=True)
