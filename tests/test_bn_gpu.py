"""The fp32 BatchNorm + Swish kernels (csrc/bn.hip) and mmdyn_act_fwd / mmdyn_act_bwd on a real MI355X, held per element and per
channel by the runners of tests/bn_cases.py: the finalize kernels from synthetic partial tables against fp64 on the table, to fp32
rounding, in the two-launch and the ticket form and the two bit for bit (B); the tables of mmdyn_colstats and
mmdyn_bn_swish_bwd_reduce per (group, channel) against fp64 sums within the derived summation depth, then colstats -> bn_finalize
against fp64 statistics of the data (C); the element-wise outputs of mmdyn_bn_swish_fwd, mmdyn_bn_swish_bwd_apply,
mmdyn_bn_eval_stats + the three instances of mmdyn_bn_eval_swish_bwd, mmdyn_act_fwd and mmdyn_act_bwd by
store16_cases.check_rule with T = fp32, on inputs that reach |u| = 100 and rstd = 316 (D); the refusals (E).  The exact column sums
at every tile regime (A) are in tests/test_exact_gpu.py::test_pure_sums.  The constants, the preconditions and the teeth of the
checks are validated on the CPU by tests/test_bn_emu.py; every test prints its figures before it asserts."""
import pytest

import bn_cases as B
import test_kernels_gpu as K
from test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu


# ---- B: finalize from a given table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["well", "edge", "spread"])
@pytest.mark.parametrize("case", B.FINALIZE_CASES)
def test_finalize_from_a_table(case, kind):
    for repeat in (1, 2):
        for running in (True, False):
            B.run_finalize(K.HIP, DEV, case, kind, repeat, running)


@pytest.mark.parametrize("case", B.CRAFTED_CASES)
def test_finalize_forms_on_the_crafted_table(case):
    """T >= 640, a column whose fp32 result depends on how the fp64 tile sums are grouped: a launch with a ticket gives the bits of
    the two-launch form (it takes the two launches there; a four-slice single launch rounds this column to 1.0 instead of 1 + 2^-23)."""
    B.run_finalize(K.HIP, DEV, case, "crafted", 2, True)
    B.run_bwd_finalize(K.HIP, DEV, case, "crafted")


@pytest.mark.parametrize("case", B.FINALIZE_CASES)
def test_finalize_sums(case):
    B.run_finalize_sums(K.HIP, DEV, case, "well")
    B.run_finalize_sums(K.HIP, DEV, case, "spread")


@pytest.mark.parametrize("kind", ["well", "spread"])
@pytest.mark.parametrize("case", B.FINALIZE_CASES)
def test_bwd_finalize(case, kind):
    B.run_bwd_finalize(K.HIP, DEV, case, kind)


# ---- C: sums from data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", B.SUM_SHAPES)
def test_colstats_per_channel(shape):
    B.run_colstats(K.HIP, DEV, shape)


@pytest.mark.parametrize("shape", B.SUM_SHAPES)
def test_bwd_reduce_per_channel(shape):
    B.run_reduce(K.HIP, DEV, shape)


@pytest.mark.parametrize("shape", B.SUM_SHAPES)
def test_statistics_from_data(shape):
    B.run_statistics(K.HIP, DEV, shape)


# ---- D: element-wise outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pattern", B.d_cases())
def test_bn_swish_fwd(shape, pattern):
    B.run_fwd(K.HIP, DEV, shape, pattern)


@pytest.mark.parametrize("da_is_du", [False, True])
@pytest.mark.parametrize("shape,pattern", B.d_cases())
def test_bn_swish_bwd_apply(shape, pattern, da_is_du):
    B.run_apply(K.HIP, DEV, shape, da_is_du, pattern)


@pytest.mark.parametrize("variant", B.EVAL_VARIANTS)
@pytest.mark.parametrize("shape,pattern", [(s, i % 2) for i, s in enumerate(B.BN_SHAPES)] + [(B.BIG, 0)])
def test_bn_eval_swish_bwd(shape, pattern, variant):
    for dest in ("both",) if shape == B.BIG else ("dy", "planes", "both"):       # (the large shape is there for the tiling)
        B.run_eval(K.HIP, DEV, shape, variant, dest, pattern)


def test_bn_eval_stats():
    for G, C in ((1, 32), (3, 256), (4, 7)):
        B.run_eval_stats(K.HIP, DEV, G, C)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("n", B.ACT_N)
def test_act_fwd_and_bwd(n, act):
    B.run_act(K.HIP, DEV, n, act)


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("shape", B.BN_SHAPES)
def test_act_bwd_rows(shape, act):
    B.run_act_bwd(K.HIP, DEV, shape, act)


# ---- E: argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    B.run_argument_errors(K.HIP, DEV)
