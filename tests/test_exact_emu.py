"""The exact-answer cases of tests/exact_cases.py on the CPU contract emulation: the builders, layouts, row orders and references
that tests/test_exact_gpu.py holds the kernels to are validated here, on a machine without a GPU, against an implementation that
shares no code with them (EmuBackend gathers with torch indexing; the family A reference is fp64 ATen convolution, the family B
reference index arithmetic).  Every comparison is `==` on values (family A) or on bits (family B); the guard rows around every
output must keep their sentinel.  The last tests show the checks bite: a reference off by 1 (family A) or by one ulp (family B) in a
single element, and a single overwritten guard element, are reported with their index; on the 16-bit stored paths, emulations
that truncate their 16-bit stores, drop the last row of a ragged weight-gradient chunk or multiply every group of a grouped GEMM
by the weights of group 0 are each reported."""
import re

import pytest
import torch

import exact_cases as X
from dirty import bits
from emu_backend import EmuBackend
from emu_backend_evalgrad import EmuBackendEvalGrad
from mmdyn_hip.ops import DENSE, CONV, TCONV_S2P1, IM2COL3, TCONV_S1P0
from test_kernels_gpu import IGEMM_CASES, WSP_CASES, WGRAD_CASES

EMU = EmuBackend()
DEV = "cpu"
FAMILIES = ["A", "B"]



def _cost(case):
    g = X.Geo(case)
    return g.rows * g.taps * g.Cin * g.N


# The emulation multiplies every tap as a dense fp32 matmul on the CPU: the cases above 2^31 multiply-adds (the same modes with more
# samples; the builders and references do not depend on the sample count) run on the GPU only, which keeps this file to seconds.
ALL_IGEMM = [c for c in list(dict.fromkeys(IGEMM_CASES + WSP_CASES)) + X.EDGE_CASES + X.NONSQUARE_CASES + X.IM2COL3_CASES
             if _cost(c) <= 1 << 31]
assert {c[0] for c in ALL_IGEMM} == {DENSE, CONV, TCONV_S2P1, IM2COL3, TCONV_S1P0}


@pytest.fixture(params=["fp32", "bf16", "fp16"])
def precision(request):
    EMU.precision = request.param
    yield request.param
    EMU.precision = "fp32"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", ALL_IGEMM)
def test_igemm(case, family):
    X.run_igemm(EMU, DEV, case, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [IGEMM_CASES[0], IGEMM_CASES[5], IGEMM_CASES[8], IGEMM_CASES[12]] + X.NONSQUARE_CASES[:4])
def test_igemm_wide_rows(case, family):
    """ldc = N + 32: the columns N..ldc of every row keep the sentinel."""
    X.run_igemm(EMU, DEV, case, family, ld_extra=32)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [IGEMM_CASES[3], IGEMM_CASES[5], IGEMM_CASES[8], IGEMM_CASES[12], X.NONSQUARE_CASES[0]])
def test_igemm_16bit_matrix_cores(case, family, precision):
    X.run_igemm(EMU, DEV, case, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [IGEMM_CASES[4], IGEMM_CASES[9], IGEMM_CASES[12]])
@pytest.mark.parametrize("mode", ["bf16s", "fp16s"])
def test_igemm_16bit_storage(case, family, mode):
    EMU.precision = mode
    try:
        X.run_igemm(EMU, DEV, case, family, store=torch.float16 if mode == "fp16s" else torch.bfloat16)
    finally:
        EMU.precision = "fp32"


@pytest.mark.parametrize("case", [IGEMM_CASES[2], IGEMM_CASES[5], IGEMM_CASES[8], IGEMM_CASES[12], X.NONSQUARE_CASES[3]])
def test_dgrad_relu(case):
    X.run_dgrad_relu(EMU, DEV, case)


# ---- 16-bit stored operands ("bf16s" / "fp16s"): the cases tests/test_exact_gpu.py runs, validated here --------------------------
@pytest.fixture(params=["bf16s", "fp16s"])
def storage(request):
    """The storage type of the mode; the emulation rounds its matrix-core operands to it for the duration."""
    EMU.precision = request.param
    yield torch.float16 if request.param == "fp16s" else torch.bfloat16
    EMU.precision = "fp32"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", X.IM2COL3_CASES)
def test_igemm_im2col3_16bit_output(case, family, storage):
    X.run_igemm(EMU, DEV, case, family, store=storage)


@pytest.mark.parametrize("case", X.MIXED_OUT_CASES)
def test_igemm_mixed_output(case, storage):
    X.run_igemm(EMU, DEV, case, "A", store=storage, mixed=True)


@pytest.mark.parametrize("case", [IGEMM_CASES[2], IGEMM_CASES[5], IGEMM_CASES[8]])
def test_dgrad_relu_16bit_storage(case, storage):
    X.run_dgrad_relu(EMU, DEV, case, store=storage)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("G,rows,K,N", X.GROUPED_16)
def test_grouped_16bit_storage(G, rows, K, N, family, storage):
    X.run_grouped(EMU, DEV, G, rows, K, N, family, store=storage)


@pytest.mark.parametrize("case,family,which", X.wgrad_store_triples(WGRAD_CASES[:7] + X.WGRAD_16))
def test_wgrad_16bit_storage(case, family, which, storage):
    X.run_wgrad(EMU, DEV, case, family, store=X.wgrad_store(which, storage))


@pytest.mark.parametrize("which", ["D", "Gt"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("G,rows,Cd,Cg", X.WGRAD_GROUPED_16)
def test_wgrad_grouped_16bit_storage(G, rows, Cd, Cg, family, which, storage):
    X.run_wgrad_grouped(EMU, DEV, G, rows, Cd, Cg, family, store=X.wgrad_store(which, storage))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Bt,Hi,Wi", X.TCONV_OUT3_16)
def test_tconv_out3_16bit_activation(Bt, Hi, Wi, family, storage):
    X.run_tconv_out3(EMU, DEV, Bt, Hi, Wi, family, store=storage)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows,K,N,splitk", [(64, 512, 256, 3), (5, 64, 32, 2), (129, 6400, 256, 25)])
def test_splitk(rows, K, N, splitk, family):
    X.run_splitk(EMU, DEV, rows, K, N, splitk, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("G,rows,K,N", [(3, 37, 64, 64), (4, 129, 512, 128), (2, 1, 32, 32)])
def test_grouped(G, rows, K, N, family):
    X.run_grouped(EMU, DEV, G, rows, K, N, family)


@pytest.mark.parametrize("case,family", X.wgrad_pairs(WGRAD_CASES[:7] + X.WGRAD_EXTRA))
def test_wgrad(case, family):
    X.run_wgrad(EMU, DEV, case, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("G,rows,Cd,Cg", [(3, 100, 64, 32), (2, 1, 32, 32), (4, 33, 32, 96)])
def test_wgrad_grouped(G, rows, Cd, Cg, family):
    X.run_wgrad_grouped(EMU, DEV, G, rows, Cd, Cg, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_direct_kernels(family):
    X.run_tconv_out3(EMU, DEV, 2, 16, 16, family)
    X.run_tconv_out3(EMU, DEV, 1, 16, 32, family)
    X.run_tconv_out3(EMU, DEV, 1, 32, 16, family)
    X.run_col2im(EMU, DEV, 3, 5, 5, 128, 1, 0, 1, 0, family)
    X.run_col2im(EMU, DEV, 2, 5, 7, 8, 1, 0, 1, 32, family)
    X.run_col2im(EMU, DEV, 2, 8, 12, 3, 2, 1, 0, 16, family)
    X.run_col2im(EMU, DEV, 1, 12, 8, 3, 2, 1, 0, 0, family)


def test_pure_sums():
    X.run_sums(EmuBackendEvalGrad(), DEV)      # (the emulation that restates mmdyn_bn_eval_swish_bwd as well)


def test_s1p0_rows_follow_the_output_pixels():
    """TCONV_S1P0 writes C as NHWC rows (sample, y, x) whatever order its tiles walk the (output pixel, sample) pairs in."""
    g = X.Geo((TCONV_S1P0, 1, 2, 5, 256, 8, 128, 1, 0))
    A = torch.zeros(g.a_shape)
    A[1 * 25 + 2 * 5 + 3, 7] = 1.0                        # sample 1, input pixel (2, 3), channel 7
    Bp = torch.zeros(16, 128, 256)
    Bp[1 * 4 + 2, 9, 7] = 1.0                             # tap (kh, kw) = (1, 2), column 9
    want = torch.zeros(g.rows, 128, dtype=torch.float64)
    want[1 * 64 + (2 + 1) * 8 + (3 + 2), 9] = 1.0         # output pixel (iy + kh, ix + kw)
    assert torch.equal(X.igemm_ref(g, A, Bp), want)
    assert torch.equal(X.select_ref(g, A, torch.full((128,), 6), torch.full((128,), 7), (torch.arange(128) == 9).float()).double(), want)


# ---- the checks bite -------------------------------------------------------------------------------------------------------------
def _launch(g, A, Bp):
    C = X.Guarded(g.rows, g.N, torch.float32, DEV, g.N + 32)
    EMU.igemm_nt(A, Bp, None, C.t, None, None, None, *g.dims, g.N + 32, g.stride, g.offset, 0, 1)
    return C


def test_a_reference_off_by_one_in_one_element_is_reported():
    g = X.Geo(X.NONSQUARE_CASES[0])
    A, Bp = X.int_operands(g, 11, sparse=False)
    ref = X.assert_int_exact(g, A, Bp)
    C = _launch(g, A, Bp)
    X.check_exact(C.values(), ref, "untouched")
    row, col = g.rows - 3, 77
    ref[row, col] += 1
    with pytest.raises(AssertionError, match=re.escape(f"1 of {ref.numel()} elements differ, the first at flat index "
                                                       f"{row * g.N + col} (row {row}, column {col})")):
        X.check_exact(C.values(), ref, "family A")


def test_a_reference_off_by_one_ulp_in_one_element_is_reported():
    g = X.Geo(X.NONSQUARE_CASES[3])
    Bp, tap, ci, scale = X.onehot_weights(g, 0)
    A = X.arbitrary(g.a_shape, 17)
    want = X.select_ref(g, A, tap, ci, scale)
    C = _launch(g, A, Bp)
    X.check_exact(C.values(), want, "untouched", bitwise=True)
    row = int((want[:, 5] != 0).nonzero()[-1])
    ulp = want.clone()
    ulp.view(torch.int32)[row, 5] += 1
    assert float((ulp[row, 5] - want[row, 5]).abs()) <= abs(float(want[row, 5])) * 2.0 ** -22
    with pytest.raises(AssertionError, match=re.escape(f"the first at flat index {row * g.N + 5} (row {row}, column 5)")):
        X.check_exact(C.values(), ulp, "family B", bitwise=True)
    # +0 against -0 is a difference too
    zero = (want == 0).nonzero()[0]
    neg = want.clone()
    neg[zero[0], zero[1]] = -0.0
    with pytest.raises(AssertionError, match=re.escape(f"(row {int(zero[0])}, column {int(zero[1])})")):
        X.check_exact(C.values(), neg, "family B", bitwise=True)


@pytest.mark.parametrize("where", ["front", "behind", "pad column"])
def test_one_overwritten_guard_element_is_reported(where):
    g = X.Geo(X.NONSQUARE_CASES[0])
    A, Bp = X.int_operands(g, 11, sparse=False)
    C = _launch(g, A, Bp)
    C.check("untouched")
    assert C.front >= X.GUARD_ROWS * C.ld and C.buf.numel() - C.front - C.n >= X.GUARD_ROWS * C.ld
    i = {"front": -1, "behind": C.n + 5, "pad column": 4 * C.ld + g.N}[where]
    C.buf[C.front + i] = 0.0
    msg = {"front": "1 elements in front of the slice", "behind": "5 elements behind the slice",
           "pad column": f"row 4, column {g.N} of the slice"}[where]
    with pytest.raises(AssertionError, match=re.escape(f"at guard index {i} ({msg})")):
        C.check("guard")
    # ... also when the stray write stored the value the kernel would have computed next to it (any bit pattern but the sentinel's)
    assert int(bits(C.buf[C.front + i:C.front + i + 1])[0]) != int(bits(C.buf[:1])[0])


# ---- ... and on the 16-bit stored paths: deliberately wrong emulations are reported ----------------------------------------------
def _truncate(x, dtype):
    """x -> dtype by dropping the low bits (round towards zero) instead of RNE."""
    if dtype == torch.bfloat16:
        return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(dtype)
    r = x.to(dtype)
    over = r.float().abs() > x.abs()                       # RNE went away from zero: one step back
    return torch.where(over, (r.view(torch.int16) - 1).view(dtype), r)


class TruncatingStore(EmuBackend):
    """Rounds what it stores into 16-bit tensors towards zero."""

    @staticmethod
    def _with_bf16(fn):
        def wrapped(*args):
            h16 = (torch.bfloat16, torch.float16)
            conv = [a.float() if torch.is_tensor(a) and a.dtype in h16 else a for a in args]
            r = fn(*conv)
            for o, c in zip(args, conv):
                if torch.is_tensor(o) and o.dtype in h16:
                    o.copy_(_truncate(c, o.dtype))
            return r
        return wrapped


class DropsLastRow(EmuBackend):
    """A weight gradient that leaves out the last row of a chunk that does not fill its 32-row K-step."""

    def __init__(self):
        super().__init__()
        inner = self.wgrad_tn

        def wgrad_tn(D, Gt, partial, mode, Bt, Hr, Wr, Cd, *rest):
            D = D.clone()
            if (Bt * Hr * Wr) % 32:
                D.reshape(Bt * Hr * Wr, Cd)[-1] = 0
            return inner(D, Gt, partial, mode, Bt, Hr, Wr, Cd, *rest)
        self.wgrad_tn = wgrad_tn


class SharesGroupZeroWeights(EmuBackend):
    """A grouped GEMM with b_group_stride = 0: every group multiplies the weights of group 0."""

    def __init__(self):
        super().__init__()
        inner = self.igemm_nt_grouped

        def igemm_nt_grouped(A, Bp, bias, C, C_act, u, G, rows, K, N, act):
            return inner(A, Bp.reshape(G, N, K)[:1].expand(G, N, K).contiguous(), bias, C, C_act, u, G, rows, K, N, act)
        self.igemm_nt_grouped = igemm_nt_grouped


@pytest.mark.parametrize("mode", ["bf16s", "fp16s"])
def test_a_truncating_16bit_store_is_reported(mode):
    be, t = TruncatingStore(), torch.float16 if mode == "fp16s" else torch.bfloat16
    be.precision = mode
    X.run_igemm(be, DEV, X.IM2COL3_CASES[0], "A", store=t)                 # (integers are stored exactly either way)
    with pytest.raises(AssertionError, match=r"C \(weight set 0\): \d+ of \d+ elements differ"):
        X.run_igemm(be, DEV, X.IM2COL3_CASES[0], "B", store=t)
    # (with a 16-bit A the selected element is a value of the type already and the store rounds nothing: the rounding mode of
    #  those stores is pinned by rule 2 of tests/store16_cases.py)
    X.run_igemm(be, DEV, IGEMM_CASES[9], "B", store=t)


@pytest.mark.parametrize("which", ["both", "D", "Gt"])
@pytest.mark.parametrize("mode", ["bf16s", "fp16s"])
def test_a_weight_gradient_that_drops_the_last_row_of_a_ragged_chunk_is_reported(mode, which):
    be, t = DropsLastRow(), torch.float16 if mode == "fp16s" else torch.bfloat16
    be.precision = mode
    X.run_wgrad(be, DEV, WGRAD_CASES[4], "A", store=X.wgrad_store(which, t))            # 768 rows: whole K-steps, nothing dropped
    for case in (X.WGRAD_EXTRA[7], X.WGRAD_EXTRA[8], X.WGRAD_EXTRA[2]):                 # 31, 33 and 120 rows
        with pytest.raises(AssertionError, match="partial summed over"):
            X.run_wgrad(be, DEV, case, "A", store=X.wgrad_store(which, t))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode", ["bf16s", "fp16s"])
def test_a_grouped_gemm_on_the_weights_of_group_zero_is_reported(mode, family):
    be, t = SharesGroupZeroWeights(), torch.float16 if mode == "fp16s" else torch.bfloat16
    be.precision = mode
    for shape in X.GROUPED_16:
        with pytest.raises(AssertionError, match=r"C: \d+ of \d+ elements differ"):
            X.run_grouped(be, DEV, *shape, family, store=t)
