"""The per-element rule of tests/store16_cases.py on the CPU: (i) the plain torch-fp32 evaluation of every formula stays within a
quarter of the bound (the constants c are 4 x what it measures) and, rounded to the storage type, within the cap of rule 2 -- so
both are known to be reachable before anything runs on a GPU; (ii) the contract emulation passes every runner that
tests/test_store16_gpu.py holds the kernels to; (iii) the checks bite: a truncating 16-bit store and one element of the last
8-vector of the last row moved by two steps are reported."""
import re

import pytest
import torch

import store16_cases as S
from dirty import bits
from emu_backend import EmuBackend
from store16_cases import BF16, F16, F32, F64

EMU = EmuBackend()
DEV = "cpu"
MODES = {"bf16s": BF16, "fp16s": F16}


@pytest.fixture(params=list(MODES))
def storage(request):
    EMU.precision = request.param
    yield MODES[request.param]
    EMU.precision = "fp32"


# ---- (i) the fp32 twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [BF16, F16, None], ids=["bf16", "half", "fp32"])
def test_fp32_evaluation_is_within_a_quarter_of_the_bound_and_within_the_cap(T):
    rows = S.twin_figures(T)
    assert len(rows) >= 12
    for name, c, ratio, share in rows:
        print(f"{T} {name}: c = {c}, fp32 evaluation at {ratio:.2f} x 2^-24 M, {share:.2e} of the rounded elements differ from RNE")
        assert ratio <= c / 4, f"{name} ({T}): the fp32 evaluation reaches {ratio:.2f} x 2^-24 M, more than a quarter of c = {c}"
        if T is not None:      # (measured: at most 9.7e-4, half, apply pass on 2 x 129 x 32)
            assert share <= S.CAP, f"{name} ({T}): {share:.2e} of the rounded fp32 evaluation differ from RNE(ref): rule 2 is out of reach"


def test_every_constant_is_four_times_its_measured_maximum():
    """... over all shapes and types, rounded up to the next integer: none is slack, none is guessed."""
    worst = {}
    for T in (BF16, F16, None):
        for name, c, ratio, _ in S.twin_figures(T):
            worst[c] = max(worst.get(c, 0.0), ratio)
    assert sorted(worst) == sorted([S.C_FWD, S.C_APPLY, S.C_APPLY_DU, S.C_ACT_BWD, S.C_SWISH_OUT, S.C_DGRAD_ACT, S.C_DGRAD_BN])
    for c, ratio in worst.items():
        assert 4 * ratio <= c < 4 * ratio + 1, (c, ratio)


def test_rne_and_ulp_helpers_agree_with_torch():
    g = torch.Generator().manual_seed(7)
    x = torch.cat([torch.randn(4096, generator=g, dtype=F64) * 10.0 ** torch.randint(-8, 6, (4096,), generator=g).double(),
                   torch.tensor([0.0, 65504.0, 65519.99, 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 1.0, 1.0 - 2.0 ** -12],
                                dtype=F64)])
    for T in (F16, F32):       # (torch converts fp64 -> half / fp32 in one rounding; fp64 -> bf16 goes through fp32)
        assert torch.equal(bits(S.rne(x, T).to(T)), bits(x.to(T))), T
    x32 = x.float().double()
    assert torch.equal(bits(S.rne(x32, BF16).to(BF16)), bits(x32.float().to(BF16)))
    assert float(S.ulp(torch.tensor([1.0], dtype=F64), F16)) == 2.0 ** -10 and float(S.ulp(torch.tensor([1e-7], dtype=F64), F16)) == 2.0 ** -24
    assert float(S.ulp(torch.tensor([1.0], dtype=F64), BF16)) == 2.0 ** -7 and S.inf_threshold(F16) == 65520.0


# ---- (ii) the emulation passes every runner --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.BN_SHAPES)
def test_elementwise(shape, storage):
    S.run_fwd(EMU, DEV, shape, storage)
    if storage == F16:
        S.run_fwd(EMU, DEV, shape, storage, scaled=True)
    S.run_reduce(EMU, DEV, shape, storage)
    S.run_apply(EMU, DEV, shape, storage, False)
    S.run_apply(EMU, DEV, shape, storage, True)
    S.run_act_bwd(EMU, DEV, shape, storage, 1)
    S.run_act_bwd(EMU, DEV, shape, storage, 2)


@pytest.mark.parametrize("case", S.EPI_CASES[:3])
def test_epilogues_16bit(case, storage):
    S.run_swish_out(EMU, DEV, case, storage)
    S.run_swish_out(EMU, DEV, case, storage, mixed=True)
    S.run_dgrad_act(EMU, DEV, case, storage)
    S.run_dgrad_bn(EMU, DEV, case, storage)


@pytest.mark.parametrize("case", S.EPI_CASES[:3])
def test_epilogues_fp32(case):
    S.run_swish_out(EMU, DEV, case, None)
    S.run_dgrad_act(EMU, DEV, case, None)
    S.run_dgrad_bn(EMU, DEV, case, None)


def test_epilogues_all16(storage):
    case = S.ALL16_CASES[0]
    S.run_swish_out(EMU, DEV, case, storage, all16=True)
    S.run_dgrad_act(EMU, DEV, case, storage, all16=True)
    S.run_dgrad_bn(EMU, DEV, case, storage, all16=True)


# ---- (iii) the checks bite -------------------------------------------------------------------------------------------------------
def _truncate(x, dtype):
    """x -> dtype by dropping the low bits (round towards zero) instead of RNE."""
    r = x.to(dtype)
    over = r.float().abs() > x.abs()
    return torch.where(over, (r.view(torch.int16) - 1).view(dtype), r)


class TruncatingStore(EmuBackend):
    """Rounds what it stores into 16-bit tensors towards zero."""

    @staticmethod
    def _with_bf16(fn):
        def wrapped(*args):
            h16 = (BF16, F16)
            conv = [a.float() if torch.is_tensor(a) and a.dtype in h16 else a for a in args]
            r = fn(*conv)
            for o, c in zip(args, conv):
                if torch.is_tensor(o) and o.dtype in h16:
                    o.copy_(_truncate(c, o.dtype))
            return r
        return wrapped


class LastVectorOff(EmuBackend):
    """Moves element `lane` of the last 8-wide vector of the last row of every 16-bit output by two steps of the type."""
    lane = 5

    @staticmethod
    def _with_bf16(fn):
        inner = EmuBackend._with_bf16(fn)

        def wrapped(*args):
            before = [a.clone() if torch.is_tensor(a) and a.dtype in (BF16, F16) else None for a in args]
            r = inner(*args)
            for o, b in zip(args, before):
                if b is not None and not torch.equal(bits(o), bits(b)):          # an output
                    flat = o.view(-1).view(torch.int16)
                    flat[flat.numel() - 8 + LastVectorOff.lane] += 2
            return r
        return wrapped


@pytest.mark.parametrize("mode", list(MODES))
def test_a_truncating_16bit_store_is_reported(mode):
    be, T = TruncatingStore(), MODES[mode]
    be.precision = mode
    # about half of the elements land one step below RNE(ref): rule 1 already refuses those more than 1/2 ulp away, rule 2 the share
    rule2 = r"elements break rule 1|elements differ in bits from the RNE-rounded reference \(rule 2"
    for shape in S.BN_SHAPES:
        with pytest.raises(AssertionError, match=rule2):
            S.run_fwd(be, DEV, shape, T)
        for is_du in (False, True):
            with pytest.raises(AssertionError, match=rule2):
                S.run_apply(be, DEV, shape, T, is_du)
        with pytest.raises(AssertionError, match=rule2):
            S.run_act_bwd(be, DEV, shape, T, 1)
    case = S.EPI_CASES[0]
    # (acc + bias in 64ths: bf16 rounds it from |v| = 2 on and the plain C store is caught first, bit for bit)
    with pytest.raises(AssertionError, match=r"C: \d+ of \d+ elements differ" if T == BF16 else rule2):
        S.run_swish_out(be, DEV, case, T)
    with pytest.raises(AssertionError, match=rule2):
        S.run_swish_out(be, DEV, case, T, mixed=True)
    with pytest.raises(AssertionError, match=rule2):
        S.run_dgrad_act(be, DEV, case, T)
    with pytest.raises(AssertionError, match=rule2):
        S.run_dgrad_bn(be, DEV, case, T)


@pytest.mark.parametrize("mode", list(MODES))
def test_one_element_of_the_last_vector_two_steps_off_is_reported(mode):
    be, T = LastVectorOff(), MODES[mode]
    be.precision = mode
    for shape in S.BN_SHAPES:
        G, rpg, C = shape
        where = re.escape(f"1 of {G * rpg * C} elements break rule 1, the first at flat index {G * rpg * C - 8 + be.lane} "
                          f"(row {G * rpg - 1}, column {C - 8 + be.lane})")
        with pytest.raises(AssertionError, match=where):
            S.run_fwd(be, DEV, shape, T)
        for is_du in (False, True):
            with pytest.raises(AssertionError, match=where):
                S.run_apply(be, DEV, shape, T, is_du)
        with pytest.raises(AssertionError, match=where):
            S.run_act_bwd(be, DEV, shape, T, 1)
        with pytest.raises(AssertionError, match=re.escape(f"(row {G * rpg - 1}, column {C - 8 + be.lane})")):
            S.run_act_bwd(be, DEV, shape, T, 2)
    case = S.EPI_CASES[2]
    g = S.epi_inputs(case, T)["g"]
    where = re.escape(f"(row {g.rows - 1}, column {g.N - 8 + be.lane})")
    for run in (S.run_swish_out, S.run_dgrad_act, S.run_dgrad_bn):
        with pytest.raises(AssertionError, match=where):
            run(be, DEV, case, T)


def test_an_infinity_where_it_is_not_due_and_a_finite_value_where_it_is_are_reported():
    ref = torch.tensor([[70000.0, 60000.0, 65519.0, 1.0]], dtype=F64)
    M = ref.abs()
    ok = torch.tensor([[float("inf"), 60000.0, 65504.0, 1.0]], dtype=F16)
    S.check_rule(ok, ref, M, F16, 8.0, "as torch rounds")
    assert torch.equal(bits(ok), bits(ref.to(F16)))
    for col, value in ((0, 65504.0), (1, float("inf")), (2, float("inf")), (3, float("nan"))):
        bad = ok.clone()
        bad[0, col] = value
        with pytest.raises(AssertionError, match=re.escape(f"(row 0, column {col})")):
            S.check_rule(bad, ref, M, F16, 8.0, "edge")
