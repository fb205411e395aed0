"""The dirty-memory harness (tests/dirty.py) on the CPU contract emulation: it passes on EmuBackend for one entry point of each
family, and it catches -- naming the right tensor -- small wrapper backends that break EmuBackend in the ways the harness is for:
a partial tile never written, an empty chunk never written, a `beta == 0` path that multiplies its destination, a write into a
read-only input and a write into a region documented as left untouched."""
import pytest
import torch

import dirty
from dirty import FILLS, JUNK, NAN, ZERO, PoisonTorch, assert_same_bits, bits, fill_, run_dirty
from emu_backend import EmuBackend
from mmdyn_hip.ops import CONV, DENSE

EMU = EmuBackend()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def igemm_args():
    mode, G, Bg, Hi, Cin, Ho, N, stride, offset = CONV, 2, 3, 16, 64, 8, 128, 2, -1
    Bt, T = G * Bg, 3
    A, Bp = rnd(Bt * Hi * Hi, Cin, seed=1), rnd(16, N, Cin, seed=2, scale=0.2)
    C, stats = torch.zeros(Bt * Ho * Ho, N), torch.zeros(G, T, 2, N)
    return [A, Bp, None, C, None, stats, None, mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N, N, stride, offset, 0, 1], [3, 5]


def wgrad_args(chunks=8):
    Bt, Hr, Cd, Hi, Cg = 3, 8, 128, 16, 64
    D, Gt = rnd(Bt * Hr * Hr, Cd, seed=7), rnd(Bt * Hi * Hi, Cg, seed=8)
    return [D, Gt, torch.zeros(chunks, 16, Cd, Cg), CONV, Bt, Hr, Hr, Cd, Hi, Hi, Cg, 2, -1, chunks], [2]


def reduce_args(beta=0.0, cgc=48):
    chunks, taps, Cd, Cg = 4, 1, 32, 64
    return [rnd(chunks, taps, Cd, Cg, seed=9), torch.zeros(Cd * cgc * taps), chunks, taps, Cd, Cg, cgc, 0, beta], [1]


def colsum_args():
    return [rnd(300, 512, seed=24), torch.zeros(512), 300, 512, 0, 0.0], [1]


def bnfin_args():
    G, T, C = 2, 5, 64
    return [rnd(G, T, 2, C, seed=61), torch.zeros(G, 2, C), torch.zeros(C), torch.zeros(C),
            torch.zeros(32, G, 2, C, dtype=torch.float64), G, T, C, 0.0], [1, 2, 3]


def repack_ld_args():
    rows, cols, ld = 40, 500, 512
    mask = torch.zeros(rows, ld, dtype=torch.bool)
    mask[:, cols:] = True                                   # the pad columns of each row: left untouched
    return [rnd(rows, cols, seed=102), torch.zeros(rows * ld), rows, cols, rows, cols, ld, 0], [1], {1: mask.reshape(-1)}


# ---- the fills themselves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
def test_fills_are_what_they_say(dtype):
    t = torch.ones(7, dtype=dtype)
    assert torch.equal(fill_(t.clone(), ZERO), torch.zeros(7, dtype=dtype))
    nan = fill_(t.clone(), NAN)
    assert torch.isnan(nan).all()
    want = {torch.float32: 0x7FC00000, torch.float64: 0x7FF8000000000000, torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}[dtype]
    assert (bits(nan).to(torch.int64) & ((1 << (8 * t.element_size())) - 1) == want).all()
    junk = fill_(t.clone(), JUNK)
    assert torch.isfinite(junk).all() and (junk.float().abs() > 5e4).all()


def test_integer_outputs_get_a5_bytes_and_views_are_filled_in_place():
    for dtype in (torch.uint8, torch.int32, torch.int64):
        t = fill_(torch.zeros(5, dtype=dtype), JUNK)
        assert (t.view(torch.uint8) == 0xA5).all()
    buf = torch.ones(4, 8)
    fill_(buf[:, 2:5], NAN)
    assert torch.isnan(buf[:, 2:5]).all() and (buf[:, :2] == 1).all() and (buf[:, 5:] == 1).all()


def test_nan_equals_nan_only_when_the_bits_match():
    a = fill_(torch.zeros(4), NAN)
    b = a.clone()
    assert dirty.first_diff(a, b) is None
    b.view(torch.int32)[2] = 0x7FC00001                     # another NaN payload
    assert dirty.first_diff(a, b) == 2


def test_poison_torch_fills_empty_only():
    pt = PoisonTorch(JUNK)
    assert pt.float32 is torch.float32 and pt.zeros(3).sum() == 0 and pt.Tensor is torch.Tensor
    assert (pt.empty(3, 4) > 1e29).all() and (pt.empty_like(torch.zeros(2, dtype=torch.bfloat16)).float() > 1e29).all()
    assert torch.isnan(PoisonTorch(NAN).empty(5, dtype=torch.float16)).all()
    assert (PoisonTorch(ZERO).empty(5) == 0).all()
    assert pt.empty(4, dtype=torch.int32).dtype == torch.int32           # integer tensors are left as they come


# ---- the emulation passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make", [("igemm_nt", igemm_args), ("wgrad_tn", wgrad_args), ("wgrad_reduce", reduce_args),
                                       ("colsum", colsum_args), ("bn_bwd_finalize", bnfin_args)])
def test_emulation_is_clean(name, make):
    args, outs = make()
    scratch = [4] if name == "bn_bwd_finalize" else []
    runs = run_dirty(EMU, name, args, outs, scratch=scratch)
    assert set(runs) == set(FILLS) and all(len(r) == len(outs) for r in runs.values())
    assert_same_bits(runs)


def test_untouched_region_is_checked_and_left_out_of_the_comparison():
    args, outs, mask = repack_ld_args()
    runs = run_dirty(EMU, "repack2d_ld", args, outs, untouched=mask)
    assert_same_bits(runs)
    assert torch.equal(runs[NAN]["dst"].reshape(40, 512)[:, :500], args[0])


def test_state_keeps_its_value_and_is_returned():
    G, T, C, rpg = 2, 3, 32, 50
    args = [rnd(G, T, 2, C, seed=3).abs(), torch.zeros(G, C), torch.zeros(G, C), rnd(C, seed=4), rnd(C, seed=5).abs() + 0.5,
            torch.full((), 7, dtype=torch.long), torch.zeros(32, G, 2, C, dtype=torch.float64), G, T, C, rpg, 1e-5, 0.1, 2]
    runs = run_dirty(EMU, "bn_finalize", args, [1, 2], scratch=[6], state=[3, 4, 5])
    assert_same_bits(runs)
    assert int(runs[JUNK]["nbt"]) == 7 + 2 * G and not torch.equal(runs[JUNK]["rm"], args[3])


# ---- broken backends: each must be caught, with the tensor named ------------------------------------------------------------
class StatTileNotWritten(EmuBackend):
    """Puts one BatchNorm partial tile back to what the buffer held before the launch: a tile no block wrote."""

    def igemm_nt(self, A, Bp, bias, C, C_act, stats, *rest):
        keep = stats[1, -1].clone()
        EmuBackend.igemm_nt(self, A, Bp, bias, C, C_act, stats, *rest)
        stats[1, -1] = keep


class LastChunkNotWritten(EmuBackend):
    """An empty K-chunk of the weight gradient's partial slabs left as it was."""

    def wgrad_tn(self, D, Gt, partial, *rest):
        keep = partial[-1].clone()
        EmuBackend.wgrad_tn(self, D, Gt, partial, *rest)
        partial[-1] = keep


class BetaWithoutGuard(EmuBackend):
    """beta * out + s with beta == 0: a stale NaN in the destination survives (0 * NaN)."""

    def wgrad_reduce(self, partial, canon, chunks, taps, Cd, Cg, cg_canon, perm, beta):
        old = canon.clone()
        EmuBackend.wgrad_reduce(self, partial, canon, chunks, taps, Cd, Cg, cg_canon, perm, 0.0)
        canon.copy_(beta * old + canon)


class WritesItsInput(EmuBackend):
    def colsum(self, x, out, rows, C, perm, beta):
        EmuBackend.colsum(self, x, out, rows, C, perm, beta)
        x.reshape(-1)[1234] += 1.0


class WritesThePadColumns(EmuBackend):
    def repack2d_ld(self, src, dst, rows_in, cols_in, rows_out, cols_out, ld_out, mode):
        EmuBackend.repack2d_ld(self, src, dst, rows_in, cols_in, rows_out, cols_out, ld_out, mode)
        dst.reshape(rows_out, ld_out)[3, cols_out + 2] = 0.0


def test_a_stat_tile_that_is_not_written_is_caught():
    args, outs = igemm_args()
    with pytest.raises(AssertionError, match=r"`stats`.*flat index"):
        assert_same_bits(run_dirty(StatTileNotWritten(), "igemm_nt", args, outs))


def test_an_empty_chunk_that_is_not_written_is_caught():
    args, outs = wgrad_args()
    with pytest.raises(AssertionError, match=r"`partial`.*flat index"):
        assert_same_bits(run_dirty(LastChunkNotWritten(), "wgrad_tn", args, outs))


def test_the_hole_is_located():
    """The message carries the first differing flat index: the start of the tile that was left out."""
    args, outs = igemm_args()
    G, T, N = 2, 3, 128
    with pytest.raises(AssertionError) as e:
        assert_same_bits(run_dirty(StatTileNotWritten(), "igemm_nt", args, outs))
    assert f"flat index {(1 * T + (T - 1)) * 2 * N} " in str(e.value)


def test_beta_zero_that_multiplies_the_destination_is_caught():
    args, outs = reduce_args(beta=0.0)
    with pytest.raises(AssertionError, match=r"`canon` holds a NaN"):
        assert_same_bits(run_dirty(BetaWithoutGuard(), "wgrad_reduce", args, outs))
    assert_same_bits(run_dirty(EMU, "wgrad_reduce", args, outs))


def test_a_write_into_a_read_only_input_is_caught():
    args, outs = colsum_args()
    with pytest.raises(AssertionError, match=r"read-only input `x` was modified at flat index 1234"):
        run_dirty(WritesItsInput(), "colsum", args, outs)


def test_a_write_into_an_untouched_region_is_caught():
    args, outs, mask = repack_ld_args()
    with pytest.raises(AssertionError, match=r"`dst` was written at flat index %d, inside the region documented" % (3 * 512 + 502)):
        run_dirty(WritesThePadColumns(), "repack2d_ld", args, outs, untouched=mask)


def test_callable_launch_and_names():
    def launch(backend, x, s, out):
        backend.scale_dev(x, s, out)
    x, s = rnd(33, seed=1), torch.tensor([0.25])
    runs = run_dirty(EMU, launch, [x, s, torch.zeros(33)], [2])
    assert_same_bits(runs)
    assert list(runs[ZERO]) == ["out"] and torch.equal(runs[NAN]["out"], x * 0.25)
