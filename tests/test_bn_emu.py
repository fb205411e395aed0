"""The checks of tests/bn_cases.py on the CPU: (i) the constants of family D are four times what a plain torch-fp32 evaluation of the
formulas measures over the tests' own inputs, and that evaluation stays within a quarter of each bound; the inputs, the tables and
the summation depth meet the preconditions the module states; (ii) the contract emulation passes every runner that
tests/test_bn_gpu.py holds the kernels to; (iii) the checks bite: fourteen wrong variants of the emulation, each a small override,
are each reported by a runner that the honest version passes."""
import pytest
import torch

import bn_cases as B
import exact_cases as X
from emu_backend import _act_grad
from emu_backend_evalgrad import EmuBackendEvalGrad

EMU = EmuBackendEvalGrad()
DEV = "cpu"


# ---- (i) constants and preconditions ---------------------------------------------------------------------------------------------
def test_fp32_evaluation_is_within_a_quarter_of_each_bound():
    rows = B.twin_figures()
    assert len(rows) >= 60
    for name, key, ratio in rows:
        c = getattr(B, key)
        print(f"{name}: {key} = {c}, fp32 evaluation at {ratio:.2f} x 2^-24 M")
        assert ratio <= c / 4, f"{name}: the fp32 evaluation reaches {ratio:.2f} x 2^-24 M, more than a quarter of {key} = {c}"


def test_every_constant_is_four_times_its_measured_maximum():
    """... over all shapes and sign patterns, rounded up to the next integer: none is slack, none is guessed."""
    worst = B.worst_figures()
    assert sorted(worst) == sorted(k for k in vars(B) if k.startswith("C_"))
    for key, ratio in worst.items():
        assert 4 * ratio <= getattr(B, key) < 4 * ratio + 1, (key, ratio)


def test_inputs_reach_the_ranges_they_promise():
    for shape, p in B.d_cases():
        B.assert_hard_ranges(shape, p)
    for n in B.ACT_N:
        u, _ = B.act_inputs(n)
        assert float(u[0]) == 0.0 and (n < 3 or (float(u[n // 2]) == 0.0 and bool(torch.signbit(u[n // 2]))))
    u = B.act_inputs(513000)[0]
    assert float(u.max()) > 99 and float(u.min()) < -99 and int((u.abs() > 88.7).sum()) > 100 and int((u.abs() < 3).sum()) > 400000
    for case in B.FINALIZE_CASES:
        for kind in ("well", "edge", "spread"):
            B.assert_table(kind, B.table(kind, *case), B.rows_for(case[1]))
    # the underflow allowance is confined to the elements it is written for
    low = B.underflow(torch.tensor([-86.0, -87.5, -89.0, -100.0, 50.0]), torch.ones(5))[1]
    assert low.tolist() == [False, True, True, True, False]


def test_summation_depth_and_tiling():
    """D = ceil(tile_rows / RL) + RL + 1, at most 133 over the admitted C; the restated tile height agrees with the library's count."""
    worst = 0
    for C in (32, 64, 128, 256):
        for rpg in (1, 63, 1000, 8224, 16385, 16447, 24609, 131073, 10 ** 6):
            worst = max(worst, B.depth(EMU, rpg, C))
    assert worst == 133 and B.depth(EMU, 131073, 256) == 133 and B.depth(EMU, 131073, 32) == 512 // 32 + 32 + 1
    assert [B.tile_rows_for(r) for r in (4097, 16385, 24609, 131073, 8224)] == [32, 64, 96, 512, 32]
    assert EMU.colstats_tiles(16385) == 257 and EMU.colstats_tiles(8224) == 257 and 16447 % 64 == 63 and 131073 % 512 == 1


# ---- (ii) the emulation passes every runner ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", X.COLSTATS_SHAPES)
def test_column_sums_exact(shape):
    X.run_colstats(EMU, DEV, shape)


@pytest.mark.parametrize("shape", X.EVAL_TABLE_SHAPES)
def test_eval_table_exact(shape):
    X.run_eval_table(EMU, DEV, shape)


@pytest.mark.parametrize("kind", ["well", "edge", "spread"])
@pytest.mark.parametrize("case", B.FINALIZE_CASES)
def test_finalize_from_a_table(case, kind):
    for repeat in (1, 2):
        for running in (True, False):
            B.run_finalize(EMU, DEV, case, kind, repeat, running)


@pytest.mark.parametrize("case", B.CRAFTED_CASES)
def test_finalize_forms_on_the_crafted_table(case):
    """(On the CPU: the table does what it is built for -- asserted by assert_table on a simulation of the kernels' summation order --
    and the emulation is within the bound.)"""
    B.run_finalize(EMU, DEV, case, "crafted", 2, True)
    B.run_bwd_finalize(EMU, DEV, case, "crafted")
    assert B.bn_splits(639) == 4 and B.bn_splits(640) == 5 and B.bn_splits(case[1]) > 4


@pytest.mark.parametrize("case", B.FINALIZE_CASES)
def test_finalize_sums(case):
    B.run_finalize_sums(EMU, DEV, case, "well")
    B.run_finalize_sums(EMU, DEV, case, "spread")


@pytest.mark.parametrize("case", B.FINALIZE_CASES)
def test_bwd_finalize(case):
    B.run_bwd_finalize(EMU, DEV, case, "well")
    B.run_bwd_finalize(EMU, DEV, case, "spread")


@pytest.mark.parametrize("shape", B.SUM_SHAPES)
def test_sums_from_data(shape):
    B.run_colstats(EMU, DEV, shape)
    B.run_reduce(EMU, DEV, shape)
    B.run_statistics(EMU, DEV, shape)


@pytest.mark.parametrize("shape,pattern", B.d_cases())
def test_elementwise(shape, pattern):
    B.run_fwd(EMU, DEV, shape, pattern)
    B.run_apply(EMU, DEV, shape, False, pattern)
    B.run_apply(EMU, DEV, shape, True, pattern)


@pytest.mark.parametrize("variant", B.EVAL_VARIANTS)
@pytest.mark.parametrize("shape,pattern", [(s, i % 2) for i, s in enumerate(B.BN_SHAPES)] + [(B.BIG, 0)])
def test_eval_backward(shape, pattern, variant):
    for dest in ("both",) if shape == B.BIG else ("dy", "planes", "both"):       # (the large shape is there for the tiling)
        B.run_eval(EMU, DEV, shape, variant, dest, pattern)


@pytest.mark.parametrize("n", B.ACT_N)
def test_activations(n):
    for act in (0, 1, 2):
        B.run_act(EMU, DEV, n, act)


@pytest.mark.parametrize("shape", B.BN_SHAPES)
def test_act_bwd_rows(shape):
    B.run_act_bwd(EMU, DEV, shape, 1)
    B.run_act_bwd(EMU, DEV, shape, 2)


def test_eval_stats():
    for G, C in ((1, 32), (3, 256), (4, 7)):
        B.run_eval_stats(EMU, DEV, G, C)


# ---- (iii) the checks bite -------------------------------------------------------------------------------------------------------
class Tiled(EmuBackendEvalGrad):
    """The emulation with the tables filled tile by tile (the row ranges of csrc/bn.hip) and the tile sums added slice by slice."""

    def rows_of(self, t, tr, rpg):
        return list(range(t * tr, min(rpg, (t + 1) * tr)))

    def _fill(self, a, b, partial, G, rpg, C):
        tr = B.tile_rows_for(rpg)
        T = -(-rpg // tr)
        p = partial.reshape(G, T, 2, C)
        for t in range(T):
            idx = torch.tensor(self.rows_of(t, tr, rpg), dtype=torch.long)
            p[:, t, 0], p[:, t, 1] = a[:, idx].sum(1), b[:, idx].sum(1)

    def colstats(self, y, partial, G, rpg, C):
        v = y.reshape(G, rpg, C)
        self._fill(v, v * v, partial, G, rpg, C)

    def bn_swish_bwd_reduce(self, da, y, mean, rstd, gamma, beta, partial, G, rpg, C):
        xh = self._xhat(y, mean, rstd, G, rpg, C)
        du = da.reshape(G, rpg, C) * _act_grad(xh * gamma + beta, 1)
        self._fill(du, du * xh, partial, G, rpg, C)

    def bn_eval_swish_bwd(self, da, y, mean, rstd, gamma, beta, dy, partial, G, rpg, C, da_is_du=False, planes=None):
        super().bn_eval_swish_bwd(da, y, mean, rstd, gamma, beta, dy, partial, G, rpg, C, da_is_du, planes)
        if partial is not None:
            xh = self._xhat(y, mean, rstd, G, rpg, C)
            du = da.reshape(G, rpg, C) * (1 if da_is_du else _act_grad(xh * gamma + beta, 1))
            self._fill(du, du * xh, partial, G, rpg, C)

    def slices(self, T):
        S = min(max(T // 128, 1), 32)
        per = -(-T // S)
        return [(s * per, min(T, (s + 1) * per)) for s in range(S)]

    def bn_finalize(self, partial, mean, rstd, rm, rv, nbt, scratch, G, T, C, rpg, eps, momentum, repeat):
        p = partial.reshape(G, T, 2, C).double()
        s = sum(p[:, lo:hi].sum(1) for lo, hi in self.slices(T))
        super().bn_finalize(s.reshape(G, 1, 2, C), mean, rstd, rm, rv, nbt, scratch, G, 1, C, rpg, eps, momentum, repeat)


def reported(honest, wrong, run):
    """`run(backend)` passes on the honest emulation and raises an AssertionError on the wrong one."""
    run(honest)
    with pytest.raises(AssertionError) as e:
        run(wrong)
    print("reported:", str(e.value)[:300])


def test_last_row_of_a_ragged_tile_left_out_is_reported():
    class V(Tiled):
        def rows_of(self, t, tr, rpg):
            r = super().rows_of(t, tr, rpg)
            return r[:-1] if len(r) < tr else r
    for shape in ((1, 16385, 32), (2, 4097, 64)):
        reported(Tiled(), V(), lambda be: X.run_colstats(be, DEV, shape))
    reported(Tiled(), V(), lambda be: X.run_eval_table(be, DEV, (1, 131073, 32)))
    reported(Tiled(), V(), lambda be: B.run_colstats(be, DEV, (2, 129, 32)))


def test_a_clamped_row_counted_twice_is_reported():
    class V(Tiled):
        def rows_of(self, t, tr, rpg):
            r = super().rows_of(t, tr, rpg)
            return r + r[:1] if len(r) < tr else r           # (the load of a row past the tile's end is clamped to the thread's first row)
    reported(Tiled(), V(), lambda be: X.run_colstats(be, DEV, (1, 16385, 32)))
    reported(Tiled(), V(), lambda be: X.run_eval_table(be, DEV, (1, 131073, 32)))
    reported(Tiled(), V(), lambda be: B.run_reduce(be, DEV, (4, 63, 128)))


def test_statistics_of_group_0_for_every_group_is_reported():
    class V(Tiled):
        def bn_swish_fwd(self, y, mean, rstd, gamma, beta, a, G, rpg, C):
            super().bn_swish_fwd(y, mean[:1].expand(G, C), rstd[:1].expand(G, C), gamma, beta, a, G, rpg, C)

        def bn_swish_bwd_apply(self, da, y, mean, rstd, gamma, beta, sums, dy, G, rpg, C, da_is_du=False):
            super().bn_swish_bwd_apply(da, y, mean[:1].expand(G, C), rstd[:1].expand(G, C), gamma, beta, sums, dy, G, rpg, C, da_is_du)
    reported(Tiled(), V(), lambda be: B.run_fwd(be, DEV, (2, 129, 32)))
    reported(Tiled(), V(), lambda be: B.run_apply(be, DEV, (4, 63, 128), True))


def test_a_slice_boundary_off_by_one_tile_is_reported():
    class V(Tiled):
        def slices(self, T):
            s = super().slices(T)
            return s if len(s) < 2 else [(s[0][0], s[0][1] - 1)] + s[1:]
    for case in ((2, 257, 64), (1, 640, 32)):
        for kind in ("well", "spread"):
            reported(Tiled(), V(), lambda be: B.run_finalize(be, DEV, case, kind, 1, True))


def _finish(variant):
    """bn_finalize restated with one line changed."""
    class V(Tiled):
        def bn_finalize(self, partial, mean, rstd, rm, rv, nbt, scratch, G, T, C, rpg, eps, momentum, repeat):
            if variant == "no clamp":
                s = partial.reshape(G, T, 2, C).double().sum(1)
                m = s[:, 0] / rpg
                var = s[:, 1] / rpg - m * m
                mean.copy_(m.float())
                rstd.copy_((1 / torch.sqrt(var + B.EPS)).float())
                return
            before = None if rv is None else rv.clone()
            super().bn_finalize(partial, mean, rstd, rm, rv, nbt, scratch, G, T, C, rpg, eps, momentum, 1 if variant == "once" else repeat)
            if variant == "once" and nbt is not None:
                nbt += G * (repeat - 1)
            if variant == "nbt" and nbt is not None:
                nbt -= G * (repeat - 1)
            if variant == "biased" and rv is not None:
                rv.copy_(before)
                var = ((1 / rstd.double()) ** 2 - B.EPS).clamp_min(0)
                for g in range(G):
                    for _ in range(repeat):
                        rv.copy_((B.OMM * rv.double() + B.MOM * var[g].float().double()).float())
    return V()


def test_biased_variance_in_running_var_is_reported():
    reported(Tiled(), _finish("biased"), lambda be: B.run_finalize(be, DEV, (4, 5, 128), "well", 1, True))


def test_running_estimates_updated_once_for_repeat_2_is_reported():
    reported(Tiled(), _finish("once"), lambda be: B.run_finalize(be, DEV, (4, 5, 128), "well", 2, True))
    reported(Tiled(), _finish("once"), lambda be: B.run_finalize(be, DEV, (1, 1, 32), "edge", 2, True))


def test_num_batches_tracked_plus_G_is_reported():
    reported(Tiled(), _finish("nbt"), lambda be: B.run_finalize(be, DEV, (2, 257, 64), "well", 2, True))


def test_no_clamp_of_a_negative_variance_is_reported():
    with pytest.raises(AssertionError, match="rstd"):
        B.run_finalize(_finish("no clamp"), DEV, (4, 5, 128), "edge", 1, False)
    B.run_finalize(_finish("no clamp"), DEV, (4, 5, 128), "well", 1, False)      # (the clamp matters on the constant channels alone)


def test_apply_pass_with_the_tile_row_count_is_reported():
    class V(Tiled):
        def bn_swish_bwd_apply(self, da, y, mean, rstd, gamma, beta, sums, dy, G, rpg, C, da_is_du=False):
            super().bn_swish_bwd_apply(da, y, mean, rstd, gamma, beta, sums * (rpg / min(rpg, B.tile_rows_for(rpg))), dy, G, rpg, C, da_is_du)
    for is_du in (False, True):
        reported(Tiled(), V(), lambda be: B.run_apply(be, DEV, (3, 1000, 64), is_du))


def test_s0_and_s1_exchanged_is_reported():
    class V(Tiled):
        def bn_swish_bwd_apply(self, da, y, mean, rstd, gamma, beta, sums, dy, G, rpg, C, da_is_du=False):
            super().bn_swish_bwd_apply(da, y, mean, rstd, gamma, beta, sums.flip(1), dy, G, rpg, C, da_is_du)
    for is_du in (False, True):
        reported(Tiled(), V(), lambda be: B.run_apply(be, DEV, (2, 129, 32), is_du))


def test_dgamma_overwritten_with_beta_acc_1_is_reported():
    class V(Tiled):
        def bn_bwd_finalize(self, partial, sums, dgamma, dbeta, scratch, G, T, C, beta_acc):
            super().bn_bwd_finalize(partial, sums, dgamma, dbeta, scratch, G, T, C, 0.0)
    with pytest.raises(AssertionError, match="beta_acc=1.0.*dgamma"):
        B.run_bwd_finalize(V(), DEV, (4, 5, 128), "well")
    B.run_bwd_finalize(Tiled(), DEV, (4, 5, 128), "well")


def test_unwritten_tail_of_act_fwd_is_reported():
    class V(Tiled):
        def act_fwd(self, u, h, act):
            n4 = u.numel() // 4 * 4
            super().act_fwd(u.reshape(-1)[:n4], h.reshape(-1)[:n4], act)
    for n in (1, 3, 5, 1027):
        for act in (0, 1, 2):
            reported(Tiled(), V(), lambda be: B.run_act(be, DEV, n, act))
    B.run_act(V(), DEV, 4, 1)


def test_a_sigmoid_that_overflows_is_reported():
    def swish(v):
        e = torch.exp(v)
        return v * (e / (1 + e))                    # NaN from 88.7 on

    class V(Tiled):
        def bn_swish_fwd(self, y, mean, rstd, gamma, beta, a, G, rpg, C):
            a.reshape(-1).copy_(swish(self._xhat(y, mean, rstd, G, rpg, C) * gamma + beta).reshape(-1))

        def act_fwd(self, u, h, act):
            h.reshape(-1).copy_(swish(u.reshape(-1)) if act == 1 else u.reshape(-1))
    reported(Tiled(), V(), lambda be: B.run_fwd(be, DEV, (4, 63, 128)))
    reported(Tiled(), V(), lambda be: B.run_act(be, DEV, 1027, 1))


def test_planes_of_the_previous_row_are_reported():
    class V(Tiled):
        def bn_eval_swish_bwd(self, da, y, mean, rstd, gamma, beta, dy, partial, G, rpg, C, da_is_du=False, planes=None):
            super().bn_eval_swish_bwd(da, y, mean, rstd, gamma, beta, dy, partial, G, rpg, C, da_is_du, planes)
            if planes is not None:
                planes.t.copy_(planes.t.roll(1, 0))
    for dest in ("planes", "both"):
        for variant in ("da", "du"):
            reported(Tiled(), V(), lambda be: B.run_eval(be, DEV, (2, 129, 32), variant, dest))
