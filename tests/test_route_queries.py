"""Host queries of the GEMM dispatch (CPU only: the library loads and answers without a GPU).  Launcher and queries share one
route per launch (igemm_route / wgrad_route), so the answers for the different flag words of one shape must agree with each
other.  Shapes: every convolution-level and FC-level launch of the three image sizes' stacks, forward and input gradient, plus a
few shapes no specialised kernel serves."""
import itertools

import pytest

from mmdyn_hip import _lib
from mmdyn_hip.models import shapes as S

DENSE, CONV, TCONV_S2P1, TCONV_S1P0 = 0, 1, 2, 4


def stack_shapes(size):
    """(mode, Hi, Cin, Ho, N) of the GEMM launches of one image size: each layer forward and as its input gradient."""
    extra = S.extra_stages(size)
    out = []
    h = size // 2                                  # the 3-channel first layer has its own kernel
    enc = S.encoder_channels(extra)
    for j, (cin, cout) in enumerate(enc):
        if j + 1 < len(enc):                       # k4 s2 p1
            out += [(CONV, h, cin, h // 2, cout), (TCONV_S2P1, h // 2, cout, h, cin)]
            h //= 2
        else:                                      # k4 s1 p0: 8 -> 5
            out += [(CONV, h, cin, h - 3, cout), (TCONV_S1P0, h - 3, cout, h, cin)]
    assert h == 8
    h = S.FEAT_HW
    for j, (cin, cout) in enumerate(S.decoder_channels(extra)):
        if j == 0:                                 # k4 s1 p0: 5 -> 8
            out += [(TCONV_S1P0, h, cin, h + 3, cout), (CONV, h + 3, cout, h, cin)]
            h += 3
        else:
            out += [(TCONV_S2P1, h, cin, 2 * h, cout), (CONV, 2 * h, cout, h, cin)]
            h *= 2
    assert 2 * h == size
    for k, n in ((S.FEAT, S.HID), (S.HID, S.FEAT), (S.HID, 256), (256, S.HID), (256, S.FEAT), (S.FEAT, 256)):
        out.append((DENSE, 1, k, 1, n))
    return out


def all_shapes():
    seen = []
    layer = [s for size in S.IMG_SIZES for s in stack_shapes(size)]
    unserved = [(CONV, 16, 48, 8, 64), (TCONV_S2P1, 8, 48, 16, 128), (CONV, 16, 64, 8, 96), (TCONV_S2P1, 16, 128, 32, 96),
                (DENSE, 1, 48, 1, 96)]
    for (mode, Hi, Cin, Ho, N), Bg, G in itertools.product(layer + unserved, (2, 32, 130, 256, 1024), (1, 4)):
        if G * Bg * max(Hi, Ho) ** 2 * max(Cin, N) >= 2 ** 31:
            continue
        seen.append((mode, G, Bg, Hi, Hi, Cin, Ho, Ho, N))
    for (mode, Hi, Cin, Ho, N) in layer:             # one-sample batches
        seen.append((mode, 1, 1, Hi, Hi, Cin, Ho, Ho, N))
    return sorted(set(seen))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_stack_shapes_cover_the_three_sizes():
    assert [len(stack_shapes(s)) for s in S.IMG_SIZES] == [18, 22, 26]
    assert len(all_shapes()) >= 200                # (the three stacks share most layers)


def test_flag_words_of_one_shape_agree(lib):
    for a in all_shapes():
        assert lib.mmdyn_igemm_stat_tiles_mx(*a, 0) == lib.mmdyn_igemm_stat_tiles(*a), a
        assert lib.mmdyn_igemm_slab_floats_mx(*a, 0) == lib.mmdyn_igemm_slab_floats(*a), a
        assert lib.mmdyn_igemm_stat_tiles_mx(*a, 1) == lib.mmdyn_igemm_stat_tiles_bf16(*a), a
        assert lib.mmdyn_igemm_stat_tiles(*a) > 0 and lib.mmdyn_igemm_stat_tiles_bf16(*a) > 0, a


def test_planes_served_is_the_plane_launch_having_tiles(lib):
    served = 0
    for a in all_shapes():
        ps = lib.mmdyn_igemm_planes_served(*a)
        assert ps in (0, 1), a
        assert (ps == 1) == (lib.mmdyn_igemm_stat_tiles_mx(*a, 384) > 0), a
        if not ps:
            assert lib.mmdyn_igemm_slab_floats_mx(*a, 384) == 0, a
        served += ps
    assert 0 < served < len(all_shapes())          # both answers occur on this grid


def test_unserved_channel_counts_are_not_plane_launches(lib):
    for a in all_shapes():
        if a[5] == 48 or a[8] == 96:
            assert lib.mmdyn_igemm_planes_served(*a) == 0, a


def test_wgrad_chunks_one_operand_split_is_the_unsplit_count(lib):
    rows = (128, 1000, 4096, 25600, 65536, 262144)
    for mode, r, (cd, cg) in itertools.product((DENSE, CONV), rows, itertools.product((32, 64, 96, 128, 256, 512), repeat=2)):
        x3 = lib.mmdyn_wgrad_chunks_mx(mode, r, cd, cg, 128)
        assert x3 >= 4 and x3 % 4 == 0, (mode, r, cd, cg)
        assert lib.mmdyn_wgrad_chunks_mx(mode, r, cd, cg, 128 | 256) == x3, (mode, r, cd, cg)
        assert lib.mmdyn_wgrad_chunks_mx(mode, r, cd, cg, 128 | 512) == x3, (mode, r, cd, cg)
        assert lib.mmdyn_wgrad_chunks_mx(mode, r, cd, cg, 0) == lib.mmdyn_wgrad_chunks(mode, r, cd, cg), (mode, r, cd, cg)
