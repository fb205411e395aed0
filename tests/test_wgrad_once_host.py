"""mmdyn_wgrad_canon_served and the argument checks of mmdyn_wgrad_tn_canon: host arithmetic only, no GPU."""
import ctypes

from mmdyn_hip import _lib

ERR_SHAPE, ERR_NULL = -1, -2


def test_query_serves_the_two_fc_layers_of_the_bs256_step():
    lib = _lib.load()
    for flags in (0, 128):
        assert lib.mmdyn_wgrad_canon_served(256, 512, 6400, 1, flags) == 1        # encoder fc_net.0
        assert lib.mmdyn_wgrad_canon_served(1024, 6400, 256, 1, flags) == 1       # decoder upsample.0 (four groups' rows)
    # the chunk counts the once form keeps are the slab form's
    assert lib.mmdyn_wgrad_chunks_mx(0, 256, 512, 6400, 128) == 4
    assert lib.mmdyn_wgrad_chunks_mx(0, 1024, 6400, 256, 128) == 8


def test_query_declines_what_the_slab_path_sums_differently_or_stores_differently():
    lib = _lib.load()
    assert lib.mmdyn_wgrad_canon_served(256, 512, 6400, 1, 128 | 256) == 0        # plane operands
    assert lib.mmdyn_wgrad_canon_served(256, 512, 6400, 1, 128 | 512) == 0
    assert lib.mmdyn_wgrad_canon_served(256, 512, 6400, 1, 1 | 2) == 0            # 16-bit storage
    assert lib.mmdyn_wgrad_canon_served(256, 512, 6400, 1, 1 | 2 | 4) == 0
    assert lib.mmdyn_wgrad_canon_served(256, 512, 6400, 1, 1 | 4 | 32) == 0
    assert lib.mmdyn_wgrad_canon_served(256, 6400, 32, 1, 0) == 0                 # Cg = 32: two waves split the rows of a tile
    assert lib.mmdyn_wgrad_canon_served(256, 64, 512, 1, 0) == 0                  # 32768 elements: wgrad_reduce_kernel's order
    assert lib.mmdyn_wgrad_canon_served(257, 64, 512, 3, 0) == 1                  # ... three groups of them: the vec kernel's
    assert lib.mmdyn_wgrad_canon_served(128 * 68, 256, 256, 1, 0) == 0            # more than 64 chunks
    assert lib.mmdyn_wgrad_chunks_mx(0, 128 * 68, 256, 256, 0) == 68


def test_entry_point_reports_argument_errors_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)          # a valid host address: the checks return before anything is launched
    ok = dict(G=1, rows=256, Cd=512, Cg=6400, cgc=6400, perm=1)

    def call(D=p, Gt=p, canon=p, chunks=4, flags=128, **kw):
        a = dict(ok, **kw)
        return lib.mmdyn_wgrad_tn_canon(D, Gt, canon, a["G"], a["rows"], a["Cd"], a["Cg"], a["cgc"], a["perm"], 0.0, chunks, flags, None)

    assert call(D=None) == ERR_NULL and call(Gt=None) == ERR_NULL and call(canon=None) == ERR_NULL
    assert call(Cg=6144, cgc=6144) == ERR_SHAPE                 # perm 1 with Cg / 256 != 25
    assert call(perm=2) == ERR_SHAPE                            # perm 2 with Cd / 256 != 25
    assert call(cgc=6401) == ERR_SHAPE and call(cgc=0) == ERR_SHAPE
    assert call(chunks=2) == ERR_SHAPE and call(chunks=68) == ERR_SHAPE
    assert call(flags=128 | 256) == ERR_SHAPE and call(flags=1 | 2) == ERR_SHAPE
    assert call(G=2) == ERR_SHAPE                               # a permutation belongs to one group
    assert call(perm=0, Cd=64, Cg=512, cgc=512) == ERR_SHAPE    # not served: too few elements
