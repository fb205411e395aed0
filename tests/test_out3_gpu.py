"""The per-element checks of tests/out3_cases.py on a real MI355X: mmdyn_tconv_out3_bn_fwd, _bn_bce, _bn_bce_rows, _bn_bce_rows_grad
and mmdyn_wgrad_out3_bn against the documented formulas in fp64 -- selection and dense weights, non-square and single-tile images,
every combination of mask, published group and gradient buffer, every output (the fp64 loss tables included) in a guarded buffer.
The constants of the bounds are validated on the CPU by tests/test_out3_emu.py, which also shows that each check reports the
mistake it is there for; every test prints its figures (largest |got - ref| / bound) before it asserts."""
import pytest

import out3_cases as O
import test_kernels_gpu as K
from test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(params=list(O.TYPES))
def T(request):
    """The storage type of y: fp32, bf16 ("bf16s") or IEEE half ("fp16s")."""
    K.HIP.precision = request.param
    yield O.TYPES[request.param]
    K.HIP.precision = "fp32"


@pytest.mark.parametrize("shape", O.FWD_SHAPES)
def test_forward_selection(shape, T):
    O.run_fwd_select(K.HIP, DEV, shape, T)


@pytest.mark.parametrize("shape", O.FWD_SHAPES)
def test_forward_and_published_logits_dense(shape, T):
    O.run_dense(K.HIP, DEV, shape, T)


@pytest.mark.parametrize("entry", O.ENTRIES)
@pytest.mark.parametrize("shape", O.LOSS_SHAPES)
def test_loss_epilogue(shape, entry, T):
    O.run_loss(K.HIP, DEV, shape, T, entry)


@pytest.mark.parametrize("shape", [O.FWD_SHAPES[1], O.FWD_SHAPES[2], O.SLOTS_SHAPE])
def test_identities_of_the_weighted_form(shape, T):
    O.run_identities(K.HIP, DEV, shape, T)


@pytest.mark.parametrize("shape", O.WGRAD_SHAPES)
def test_weight_gradient_one_hot(shape, T):
    for label in O.chunk_values(K.HIP, shape):
        O.run_wgrad_select(K.HIP, DEV, shape, T, label)


@pytest.mark.parametrize("shape", O.WGRAD_SHAPES)
def test_weight_gradient_dense(shape, T):
    for label in O.chunk_values(K.HIP, shape):
        O.run_wgrad_dense(K.HIP, DEV, shape, T, label)


def test_weight_gradient_refuses_other_sizes(T):
    O.run_wgrad_refused(K.HIP, DEV, T)
