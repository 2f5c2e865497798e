"""CPU checks of tests/_stash_ref.py, the plain-torch statement of the stash layout the GPU tests of the converters and of
the weight-gradient GEMMs are measured against."""
import pytest
import torch

from tests._stash_ref import Carved, stash_decode, stash_encode, stash_encode_loops


@pytest.mark.parametrize("n", [1, 31, 32, 33, 130])
@pytest.mark.parametrize("F,rb", [(3, 1), (32, 1), (39, 2), (256, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_encode_then_decode_is_the_identity(n, F, rb, dtype):
    g = torch.Generator().manual_seed(n * 1000 + F)
    rows = torch.randn(n, F, generator=g)
    st = stash_encode(rows, rb, dtype)
    assert st.shape == ((n + 31) // 32, rb, 4, 64, 4) and st.dtype == dtype
    assert torch.equal(stash_decode(st, n, F), rows.to(dtype))
    # the padding is zero: as many non-zeros as the rows hold
    assert int((st != 0).sum()) == int((rows.to(dtype) != 0).sum())
    full = stash_decode(st, 32 * st.shape[0], 32 * rb)
    assert not full[n:].any() and not full[:, F:].any()


def test_encoder_agrees_with_explicit_loops():
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(37, 39, generator=g)
    assert torch.equal(stash_encode(rows, 2), stash_encode_loops(rows, 2))
    assert torch.equal(stash_encode(rows, 2, torch.bfloat16), stash_encode_loops(rows, 2, torch.bfloat16))
    # one element by hand: point 33 = tile 1, p 1; feature 38 = block 1, g 0, h 1, c 2 -> lane 33
    assert stash_encode(rows, 2)[1, 1, 0, 33, 2] == rows[33, 38]


def test_carved_vectors_sit_between_nan_gaps():
    a, b = stash_encode(torch.ones(5, 3), 1, torch.float16), stash_encode(torch.ones(40, 33), 2, torch.float16)
    cv = Carved([a, b], "cpu")
    assert torch.equal(cv.view(0), a) and torch.equal(cv.view(1), b) and cv.gaps_untouched()
    assert cv.ptr(0) % 256 == cv.buf.data_ptr() % 256 and (cv.ptr(1) - cv.ptr(0)) == 2 * (a.numel() + 256)
    assert int(torch.isnan(cv.buf).sum()) == 3 * 256
    cv.buf[0] = 0.0
    assert not cv.gaps_untouched()
