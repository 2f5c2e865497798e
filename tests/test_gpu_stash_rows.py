"""ncw_stash_from_rows / ncw_stash_to_rows (csrc/ncw_pack.hip) against the plain-torch statement of the stash layout
(tests/_stash_ref.py), bit for bit, in f32, bf16 and fp16.  Every module test feeds and reads its stashes through these two."""
import pytest
import torch

from tests._stash_ref import DTYPES, Carved, sync_or_stop, stash_decode, stash_encode

pytestmark = pytest.mark.gpu

NS = [1, 31, 32, 33, 130]
SHAPES = [(3, 1), (32, 1), (39, 2), (256, 8)]
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _prec(name):
    from neuralrecon_w_amd import lib as L

    return {"f32": L.PREC_F32, "bf16": L.PREC_BF16, "f16": L.PREC_F16}[name]


def _rows(n, F):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(7 * n + F))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("F,rb", SHAPES)
@pytest.mark.parametrize("prec_name", ["f32", "bf16", "f16"])
def test_from_rows_matches_the_torch_encoder(n, F, rb, prec_name):
    """From a NaN-filled stash: values rounded like torch's `.to(dtype)`, padded lanes and features written as zero, nothing
    written outside the ceil(n / 32) tiles."""
    from neuralrecon_w_amd import lib as L

    dtype = DTYPES[prec_name]
    rows = _rows(n, F)
    want = stash_encode(rows, rb, dtype)
    cv = Carved([torch.full_like(want, float("nan"))], "cuda")
    rows_d = rows.cuda()
    L.check(L.get_lib().ncw_stash_from_rows(_prec(prec_name), L.ptr(rows_d), n, F, rb, cv.ptr(0), L.stream_ptr()),
            "ncw_stash_from_rows")
    sync_or_stop()
    got = cv.view(0).cpu()
    assert torch.equal(got.view(BITS[dtype]), want.view(BITS[dtype]))
    assert cv.gaps_untouched()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("F,rb", SHAPES)
@pytest.mark.parametrize("prec_name", ["f32", "bf16", "f16"])
def test_to_rows_matches_the_torch_decoder(n, F, rb, prec_name):
    """The stash comes from the torch encoder, between NaN gaps; the rows buffer has a NaN guard behind it."""
    from neuralrecon_w_amd import lib as L

    dtype = DTYPES[prec_name]
    st = stash_encode(_rows(n, F), rb, dtype)
    cv = Carved([st], "cuda")
    out = torch.full((n * F + 64,), float("nan"), device="cuda")
    L.check(L.get_lib().ncw_stash_to_rows(_prec(prec_name), cv.ptr(0), n, F, rb, L.ptr(out), L.stream_ptr()),
            "ncw_stash_to_rows")
    sync_or_stop()
    want = stash_decode(st, n, F).float()
    assert torch.equal(out[:n * F].cpu().view(n, F).view(torch.int32), want.view(torch.int32))
    assert bool(torch.isnan(out[n * F:]).all())


@pytest.mark.parametrize("prec_name", ["f32", "bf16", "f16"])
def test_more_features_than_the_blocks_hold_is_refused(prec_name):
    from neuralrecon_w_amd import lib as L

    rows = torch.zeros(32, 33, device="cuda")
    st = torch.full((2 * 1024,), float("nan"), dtype=DTYPES[prec_name], device="cuda")
    lib = L.get_lib()
    assert lib.ncw_stash_from_rows(_prec(prec_name), L.ptr(rows), 32, 33, 1, L.ptr(st), L.stream_ptr()) == -1
    assert lib.ncw_stash_to_rows(_prec(prec_name), L.ptr(st), 32, 33, 1, L.ptr(rows), L.stream_ptr()) == -1
    sync_or_stop()
    assert bool(torch.isnan(st).all()) and not bool(rows.any())
