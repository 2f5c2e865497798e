"""The weight-gradient GEMMs of csrc/ncw_wgrad.hip, called directly and checked EXACTLY.

Both operands hold small integers ({-2 .. 2}), so every product and every partial sum is an integer far below 2^24: fp32
represents them exactly in any summation order (the order of the f32 atomics included), and the integers survive the
conversion to bf16 / fp16 unchanged.  dense += X^T Y and dbias += column sums of X must therefore equal an int64 reference bit
for bit in all three precisions -- a dropped, duplicated or misplaced tile, block, K-slice or bias term cannot hide.

The operands are laid out by tests/_stash_ref.py (plain torch, not the library's converter) inside one NaN-filled buffer, so a
read outside a product's own vectors poisons the result; the workgroup prefix is computed here from the header's formulas (4 x 4,
4 x 8 and 8 x 8 blocks per workgroup), not taken from stash.WgradBatch.  One last case per entry point runs real-valued rows
and bounds the accumulation error by the textbook fp32 bound."""
import functools

import pytest
import torch

from tests._stash_ref import DTYPES, Carved, sync_or_stop, n_tiles, stash_decode, stash_encode

pytestmark = pytest.mark.gpu

NCW_E_BADARG = -1
# (entry point, precision): every pair that exists
PAIRS = [("wgrad", "f32"), ("wgrad", "bf16"), ("wgrad", "f16"), ("ordered", "f32"), ("ordered", "bf16"), ("ordered", "f16"),
         ("tiled0", "bf16"), ("tiled1", "bf16"), ("tiled0", "f16"), ("tiled1", "f16")]
PAIR_IDS = ["%s-%s" % p for p in PAIRS]
# feature blocks (X, Y) per workgroup: include/neuconw_hip.h, ncw_wgrad / ncw_wgrad_tiled
WG_BLOCKS = {"wgrad": (4, 4), "ordered": (4, 4), "tiled0": (4, 8), "tiled1": (8, 8)}


def _prec(name):
    from neuralrecon_w_amd import lib as L

    return {"f32": L.PREC_F32, "bf16": L.PREC_BF16, "f16": L.PREC_F16}[name]


def _tiled(entry):
    return entry.startswith("tiled")


@functools.lru_cache(maxsize=None)
def _ints(n, cols, seed, lo=-2, hi=2):
    """[n, cols] int64 drawn from {lo .. hi}; cached, never modified (callers clone before they write)"""
    return torch.randint(lo, hi + 1, (n, cols), generator=torch.Generator().manual_seed(seed))


class Product:
    """One row of the descriptor table.  X [n, 32 rbx], Y [n, 32 rby]: int64 (exact cases) or float rows; dense / dbias: keys
    of the launch's output buffers; col0: column offset applied to the dense pointer; ksplit / n_points: the per-product
    overrides (0 = launch-wide); count: value of *n_points_dev, or None for a NULL pointer."""

    def __init__(self, X, Y, dense, col0=0, dbias=None, ksplit=0, n_points=0, count=None):
        self.X, self.Y, self.dense, self.col0, self.dbias = X, Y, dense, col0, dbias
        self.ksplit, self.n_points, self.count = ksplit, n_points, count
        self.rbx, self.rby = X.shape[1] // 32, Y.shape[1] // 32
        assert X.shape[0] == Y.shape[0] and X.shape[1] == 32 * self.rbx and Y.shape[1] == 32 * self.rby


def _call(entry, prec_name, specs, n_points, ksplit, n_desc=None, partials="nan", prec=None, tile=None):
    """Builds the device table and the workgroup prefix of `specs` -- dicts(x, y, dense, dbias, count: device addresses or
    None; rbx, rby, ld, ksplit, n_points) -- and calls the entry point.  -> its return code (after a synchronise)."""
    from neuralrecon_w_amd import lib as L

    lib = L.get_lib()
    xb, yb = WG_BLOCKS[entry]
    descs, prefix = [], [0]
    for s in specs:
        d = L.NcwWgradDesc()
        d.x, d.y, d.dense, d.dbias = s["x"], s["y"], s["dense"], s.get("dbias")
        d.rbx, d.rby, d.ld = s["rbx"], s["rby"], s["ld"]
        d.ksplit, d.n_points, d.n_points_dev = s.get("ksplit", 0), s.get("n_points", 0), s.get("count")
        descs.append(d)
        ks = s.get("ksplit", 0) if (_tiled(entry) and s.get("ksplit", 0) > 0) else ksplit
        prefix.append(prefix[-1] + ((s["rbx"] + xb - 1) // xb) * ((s["rby"] + yb - 1) // yb) * max(ks, 1))
    arr = (L.NcwWgradDesc * len(descs))(*descs)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    pre = torch.tensor(prefix, dtype=torch.int32, device="cuda")
    nd = len(descs) if n_desc is None else n_desc
    total = prefix[-1]
    p = _prec(prec_name) if prec is None else prec
    st = L.stream_ptr()
    if entry == "wgrad":
        rc = lib.ncw_wgrad(L.ptr(tab), L.ptr(pre), nd, total, ksplit, p, n_points, st)
    elif entry == "ordered":
        scr = None
        if partials == "nan":  # its contents are irrelevant on entry
            scr = torch.full((int(lib.ncw_wgrad_ordered_scratch_floats(total)),), float("nan"), device="cuda")
        rc = lib.ncw_wgrad_ordered(L.ptr(tab), L.ptr(pre), nd, total, ksplit, p, n_points, L.ptr(scr), st)
    else:
        fn = lib.ncw_wgrad_tiled_f16 if prec_name == "f16" else lib.ncw_wgrad_tiled
        rc = fn(L.ptr(tab), L.ptr(pre), nd, total, ksplit, int(entry[-1]) if tile is None else tile, n_points, st)
    sync_or_stop()
    return rc


def _covered(entry, p, n_points):
    """points product p covers: the launch-wide count, its own override (tiled entry points), clamped by *n_points_dev"""
    m = p.n_points if (_tiled(entry) and p.n_points > 0) else n_points
    return m if p.count is None else min(m, max(p.count, 0))


def _run_exact(entry, prec_name, prods, dense_shapes, bias_sizes, n_points, ksplit, seed=0):
    """Launch `prods` over integer operands and require the int64 reference in every output buffer, everywhere."""
    dtype = DTYPES[prec_name]
    dense0 = {k: _ints(r, ld, 900 + seed + i, -3, 3) for i, (k, (r, ld)) in enumerate(dense_shapes.items())}
    bias0 = {k: _ints(1, m, 950 + seed + i, -3, 3)[0] for i, (k, m) in enumerate(bias_sizes.items())}
    ref_d = {k: v.clone() for k, v in dense0.items()}
    ref_b = {k: v.clone() for k, v in bias0.items()}
    vecs = []
    for p in prods:
        m = _covered(entry, p, n_points)
        X = p.X.clone()
        # the kernels work in whole tiles: X is zero in the padded lanes of the last covered tile (what the producers write
        # there: their cotangents carry the lane mask); Y keeps its values, and both keep theirs beyond that tile
        X[m:32 * n_tiles(m)] = 0
        assert n_tiles(m) <= n_tiles(X.shape[0])  # every tile the launch may read exists
        r, ld = dense_shapes[p.dense]
        assert 32 * p.rbx <= r and p.col0 + 32 * p.rby <= ld and (p.dbias is None or 32 * p.rbx <= bias_sizes[p.dbias])
        prod = (X[:m].double().t() @ p.Y[:m].double()).to(torch.int64)  # exact: integers far below 2^53
        ref_d[p.dense][:32 * p.rbx, p.col0:p.col0 + 32 * p.rby] += prod
        if p.dbias is not None:
            ref_b[p.dbias][:32 * p.rbx] += X[:m].sum(0)
        vecs += [stash_encode(X.float(), p.rbx, dtype), stash_encode(p.Y.float(), p.rby, dtype)]
    assert max(int(v.abs().max()) for v in list(ref_d.values()) + list(ref_b.values())) < 2 ** 24
    cv = Carved(vecs, "cuda")
    dd = {k: v.float().cuda() for k, v in dense0.items()}
    bb = {k: v.float().cuda() for k, v in bias0.items()}
    counts = [None if p.count is None else torch.tensor([p.count], dtype=torch.int32, device="cuda") for p in prods]
    specs = [dict(x=cv.ptr(2 * i), y=cv.ptr(2 * i + 1), dense=dd[p.dense].data_ptr() + 4 * p.col0,
                  dbias=None if p.dbias is None else bb[p.dbias].data_ptr(), rbx=p.rbx, rby=p.rby,
                  ld=dense_shapes[p.dense][1], ksplit=p.ksplit, n_points=p.n_points,
                  count=None if counts[i] is None else counts[i].data_ptr()) for i, p in enumerate(prods)]
    assert _call(entry, prec_name, specs, n_points, ksplit) == 0
    for k in dd:
        got, want = dd[k].cpu(), ref_d[k].float()
        assert torch.equal(got, want), "dense %s: %d of %d elements differ, largest |difference| %s" % (
            k, int((got != want).sum()), got.numel(), float((got.double() - want.double()).abs().nan_to_num(1e30).max()))
    for k in bb:
        got, want = bb[k].cpu(), ref_b[k].float()
        assert torch.equal(got, want), "dbias %s: %s" % (k, (got - want).tolist())
    assert cv.gaps_untouched()


# (rbx, rby, n, launch-wide ksplit, dbias, ld > 32 rby with a column offset)
#   blocks: (1,1) one block, two of four waves idle; (3,2) odd remainders inside a quadrant; (5,9) one block past a full
#   quadrant on both axes for 4x4, 4x8 and 8x8 (with dbias: a column sum added once per qj shows); (8,8); (16,2) W = 512 x narrow
#   points: 1 / 31 / 32 / 33 tile boundaries; 65 = three tiles (the bf16 generic kernel's two-tile chunk gets a one-tile tail);
#   96 = three tiles, fewer than the DMA ring's four buffers; 229 / 3 = eight tiles in slices of 3, 3, 2; 40 / 4 = two tiles and
#   two EMPTY slices (zero slabs in the ordered variant, early return in the DMA kernel); 4001 / 16 = many tiles
CASES = [(1, 1, 1, 1, True, True), (1, 1, 31, 1, False, False), (3, 2, 32, 1, True, False), (3, 2, 33, 1, False, True),
         (5, 9, 65, 1, True, True), (5, 9, 229, 3, True, False), (5, 9, 40, 4, False, True), (8, 8, 96, 1, True, False),
         (8, 8, 229, 3, False, True), (16, 2, 4001, 16, True, True), (5, 9, 4001, 16, True, False),
         (16, 2, 40, 4, True, False)]


@pytest.mark.parametrize("rbx,rby,n,ksplit,bias,offset", CASES)
@pytest.mark.parametrize("entry,prec_name", PAIRS, ids=PAIR_IDS)
def test_single_product_is_exact(entry, prec_name, rbx, rby, n, ksplit, bias, offset):
    X, Y = _ints(n, 32 * rbx, 1), _ints(n, 32 * rby, 2)
    col0, ld = (32, 32 * rby + 96) if offset else (0, 32 * rby)
    _run_exact(entry, prec_name, [Product(X, Y, "w", col0, "b" if bias else None)], {"w": (32 * rbx, ld)},
               {"b": 32 * rbx}, n, ksplit)


@pytest.mark.parametrize("entry,prec_name", PAIRS, ids=PAIR_IDS)
def test_batched_launch_is_exact(entry, prec_name):
    """Three products of different shapes in one table -- the binary search over the workgroup prefix.  The first and the
    third add into the same dense region and the same dbias, as the first- and second-order products of one Linear do.
    Tiled entry points: per-product ksplit 1, 3, 2 and n_points 229, 65, 4001 under a launch-wide n_points of 4001 and a
    launch-wide ksplit that none of them uses; the prefix follows the per-product splits."""
    if _tiled(entry):
        ns, kss, launch_n, launch_ks = (229, 65, 4001), (1, 3, 2), 4001, 5
    else:
        ns, kss, launch_n, launch_ks = (229, 229, 229), (0, 0, 0), 229, 3
    shapes = [(5, 9), (1, 1), (5, 2)]
    prods = []
    for i, ((rbx, rby), n, ks) in enumerate(zip(shapes, ns, kss)):
        prods.append(Product(_ints(n, 32 * rbx, 10 + i), _ints(n, 32 * rby, 20 + i), "a" if i != 1 else "b", 32,
                             "a" if i != 1 else "b", ks, n if _tiled(entry) else 0))
    _run_exact(entry, prec_name, prods, {"a": (160, 32 * 9 + 96), "b": (32, 32 + 96)}, {"a": 160, "b": 32}, launch_n, launch_ks)


@pytest.mark.parametrize("count", [0, 1, 33, 100, 300])
@pytest.mark.parametrize("entry,prec_name", PAIRS, ids=PAIR_IDS)
def test_device_side_point_count(entry, prec_name, count):
    """*n_points_dev under n_points = 229 (300 clamps): the product is X[:count]^T Y[:count] given X = 0 in the padded
    lanes of the last covered tile; the tiles behind it hold ordinary values and must not be read."""
    X, Y = _ints(229, 160, 31), _ints(229, 288, 32)
    _run_exact(entry, prec_name, [Product(X, Y, "w", 0, "b", count=count)], {"w": (160, 288)}, {"b": 160}, 229, 3)


def _tiny_specs(keep):
    x = torch.zeros(1024, device="cuda")  # one tile of one block in any of the three element types
    dense = torch.full((32, 32), 7.0, device="cuda")
    keep += [x, dense]
    return [dict(x=x.data_ptr(), y=x.data_ptr(), dense=dense.data_ptr(), rbx=1, rby=1, ld=32)], dense


@pytest.mark.parametrize("entry,prec_name", PAIRS, ids=PAIR_IDS)
def test_argument_handling(entry, prec_name):
    keep = []
    specs, dense = _tiny_specs(keep)
    assert _call(entry, prec_name, specs, 32, 0) == NCW_E_BADARG  # ksplit = 0
    if _tiled(entry):
        assert _call(entry, prec_name, specs, 32, 1, tile=2) == NCW_E_BADARG
    else:
        assert _call(entry, prec_name, specs, 32, 1, prec=7) == NCW_E_BADARG  # unknown precision
    if entry == "ordered":
        assert _call(entry, prec_name, specs, 32, 1, partials=None) == NCW_E_BADARG
    assert _call(entry, prec_name, specs, 0, 1) == 0  # n_points = 0: nothing to do
    assert _call(entry, prec_name, specs, 32, 1, n_desc=0) == 0
    assert bool((dense == 7.0).all())
    assert _call(entry, prec_name, specs, 32, 1) == 0  # and the same table does run: 7 + 0
    assert bool((dense == 7.0).all())


@pytest.mark.parametrize("entry,prec_name", PAIRS, ids=PAIR_IDS)
def test_accumulation_error_of_real_valued_rows(entry, prec_name):
    """(5, 9) blocks, 4001 standard-normal points, ksplit 16.  The library rounds the rows into the stash
    (ncw_stash_from_rows); the reference is the fp64 product of the DECODED values, so only the accumulation is measured:
        |got - ref| <= 2 n 2^-24 sum_p |x_pi y_pj|
    the forward bound of an fp32 sum of n terms in any order (n u sum|terms|, u = 2^-24), the products of two 16-bit values
    being exact in fp32 and the factor 2 covering the product rounding of the fp32 mode.  A 16-bit accumulator misses it by
    orders of magnitude.  The bias column sums get the same bound over |x_pi|.  Ordered variant: twice, identical bits."""
    from neuralrecon_w_amd import lib as L

    n, rbx, rby, ksplit = 4001, 5, 9, 16
    dtype, prec = DTYPES[prec_name], _prec(prec_name)
    g = torch.Generator().manual_seed(5)
    rows = [torch.randn(n, 32 * rbx, generator=g), torch.randn(n, 32 * rby, generator=g)]
    T = n_tiles(n)
    cv = Carved([torch.full((T, rb, 4, 64, 4), float("nan"), dtype=dtype) for rb in (rbx, rby)], "cuda")
    for i, rb in enumerate((rbx, rby)):
        r = rows[i].cuda()
        L.check(L.get_lib().ncw_stash_from_rows(prec, L.ptr(r), n, 32 * rb, rb, cv.ptr(i), L.stream_ptr()), "ncw_stash_from_rows")
    sync_or_stop()
    Xd, Yd = (stash_decode(cv.view(i).cpu(), n, 32 * rb).double() for i, rb in enumerate((rbx, rby)))
    assert torch.equal(Xd, rows[0].to(dtype).double())
    ref, ref_b = Xd.t() @ Yd, Xd.sum(0)
    bound, bound_b = 2 * n * 2.0 ** -24 * (Xd.abs().t() @ Yd.abs()), 2 * n * 2.0 ** -24 * Xd.abs().sum(0)
    outs = []
    for _ in range(2 if entry == "ordered" else 1):
        dense, dbias = torch.zeros(32 * rbx, 32 * rby, device="cuda"), torch.zeros(32 * rbx, device="cuda")
        spec = dict(x=cv.ptr(0), y=cv.ptr(1), dense=dense.data_ptr(), dbias=dbias.data_ptr(), rbx=rbx, rby=rby, ld=32 * rby)
        assert _call(entry, prec_name, [spec], n, ksplit) == 0
        outs.append((dense.cpu(), dbias.cpu()))
    ratio = float(((outs[0][0].double() - ref).abs() / bound).max())
    ratio_b = float(((outs[0][1].double() - ref_b).abs() / bound_b).max())
    print("wgrad rounding %s %s: largest |got - ref| / bound = %.3e (dense), %.3e (dbias)" % (entry, prec_name, ratio, ratio_b))
    assert ratio <= 1.0 and ratio_b <= 1.0, (ratio, ratio_b)
    if entry == "ordered":
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
        assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
