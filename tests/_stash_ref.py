"""The activation-stash layout restated in plain torch, on the CPU, independently of the library's converters.

A stash vector of `rb` feature blocks over n points is `[tile32][rb][g = 4][lane = 64][c = 4]` elements (ceil(n / 32) tiles):
point 32 tile + p, feature 32 b + 8 g + 4 h + c sits at lane 32 h + p, element c of group g of block b.  Lanes past n and
features past F hold zero.  (include/neuconw_hip.h "Activation stash"; csrc/ncw_pack.hip stash_rows_kernel is the library's own
statement of it -- nothing here calls or imports it.)"""
import torch

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def n_tiles(n):
    return (int(n) + 31) // 32


def stash_encode(rows, rb, dtype=torch.float32):
    """rows [n, F <= 32 rb] -> stash [T, rb, 4, 64, 4] of `dtype` (rounded by torch's own conversion), zero padded."""
    n, F = rows.shape
    assert F <= 32 * rb
    T = n_tiles(n)
    pad = torch.zeros(T * 32, rb * 32, dtype=dtype)
    pad[:n, :F] = rows.to(dtype)
    # [T, p, b, g, h, c] -> [T, b, g, h, p, c]; lane = 32 h + p
    return pad.view(T, 32, rb, 4, 2, 4).permute(0, 2, 3, 4, 1, 5).reshape(T, rb, 4, 64, 4).contiguous()


def stash_decode(stash, n, F):
    """stash [T, rb, 4, 64, 4] (any float type) -> rows [n, F] in the stash's type."""
    T, rb = stash.shape[0], stash.shape[1]
    assert stash.shape[2:] == (4, 64, 4) and n <= 32 * T and F <= 32 * rb
    rows = stash.reshape(T, rb, 4, 2, 32, 4).permute(0, 4, 1, 2, 3, 5).reshape(T * 32, rb * 32)
    return rows[:n, :F].contiguous()


def stash_encode_loops(rows, rb, dtype=torch.float32):
    """The same layout, element by element: five loops over (tile, block, g, lane, c)."""
    n, F = rows.shape
    T = n_tiles(n)
    out = torch.zeros(T, rb, 4, 64, 4, dtype=dtype)
    r = rows.to(dtype)
    for t in range(T):
        for b in range(rb):
            for g in range(4):
                for lane in range(64):
                    for c in range(4):
                        h, p = lane // 32, lane % 32
                        point, feat = 32 * t + p, 32 * b + 8 * g + 4 * h + c
                        if point < n and feat < F:
                            out[t, b, g, lane, c] = r[point, feat]
    return out


def sync_or_stop():
    """torch.cuda.synchronize().  A GPU fault ends the whole session instead of failing one test: nothing more is started on
    a device that has faulted."""
    import pytest

    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU fault, stopping the session: %s" % e, returncode=3)


class Carved:
    """Several stash vectors inside ONE device buffer whose every other element -- in front of the first vector, between
    two vectors and behind the last -- is NaN in the element type: a kernel that reads a tile or a block that is not its
    own vector's poisons its result.  `gap` elements (a multiple of 128: the vectors stay 256-byte aligned like the
    arena's) separate them."""

    def __init__(self, vectors, device, gap=256):
        assert gap % 128 == 0 and len({v.dtype for v in vectors}) == 1
        dtype = vectors[0].dtype
        total = gap + sum(v.numel() + gap for v in vectors)
        self.buf = torch.full((total,), float("nan"), dtype=dtype, device=device)
        self.offsets, off = [], gap
        for v in vectors:
            self.buf[off:off + v.numel()] = v.reshape(-1).to(device)
            self.offsets.append((off, tuple(v.shape)))
            off += v.numel() + gap
        self.esize = self.buf.element_size()

    def ptr(self, i):
        return self.buf.data_ptr() + self.offsets[i][0] * self.esize

    def view(self, i):
        off, shape = self.offsets[i]
        n = 1
        for s in shape:
            n *= s
        return self.buf[off:off + n].view(shape)

    def gaps_untouched(self):
        """every element outside the vectors is still NaN"""
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for off, shape in self.offsets:
            n = 1
            for s in shape:
                n *= s
            mask[off:off + n] = False
        return bool(torch.isnan(self.buf[mask]).all())
