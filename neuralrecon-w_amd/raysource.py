"""Training rays straight from a scene: no ray cache on disk, no dense rows in HBM.

    source = RaySource.from_scene("data/heritage-recon/brandenburg_gate", semantic_map_path="semantic_maps",
                                  ray_mask_list=["person", "car"], prefilter=True)
    for b in source.epoch(2048, generator=gen, drop_last=True): ...

`RaySource` has `raycache.RayCache`'s surface (`__len__`, `batch`, `filtered`, `epoch`, `prefiltered`, `mask_ids`), so
scripts/train.py holds either.  Where the cache keeps 64 bytes per ray (13 + 3 floats), written by `cachebuild.build_cache`,
compressed, read back and uploaded, the source keeps an 8-byte record per kept ray -- pixel index, a key-point flag, the uint8
pixel and its label -- plus one camera per image, the key-points that land on a kept pixel, and the range octree; every batch is
ONE launch (`ncw_source_batch`, csrc/ncw_source.hip) that rebuilds the rows `RayCache.batch` returns for the same rays, bit for
bit, with the device functions `ncw_cache_rows` uses.  Replaces datasets/phototourism.py:557-657, 709-726 and the black-list
test of neuconw_system.py:345-349, like the cache path it stands beside.

Building (`from_images`) runs `cachebuild.sfm_depth_planes` + `cachebuild.cache_rows` once per image -- what `build_image`
runs -- and keeps only the records: nothing about the selection, the labels or the key-point depths is restated here.
Changing `img_downscale`, the label maps, the SfM model or `voxel_size` needs no files rewritten.
"""
import ctypes as C

import numpy as np
import torch

from . import cachebuild
from . import lib as L
from .labels import label_id
from .raycache import RayCache, shuffled_epoch

PIX_MASK = 0x7FFFFFFF   # NcwSourceRec.pix bits 0..30; bit 31: the pixel has an entry in the key-point table
PIX_LIMIT = 2 ** 31 - 1  # pixel indices stay below this: the kernel's row / col arithmetic is int32


def rank_share(n, world_size, rank):
    """The global record numbers rank `rank` of `world_size` keeps out of n: g with g % world_size == rank (numbered over all
    images in order, after padding and prefilter).  The ranks' shares are disjoint, cover range(n), and differ in length by at
    most one.  Returns (first, step) of that arithmetic progression and its length."""
    n, world_size, rank = int(n), int(world_size), int(rank)
    if world_size < 1 or not 0 <= rank < world_size:
        raise ValueError("rank_share: rank %d of world size %d" % (rank, world_size))
    return rank, world_size, max(0, (n - rank + world_size - 1) // world_size)


def pack_records(pix, rgb, label, has_kp):
    """NcwSourceRec as int32 words [n, 2] (tensors on any device): word 0 = pix | has_kp << 31, word 1 = r | g << 8 | b << 16 |
    label << 24 (the struct's bytes, little-endian).  pix int64 [n] in [0, 2^31 - 1); rgb uint8 [n, 3]; label [n] in 0..255 or
    None (0); has_kp bool [n]."""
    pix = torch.as_tensor(pix).to(torch.int64).reshape(-1)
    n = pix.shape[0]
    if n and (int(pix.min()) < 0 or int(pix.max()) >= PIX_LIMIT):
        raise ValueError("pack_records: pixel index outside [0, 2^31 - 1): the record holds 31 bits")
    rgb = torch.as_tensor(rgb).reshape(n, 3).to(torch.int64)
    lab = torch.zeros(n, dtype=torch.int64, device=pix.device) if label is None else torch.as_tensor(label).to(torch.int64).reshape(n)
    if n and (int(lab.min()) < 0 or int(lab.max()) > 255 or int(rgb.min()) < 0 or int(rgb.max()) > 255):
        raise ValueError("pack_records: rgb and label are bytes")
    w0 = pix | (torch.as_tensor(has_kp).to(torch.int64).reshape(n) << 31)
    w1 = rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16) | (lab << 24)
    words = torch.stack([w0, w1], 1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)  # the same 32 bits as a signed word
    return words.to(torch.int32).contiguous()


def unpack_records(words):
    """The inverse of `pack_records`: (pix int64 [n], rgb uint8 [n, 3], label int64 [n], has_kp bool [n])."""
    w = torch.as_tensor(words).to(torch.int64).reshape(-1, 2) & 0xFFFFFFFF
    w0, w1 = w[:, 0], w[:, 1]
    rgb = torch.stack([w1 & 255, (w1 >> 8) & 255, (w1 >> 16) & 255], 1).to(torch.uint8)
    return w0 & PIX_MASK, rgb, (w1 >> 24) & 255, (w0 >> 31) != 0


def depth_padding(depth, depth_percent, generator):
    """The indices `cachebuild.pad_depth_percent` appends (phototourism.py:659-675) for an image whose kept rows have the
    key-point depths `depth` [m]: positions among the m rows, drawn with the same calls in the same order -- including the
    `randperm` it applies afterwards, which is consumed and NOT applied (`epoch` shuffles), so `generator` stays aligned with
    `build_cache`'s."""
    valid = depth > 0
    valid_num = int(valid.sum())
    cur = int(depth.shape[0])
    pad = int(np.ceil((depth_percent * cur - valid_num) / (1 - depth_percent)))
    pad = max(pad, 0) if valid_num > 0 else 0
    pad_ind = torch.floor(torch.rand(pad, generator=generator) * valid_num).long().to(depth.device)
    torch.randperm(cur + pad, generator=generator)
    return valid.nonzero().reshape(-1)[pad_ind]


def image_table(cameras, image_ids):
    """NcwSourceImage [n_img] as a uint8 tensor (host)."""
    arr = (L.NcwSourceImage * len(cameras))()
    for k, (cam, iid) in enumerate(zip(cameras, image_ids)):
        arr[k].cam = cam.struct()
        arr[k].ts = int(iid)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)


class RaySource:
    """The rank's training rays as records, resident on `device`.  batch(idx) -> the dictionary `RayCache.batch` returns."""

    def __init__(self, recs, images, row_start, kp_start, kp_pix, kp_depth, kp_weight, range_octree, voxel_size, with_semantics,
                 ray_mask_list=None, prefiltered=False):
        self.device = recs.device
        self.recs, self.images, self.row_start, self.kp_start = recs, images, row_start, kp_start
        self.kp_pix, self.kp_depth, self.kp_weight = kp_pix, kp_depth, kp_weight
        self.n_img = int(row_start.shape[0]) - 1
        self.range_octree, self.voxel_size = range_octree, float(voxel_size)
        self.with_semantics = bool(with_semantics)
        ids = [label_id(n) for n in (ray_mask_list or [])]
        if len(ids) > 4:
            raise NotImplementedError("RAY_MASK_LIST with more than 4 labels")
        self.mask_ids = ids
        self._ids_arr = (C.c_int * 4)(*(ids + [0] * (4 - len(ids))))
        self.prefiltered = bool(prefiltered)

    def __len__(self):
        return int(self.recs.shape[0])

    def nbytes(self):
        """Bytes resident on the device: records, image table, row / key-point starts, key-points (the SfM octrees, which the
        renderer's coarse octree also needs, are not counted)."""
        return sum(int(t.numel()) * t.element_size() for t in (self.recs, self.images, self.row_start, self.kp_start, self.kp_pix,
                                                               self.kp_depth, self.kp_weight))

    # ------------------------------------------------------------------------------------------------
    @classmethod
    def from_images(cls, items, hit_octree=None, range_octree=None, voxel_size=0.0, depth_percent=0.0, generator=None,
                    ray_mask_list=None, prefilter=False, world_size=1, rank=0, device=None):
        """items: per image the arguments of `cachebuild.build_image` -- (camera, decoded uint8 image [h, w, 3], image id,
        key-point tuple, w2c, label map or None); all with a label map or none.  hit_octree / range_octree / voxel_size: as
        `build_image` takes them (either octree None: every pixel is a ray with the camera's near / far).
        depth_percent / generator: `cachebuild.pad_depth_percent`'s padding (copies of records; a CPU torch.Generator).
        ray_mask_list + prefilter: black-listed records are dropped here, as `RayCache(prefilter=True)` drops rows (every `keep`
        is then true); without prefilter `batch` returns the flags.
        world_size / rank: this rank's share of the records (`rank_share`); every rank builds all images."""
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise L.NeuconwHipError("raysource.RaySource: not a GPU device; the ray source has no CPU fallback")
        first, step, _ = rank_share(0, world_size, rank)
        use_voxel = hit_octree is not None and range_octree is not None
        ids = [label_id(n) for n in (ray_mask_list or [])]
        gen = generator
        cams, iids, recs, kps = [], [], [], []
        row_start, kp_start = [0], [0]
        with_sem = None
        g0 = 0  # global number of the image's first record
        for cam, image, image_id, kp, w2c, label_map in items:
            sem = label_map is not None
            if with_sem is None:
                with_sem = sem
            elif sem != with_sem:
                raise ValueError("RaySource.from_images: some images have a label map and some have none")
            if cam.width * cam.height > PIX_LIMIT:
                raise ValueError("RaySource.from_images: a %d x %d image has pixel indices beyond 31 bits" % (cam.width, cam.height))
            xyz, err, px, err_mean = kp
            depth_z, weight = cachebuild.sfm_depth_planes(xyz, err, px, err_mean, w2c, cam.width, cam.height, device)
            img = cachebuild._dev_u8(image, device)
            lab = cachebuild._dev_u8(label_map, device) if sem else None
            rows, _, keep = cachebuild.cache_rows(cam, img, image_id, depth_z, weight, lab, hit_octree, range_octree, voxel_size)
            nc = rows.shape[1]
            pix = keep.nonzero().reshape(-1) if use_voxel else torch.arange(rows.shape[0], device=device)
            kept = rows[pix]
            del rows, depth_z, weight
            d, w = kept[:, nc - 3], kept[:, nc - 2]
            has_kp = (d != 0) | (w != 0)
            kpi = has_kp.nonzero().reshape(-1)  # pix ascends, so these entries are sorted by pixel
            kps.append((pix[kpi].to(torch.int32), d[kpi].clone(), w[kpi].clone()))
            kp_start.append(kp_start[-1] + int(kpi.shape[0]))
            rec = pack_records(pix, img.reshape(-1, 3)[pix], kept[:, 9].to(torch.int64) if sem else None, has_kp)
            if depth_percent > 0 and rec.shape[0] > 0:
                if gen is None:
                    gen = torch.Generator().manual_seed(0)
                rec = torch.cat([rec, rec[depth_padding(d, float(depth_percent), gen)]], 0)
            if prefilter and ids and sem:
                lab_r = unpack_records(rec)[2]
                ok = torch.ones_like(lab_r, dtype=torch.bool)
                for i in ids:
                    ok &= lab_r != i
                rec = rec[ok]
            m = int(rec.shape[0])
            if step > 1:  # this rank's share: global numbers g0 .. g0 + m - 1 with g % world_size == rank
                rec = rec[(first - g0) % step::step]
            g0 += m
            recs.append(rec.contiguous())
            row_start.append(row_start[-1] + int(rec.shape[0]))
            cams.append(cam)
            iids.append(int(image_id))
            del kept, d, w
        if not cams:
            raise ValueError("RaySource.from_images: no image")
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=device)  # noqa: E731
        return cls(torch.cat(recs, 0).contiguous(), image_table(cams, iids).to(device), i64(row_start), i64(kp_start),
                   torch.cat([k[0] for k in kps]).contiguous(), torch.cat([k[1] for k in kps]).contiguous(),
                   torch.cat([k[2] for k in kps]).contiguous(), range_octree if use_voxel else None, voxel_size if use_voxel else 0.0,
                   bool(with_sem), ray_mask_list, prefiltered=bool(prefilter and ids and with_sem))

    @classmethod
    def from_scene(cls, root_dir, img_downscale=1, semantic_map_path=None, sfm_path=None, seed=0, depth_percent=None,
                   use_voxel=True, scene_origin=None, scene_radius=None, ray_mask_list=None, prefilter=False, world_size=1, rank=0,
                   device=None, stats=None):
        """`cachebuild.build_cache`'s loop up to, and without, the files: the same readers, octrees and defaults
        (`cachebuild.open_scene` / `scene_items`), the records instead of the rows.  seed: the generator of the
        `depth_percent` padding, as `build_cache` seeds it."""
        if torch.device("cuda" if device is None else device).type != "cuda":
            raise L.NeuconwHipError("raysource.RaySource: not a GPU device; the ray source has no CPU fallback")
        sc = cachebuild.open_scene(root_dir, img_downscale, sfm_path, device, depth_percent, use_voxel, who="open_scene")
        if not sc["scene"]["ids_train"]:
            raise ValueError("%s lists no training image registered in images.bin" % sc["scene"]["tsv"])
        gen = torch.Generator().manual_seed(int(seed))
        return cls.from_images(cachebuild.scene_items(sc, semantic_map_path, scene_origin, scene_radius, stats), sc["hit"],
                               sc["range"], sc["voxel_size"], sc["depth_percent"], gen, ray_mask_list, prefilter, world_size, rank,
                               sc["device"])

    # ------------------------------------------------------------------------------------------------
    def batch(self, idx):
        """idx: int64 tensor [B] of record numbers on the device (None = every record in order)."""
        dev = self.device
        if dev.type != "cuda":
            raise L.NeuconwHipError("RaySource: the records are not on a GPU; batch assembly has no CPU fallback")
        n = len(self)
        B = n if idx is None else int(idx.shape[0])
        if idx is not None:
            idx = idx.to(dev, torch.int64).contiguous()
        rays = torch.empty(B, 11, device=dev)
        ts = torch.empty(B, dtype=torch.int64, device=dev)
        label = torch.empty(B, dtype=torch.int64, device=dev)
        rgbs = torch.empty(B, 3, device=dev)
        keep = torch.empty(B, dtype=torch.uint8, device=dev)
        if B > 0:
            if n == 0:
                raise L.NeuconwHipError("RaySource.batch: the source holds no ray")
            rng_s = cachebuild._octree_struct(self.range_octree) if self.range_octree is not None else None
            L.check(L.get_lib().ncw_source_batch(
                L.ptr(self.recs), n, L.ptr(self.images), L.ptr(self.row_start), L.ptr(self.kp_start), self.n_img,
                L.ptr(self.kp_pix) if self.kp_pix.numel() else None, L.ptr(self.kp_depth) if self.kp_pix.numel() else None,
                L.ptr(self.kp_weight) if self.kp_pix.numel() else None, C.byref(rng_s) if rng_s is not None else None,
                self.voxel_size, L.ptr(idx), B, int(self.with_semantics), L.ptr(rays), L.ptr(ts), L.ptr(label), L.ptr(rgbs),
                self._ids_arr, len(self.mask_ids), L.ptr(keep), L.stream_ptr(dev)), "ncw_source_batch")
        out = {"rays": rays, "ts": ts, "rgbs": rgbs, "keep": keep.bool()}
        if self.with_semantics:
            out["semantics"] = label
        return out

    filtered = staticmethod(RayCache.filtered)  # neuconw_system.py:345-353, the same boolean index

    def epoch(self, batch_size, generator=None, drop_last=False, max_batches=None, skip_batches=0):
        """`RayCache.epoch`: shuffled batches of one epoch, the same loop (raycache.shuffled_epoch)."""
        return shuffled_epoch(self, batch_size, generator, drop_last, max_batches, skip_batches)
