"""TEST INFRASTRUCTURE ONLY: numpy restatement of csrc/ncw_synth.hip for tests/test_synth_host.py and tests/test_gpu_synth.py.
`shade` runs in float32 with every product, sum and quotient rounded once in the kernel's order (dtype=np.float64 runs the same
sequence in float64: the yardstick of the pixel-convention test); `observe` is float64.  Philox comes from tests/_surf_ref.py."""
import numpy as np

from tests._surf_ref import philox4x32_10

LIM = 2.0 ** 30


def lattice(ix, iy, iz, seed, octave, dtype=np.float32):
    """(w0 >> 8) 2^-24 of Philox4x32-10 of counter (ix, iy, iz, seed), key (octave, 0); ix.. int64 arrays (taken mod 2^32)."""
    ix, iy, iz = [np.asarray(v, dtype=np.int64) & 0xFFFFFFFF for v in (ix, iy, iz)]
    ctr = np.stack([ix, iy, iz, np.full_like(ix, int(seed) & 0xFFFFFFFF)], -1).astype(np.uint64)
    w = philox4x32_10(ctr.reshape(-1, 4), (octave, 0))[:, 0].reshape(ix.shape)
    return ((w >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)).astype(dtype)


def _lerp(a, b, t):
    return a + t * (b - a)


def value_noise(q, seed, octave, dtype=np.float32):
    """Trilinear value noise at q [n, 3] (dtype), x first, then y, then z; lattice coordinates clamped to +-2^30."""
    q = np.asarray(q, dtype=dtype)
    with np.errstate(invalid="ignore"):
        f = np.fmin(np.fmax(np.floor(q), dtype(-LIM)), dtype(LIM)).astype(dtype)
        t = (q - f).astype(dtype)
    i = f.astype(np.int64)
    h = lambda dx, dy, dz: lattice(i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz, seed, octave, dtype)
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    c00, c10 = _lerp(h(0, 0, 0), h(1, 0, 0), tx), _lerp(h(0, 1, 0), h(1, 1, 0), tx)
    c01, c11 = _lerp(h(0, 0, 1), h(1, 0, 1), tx), _lerp(h(0, 1, 1), h(1, 1, 1), tx)
    return _lerp(_lerp(c00, c10, ty), _lerp(c01, c11, ty), tz).astype(dtype)


def _clamp01(v, dtype):
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(v, dtype(0)), dtype(1)).astype(dtype)


def _mul34(M, x, y, z):
    return [M[4 * a] * x + M[4 * a + 1] * y + M[4 * a + 2] * z + M[4 * a + 3] for a in range(3)]


def shade(depth_ss, face_ss, img, face_normal, face_material, materials, dtype=np.float32, with_points=False):
    """ncw_synth_shade.  img: dict of the NcwSynthImage fields (python floats / lists, already float32-representable when the
    kernel is compared); materials: list of dicts base [3], freq, amp, label.  Returns rgb uint8 [h, w, 3], label uint8 [h, w],
    depth float32 [h, w]; with_points also the GT-frame point of the centre sub-sample [h, w, 3] (dtype; NaN without a face)."""
    F = dtype
    h, w, ss = int(img["height"]), int(img["width"]), int(img["ss"])
    depth_ss = np.asarray(depth_ss, dtype=np.float32).reshape(h * ss, w * ss)
    face_ss = np.asarray(face_ss, dtype=np.int64).reshape(h * ss, w * ss)
    nf = len(face_material)
    fn = np.asarray(face_normal, dtype=F).reshape(-1, 3)
    fm = np.minimum(np.asarray(face_material, dtype=np.int64), len(materials) - 1)
    base = np.array([m["base"] for m in materials], dtype=F).reshape(-1, 3)
    freq = np.array([m["freq"] for m in materials], dtype=F)
    amp = np.array([m["amp"] for m in materials], dtype=F)
    mlabel = np.array([m["label"] for m in materials], dtype=np.int64)
    c2w, s2g = [F(v) for v in img["c2w"]], [F(v) for v in img["sfm2gt"]]
    light = [F(v) for v in img["light"]]
    gain, bias = [F(v) for v in img["gain"]], [F(v) for v in img["bias"]]
    top, bot = [F(v) for v in img["sky_top"]], [F(v) for v in img["sky_bottom"]]
    fx, fy, cx, cy = F(img["fx"]), F(img["fy"]), F(img["cx"]), F(img["cy"])
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rf, cf = r.astype(F), c.astype(F)
    trow = (rf / F(h)).astype(F)
    sky = [_clamp01(_lerp(top[ch], bot[ch], trow), F) for ch in range(3)]
    acc = [np.zeros((h, w), dtype=F) for _ in range(3)]
    lab = np.full((h, w), int(img["sky_label"]), dtype=np.int64)
    dep = np.zeros((h, w), dtype=np.float32)
    gpt = np.full((h, w, 3), np.nan, dtype=F)
    for j in range(ss):
        for i in range(ss):
            d32 = depth_ss[j::ss, i::ss]
            f = face_ss[j::ss, i::ss]
            hit = (f >= 0) & (f < nf) & (d32 > 0)
            fs = np.where(hit, f, 0)
            d = d32.astype(F)
            px = (cf + (F(i) + F(0.5)) / F(ss) - F(0.5)).astype(F)
            py = (rf + (F(j) + F(0.5)) / F(ss) - F(0.5)).astype(F)
            X, Y = ((px - cx) / fx) * d, ((py - cy) / fy) * d
            wx, wy, wz = _mul34(c2w, X, Y, d)
            g = np.stack(_mul34(s2g, wx, wy, wz), -1).astype(F)
            m = fm[fs] if nf else np.zeros_like(fs)
            f0 = freq[m]
            n, wgt = np.zeros((h, w), dtype=F), F(0.5)
            for o in range(3):
                q = (g * f0[..., None]).astype(F)
                n = n + wgt * value_noise(q.reshape(-1, 3), img["tex_seed"], o, F).reshape(h, w)
                f0 = f0 * F(2)
                wgt = wgt * F(0.5)
            tex = F(1) + amp[m] * (n - F(0.4375))
            nrm = fn[fs] if nf else np.zeros((h, w, 3), dtype=F)
            ndl = nrm[..., 0] * light[0] + nrm[..., 1] * light[1] + nrm[..., 2] * light[2]
            lam = F(img["ambient"]) + F(img["diffuse"]) * np.fmax(F(0), ndl)
            for ch in range(3):
                v = _clamp01(gain[ch] * ((base[m][..., ch] * tex) * lam) + bias[ch], F)
                acc[ch] = (acc[ch] + np.where(hit, v, sky[ch])).astype(F)
            if j == ss // 2 and i == ss // 2:
                lab = np.where(hit, mlabel[m], int(img["sky_label"]))
                dep = np.where(hit, d32, np.float32(0))
                gpt = np.where(hit[..., None], g, F(np.nan))
    cnt = F(ss * ss)
    rgb = np.stack([((a / cnt) * F(255) + F(0.5)).astype(F).astype(np.int64) for a in acc], -1).astype(np.uint8)
    out = (rgb, lab.astype(np.uint8), dep.astype(np.float32))
    return out + (gpt,) if with_points else out


def usum4(index, serial, call, seed):
    """(((u0 + u1) + u2) + u3) - 2 of the four 24-bit uniforms of Philox(counter (index, index >> 32, serial, call), key seed)."""
    idx = np.asarray(index, dtype=np.int64).astype(np.uint64)
    ctr = np.stack([idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), np.full_like(idx, serial), np.full_like(idx, call)], -1)
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return (((u[:, 0] + u[:, 1]) + u[:, 2]) + u[:, 3]) - 2.0


def observe(pts, nrm, index, view, depth):
    """ncw_synth_observe.  view: dict of the NcwSynthView fields.  Returns xy [n, 2], err2 [n] float64, vis uint8 [n]."""
    p, nr = np.asarray(pts, dtype=np.float64).reshape(-1, 3), np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    M = [float(v) for v in view["w2c"]]
    ce = [float(v) for v in view["centre"]]
    h, w = int(view["height"]), int(view["width"])
    depth = np.asarray(depth, dtype=np.float32).reshape(h, w)
    x, y, z = _mul34(M, p[:, 0], p[:, 1], p[:, 2])
    front = z > view["znear"]
    with np.errstate(all="ignore"):
        u = view["fx"] * (x / z) + view["cx"]
        v = view["fy"] * (y / z) + view["cy"]
        facing = nr[:, 0] * (ce[0] - p[:, 0]) + nr[:, 1] * (ce[1] - p[:, 1]) + nr[:, 2] * (ce[2] - p[:, 2])
        nx = view["sigma_r3"] * usum4(index, view["serial"], 0, view["seed"])
        ny = view["sigma_r3"] * usum4(index, view["serial"], 1, view["seed"])
        cu, cv = np.floor(u + 0.5), np.floor(v + 0.5)
        inside = (cu >= 0) & (cu < w) & (cv >= 0) & (cv < h)
        seen = front & (facing > 0) & inside
        col, row = np.where(seen, cu, 0).astype(np.int64), np.where(seen, cv, 0).astype(np.int64)
        d = depth[row, col].astype(np.float64)
        seen &= (d > 0) & (np.abs(z - d) <= view["depth_tol"] * z)
    xy = np.where(front[:, None], np.stack([u + nx, v + ny], -1), 0.0)
    err2 = np.where(front, nx * nx + ny * ny, 0.0)
    return xy, err2, seen.astype(np.uint8)
