"""The fixture of the sfm2gt tests (tests/test_align_host.py, tests/test_gpu_align.py): a ground-truth cloud without symmetry,
far from the origin, and a source that is a subset of it carried back by a known similarity, plus outliers.  Built once per
process (`fixture()` caches) and never modified."""
import functools

import numpy as np

SEED = 16        # chosen so that the conditions of tests/test_align_host.py hold at every iteration of the restated run
GATE0, SHRINK, GATE_MIN = 0.4, 0.85, 0.01
OFFSET = np.array([100.0, -50.0, 20.0])
N_GT, N_SRC, N_OUT = 12000, 1500, 360


def rotation(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64)
    k = axis / np.linalg.norm(axis)
    a = np.radians(degrees)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def similarity(scale, axis, degrees, t, about=None):
    """4x4 [sR t; 0 1]; with `about` the rotation and scale act around that point (x -> sR (x - about) + about + t)."""
    T = np.eye(4)
    T[:3, :3] = scale * rotation(axis, degrees)
    T[:3, 3] = t
    if about is not None:
        about = np.asarray(about, dtype=np.float64)
        T[:3, 3] = about + T[:3, 3] - T[:3, :3] @ about
    return T


def apply(T, x):
    return np.asarray(x, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]


def surface(n, g):
    """n points on three unequal rectangles meeting at a corner (floor 3 x 2, wall 3 x 1.5, wall 2 x 1) with a Gaussian bump on
    the floor, area-weighted, offset to OFFSET."""
    areas = np.array([3 * 2, 3 * 1.5, 2 * 1.0])
    which = g.choice(3, size=n, p=areas / areas.sum())
    u, v = g.rand(n), g.rand(n)
    x = np.zeros((n, 3))
    f = which == 0
    x[f, 0], x[f, 1] = 3 * u[f], 2 * v[f]
    x[f, 2] = 0.4 * np.exp(-((x[f, 0] - 1.8) ** 2 + (x[f, 1] - 1.1) ** 2) / (2 * 0.3 ** 2))
    f = which == 1
    x[f, 0], x[f, 2] = 3 * u[f], 1.5 * v[f]
    f = which == 2
    x[f, 1], x[f, 2] = 2 * u[f], 1.0 * v[f]
    return x + OFFSET


def _dist_to_cloud(x, cloud, chunk=512):
    out = np.zeros(len(x))
    for s in range(0, len(x), chunk):
        d = x[s:s + chunk, None, :] - cloud[None, :, :]
        out[s:s + chunk] = np.sqrt((d * d).sum(-1).min(1))
    return out


def build(seed=SEED, rigid=False):
    g = np.random.RandomState(seed)
    gt = surface(N_GT, g)
    truth = similarity(1.0 if rigid else 3.7, [0.3, -0.5, 0.8], 40.0, [0.0, 0.0, 0.0])
    truth[:3, 3] = OFFSET - truth[:3, :3] @ np.array([0.7, -0.2, 0.4])      # the SfM frame sits near its own origin
    inv = np.linalg.inv(truth)
    pick = np.sort(g.choice(N_GT, size=N_SRC, replace=False))
    lo, hi = gt.min(0) - 0.3, gt.max(0) + 0.3
    out = lo + (hi - lo) * g.rand(N_OUT, 3)
    for _ in range(50):                                                      # outliers closer than 0.1 to the cloud are redrawn
        near = _dist_to_cloud(out, gt) < 0.1
        if not near.any():
            break
        out[near] = lo + (hi - lo) * g.rand(int(near.sum()), 3)
    assert not (_dist_to_cloud(out, gt) < 0.1).any()
    src = np.concatenate([apply(inv, gt[pick]), apply(inv, out)])
    order = g.permutation(len(src))                                          # inliers and outliers interleaved
    src = np.ascontiguousarray(src[order])
    partner = np.concatenate([pick, np.full(N_OUT, -1)])[order]
    centre = gt.mean(0)
    pert = similarity(1.0 if rigid else 1.1, [0.6, 0.7, -0.2], 15.0, 0.2 * np.array([0.6, -0.64, 0.48]), about=centre)
    return {"gt": gt, "src": src, "truth": truth, "init": pert @ truth, "partner": partner, "rigid": rigid,
            "far": similarity(1.0, [0.0, 0.0, 1.0], 90.0, [0.0, 0.0, 0.0], about=centre) @ truth}


@functools.lru_cache(maxsize=None)
def fixture(rigid=False):
    return build(SEED, rigid)


@functools.lru_cache(maxsize=None)
def restated(rigid=False, conditions=False):
    """(T, history, target) of the restated loop (tests/_align_ref.icp) on the fixture: computed once per process, shared."""
    from tests import _align_ref as R

    fx = fixture(rigid)
    target = R.Target(fx["gt"])
    T, hist = R.icp(fx["src"], target, fx["init"], GATE0, SHRINK, GATE_MIN, with_scale=not rigid, conditions=conditions)
    return T, hist, target


def true_pairs_error(fx):
    """The error of align.similarity_from_pairs given the fixture's true pairs: the yardstick of the loop's final matrix."""
    from neuralrecon_w_amd import align

    ok = fx["partner"] >= 0
    T = align.similarity_from_pairs(fx["src"][ok], fx["gt"][fx["partner"][ok]], with_scale=not fx["rigid"])
    return matrix_error(T, fx["truth"])


def scene_case(points3d_path, seed=2, n_extra=1500):
    """The end-to-end case on a COLMAP model: truth (4x4), gt = the model's own points carried by it plus `n_extra` further points
    of the same surface (midpoints between a point and one of its six nearest neighbours), shuffled, so that the SfM points are
    a strict subset; pairs [4,6] = four spread SfM points with their exact images perturbed by 1 % of the cloud's extent."""
    from neuralrecon_w_amd import colmap

    xyz = colmap.read_points3d(points3d_path)[1]
    g = np.random.RandomState(seed)
    truth = similarity(1.7, [0.2, -0.3, 0.9], 25.0, [10.0, -5.0, 3.0])
    d = np.linalg.norm(xyz[:, None] - xyz[None], axis=-1)
    near = np.argsort(d, axis=1)[:, 1:7]
    a = g.randint(0, len(xyz), n_extra)
    b = near[a, g.randint(0, 6, n_extra)]
    w = 0.25 + 0.5 * g.rand(n_extra, 1)
    extra = w * xyz[a] + (1 - w) * xyz[b]
    gt = apply(truth, np.concatenate([xyz, extra]))
    gt = np.ascontiguousarray(gt[g.permutation(len(gt))])
    picks = [int(np.argmin(xyz[:, 0])), int(np.argmax(xyz[:, 0])), int(np.argmax(xyz[:, 1])), int(np.argmin(xyz[:, 2]))]
    extent = float((gt.max(0) - gt.min(0)).max())
    noise = g.randn(4, 3)
    noise *= 0.01 * extent / np.linalg.norm(noise, axis=1, keepdims=True)
    pairs = np.concatenate([xyz[picks], apply(truth, xyz[picks]) + noise], -1)
    return {"src": xyz, "gt": gt, "truth": truth, "pairs": pairs, "rigid": False,
            "partner": None}


def matrix_error(T, truth):
    """max |T - truth| / max |truth|"""
    return float(np.abs(np.asarray(T) - truth).max() / np.abs(truth).max())
