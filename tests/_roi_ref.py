"""float64 restatement of the region-of-interest test of the split writer (tools/prepare_data/dataset_filter_utils.py:168-177
over datasets/ray_utils.py:18-52) and the AMBIGUOUS BAND around its three comparisons.  Shared by
tests/golden/make_golden_split.py, tests/test_split_host.py and tests/test_gpu_roi.py.

The float32 chain (the reference's torch ops, csrc/ncw_roi.hip) rounds each operand a few tens of times: about
2e-6 (radius + dist_cam) on dist_ray.  The band is 50 times that and still a fraction of a pixel wide; a pixel inside it may
fall on either side in float32 and is excluded from exact comparisons, a pixel outside it may not."""
import numpy as np

BAND = 1e-4


def roi_f64(K, c2w, width, height, origin, radius):
    """Per pixel (row-major, [h * w]) of the view with float32 K [3,3] / c2w [3,4] taken as they are: dist_ray, dist_cam, dot,
    roi (bool) and band (bool), all from float64 arithmetic."""
    K, c2w = np.asarray(K, dtype=np.float64), np.asarray(c2w, dtype=np.float64)
    origin, radius = np.asarray(origin, dtype=np.float64), float(radius)
    col, row = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    dirs = np.stack([(col - K[0, 2]) / K[0, 0], -(row - K[1, 2]) / K[1, 1], -np.ones_like(col)], -1).reshape(-1, 3)
    d = dirs @ c2w[:, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = origin - c2w[:, 3]
    dot = d @ c
    dist_ray = np.linalg.norm(c[None] - dot[:, None] * d, axis=1)
    dist_cam = np.full(len(d), np.linalg.norm(c))
    roi = ((radius > dist_cam) | (dot > 0)) & (dist_ray < radius)
    band = (np.abs(dist_ray - radius) <= BAND * (radius + dist_cam)) | (np.abs(dist_cam - radius) <= BAND * radius) | \
        ((np.abs(dot) <= BAND * dist_cam) & (dist_cam >= radius * (1 - BAND)))
    return {"dist_ray": dist_ray, "dist_cam": dist_cam, "dot": dot, "roi": roi, "band": band}
