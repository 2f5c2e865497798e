// The pinhole ray arithmetic the view kernels share (ncw_view.hip: ncw_view_rays; ncw_cache.hip: the ray-cache rows):
// datasets/ray_utils.py:18-52 for one pixel, float32 like the dataset.
#pragma once
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

// d = c2w[:, :3] dir of pixel (row, col), NOT yet normalised; returns |d|
__device__ __forceinline__ float view_ray_dir(const NcwViewCamera& cam, int row, int col, float (&d)[3]) {
    // get_ray_directions: integer pixel coordinates, no +0.5 (ray_utils.py:18-24)
    const float dx = ((float)col - cam.cx) / cam.fx;
    const float dy = -((float)row - cam.cy) / cam.fy;
    const float dz = -1.f;
    // get_rays: directions @ c2w[:, :3]^T, normalised (ray_utils.py:44-45)
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = dx * cam.c2w[4 * k] + dy * cam.c2w[4 * k + 1] + dz * cam.c2w[4 * k + 2];
    const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    return nrm;
}
