// The per-pixel arithmetic of a training row that ncw_cache.hip (the cached rows) and ncw_source.hip (the rows rebuilt per
// batch) must agree on to the bit: both call these, neither restates them.
#pragma once
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_dda.h"
#include "ncw_raymath.h"

// origin and normalised direction of pixel (row, col): datasets/ray_utils.py:44-45 on top of view_ray_dir
__device__ __forceinline__ void row_ray(const NcwViewCamera& cam, int row, int col, float (&o)[3], float (&dn)[3]) {
    float d[3];
    const float nrm = view_ray_dir(cam, row, col, d);
    o[0] = cam.c2w[3]; o[1] = cam.c2w[7]; o[2] = cam.c2w[11];
    dn[0] = d[0] / nrm; dn[1] = d[1] / nrm; dn[2] = d[2] / nrm;
}

// near / far of a KEPT ray from the range octree (phototourism.py:638-657)
__device__ __forceinline__ void row_range_near_far(const float (&o)[3], const float (&dn)[3], const NcwCacheOctree& range,
                                                   float voxel_size, float& near, float& far) {
    float rn, rf;
    ray_voxel_near_far(o, dn, range, rn, rf);
    near = rn;                                // 0 / 0 where the range octree misses (:653-654)
    far = rn > 0.f ? rf + voxel_size : rf;    // :305-308
}

// torchvision ToTensor: value / 255
__device__ __forceinline__ float row_rgb(uint8_t v) { return (float)v / 255.f; }
