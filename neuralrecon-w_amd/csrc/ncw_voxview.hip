// Voxel first-hit views: the point-cloud source of the reprojection filter (utils/reproj_filter.py:110-115, 195-196, 224-225,
// 234-240 over utils/kaolin_renderer.py).  The reference voxelises the source cloud over the evaluation box, ray-traces every
// pixel of every training view to the FIRST occupied voxel (kaolin_renderer.py:110-141 -> generate_voxel.py:311-439 with
// return_pts) and keeps the target points whose voxel some view saw.  Here one launch per view walks one ray per lane, stops at
// the first occupied voxel and sets that voxel's bit in `seen` (same layout as the occupancy); a second kernel reads the bit of
// each target point's voxel.  Nothing per crossing is written, nothing goes through the host.
// kaolin's source is not part of the reference tree: as in ncw_voxel.hip the contract followed is its documented one, pinned to
// the float64 slab oracle (oracle.ray_voxel_nuggets).
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_dda.h"

// One lane per pixel of [p0, p0 + n), row-major.  A wave covers 64 neighbouring pixels of a row: their rays start together and
// mostly end in the same few words of the grid, so the loads of occ / brick coalesce early in the walk and the bit is usually
// set already when a lane arrives.
__global__ void voxel_view_seen_kernel(NcwVoxelView cam, int level, float scale, const uint32_t* __restrict__ occ,
                                       const uint32_t* __restrict__ brick, int64_t p0, int64_t n, uint32_t* seen,
                                       float* __restrict__ depth, int32_t* __restrict__ voxel) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;  // padded lanes of the last workgroup
    const int64_t p = p0 + k;
    const int j = (int)(p / cam.width), i = (int)(p - (int64_t)j * cam.width);
    // kaolin_renderer.py:33-51 (gen_rays): integer pixel coordinates, dir = pose (x, y, 1), normalised
    const float x = ((float)i - cam.cx) / cam.fx, y = ((float)j - cam.cy) / cam.fy;
    float dir[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) dir[a] = cam.pose[3 * a] * x + cam.pose[3 * a + 1] * y + cam.pose[3 * a + 2];
    const float dir_norm = sqrtf(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    const int G = 1 << level;
    const float half = 0.5f * (float)G;
    float u[3], du[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d = dir[a] / dir_norm + 1e-7f;  // generate_voxel.py:332
        u[a] = (cam.o_norm[a] + 1.0f) * half;       // grid coordinates, as ray_voxel_near_far (ncw_dda.h)
        du[a] = d * half;
    }
    float near = 0.f;
    int v = -1;
    dda_walk(u, du, G, occ, brick, [&](float t_in, float, int vox) {  // the first occupied voxel ends the walk
        near = t_in;
        v = vox;
        return true;
    });
    const bool found = v >= 0;
    const bool valid = found && near > 1e-4f;  // generate_voxel.py:397-400
    if (valid) {
        // the grid only gains bits: a stale read of a clear bit costs one redundant atomic, nothing else
        const uint32_t bit = 1u << (v & 31);
        uint32_t* w = seen + (v >> 5);
        if (!(*w & bit)) atomicOr(w, bit);
    }
    if (voxel) voxel[k] = valid ? v : -1;
    if (depth) depth[k] = valid ? near * scale / dir_norm + 0.02f : 0.f;  // kaolin_renderer.py:127, 141
}

// The bit of each point's voxel (voxel_of_point: the index voxel_build_kernel sets).
__global__ void voxel_points_seen_kernel(const float* __restrict__ pts, int64_t n, int level, const uint32_t* __restrict__ seen,
                                         uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int G = 1 << level;
    int c[3];
    uint8_t f = 0;
    if (voxel_of_point(pts + i * 3, G, c)) {
        const int64_t v = ((int64_t)c[0] * G + c[1]) * G + c[2];
        f = (uint8_t)((seen[v >> 5] >> (v & 31)) & 1u);
    }
    flags[i] = f;
}

extern "C" int ncw_voxel_view_seen(const NcwVoxelView* view, const NcwCacheOctree* grid, int64_t p0, int64_t n, uint32_t* seen,
                                   float* depth, int32_t* voxel, void* stream) {
    if (!view || !grid || !grid->occ || !grid->brick || !seen) return NCW_E_BADARG;
    if (grid->level < 3 || grid->level > 10) return NCW_E_BADARG;
    if (view->width <= 0 || view->height <= 0 || p0 < 0 || n < 0 || p0 + n > (int64_t)view->width * view->height)
        return NCW_E_BADARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(voxel_view_seen_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *view,
                       grid->level, grid->scale, grid->occ, grid->brick, p0, n, seen, depth, voxel);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_voxel_points_seen(const float* pts_normalised, int64_t n, int level, const uint32_t* seen, uint8_t* flags,
                                     void* stream) {
    if (!pts_normalised || !seen || !flags || n < 0 || level < 3 || level > 10) return NCW_E_BADARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(voxel_points_seen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       pts_normalised, n, level, seen, flags);
    NCW_CHECK_LAUNCH();
    return 0;
}
