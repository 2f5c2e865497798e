// Ray / sparse-voxel near-far (config 3, voxel-guided sampling): native replacement of kaolin's
// `spc_render.unbatched_raytrace(..., return_depth=True, with_exit=False)` as used by
// tools/prepare_data/generate_voxel.py:311-439 (get_near_far) and rendering/renderer.py:380-456.
//
// Occupancy is a bit-packed dense grid of side G = 2^level over the normalised cube [-1,1]^3 (x index
// slowest, like kaolin's points[:,0]) plus a brick mask (8^3 voxels per brick) for empty-space
// skipping.  One thread per ray: 3-D DDA; per ray we need the ENTRY depth of the first and of the last
// occupied voxel (with_exit=False: "far" is the entry of the last voxel, generate_voxel.py:370-372).
// kaolin's source is not part of the reference tree (unpinned fork): this follows the documented
// contract and is validated geometrically against a brute-force slab test (oracle.ray_voxel_near_far).
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_dda.h"

__global__ void voxel_build_kernel(const float* __restrict__ pts, int64_t n, int level, uint32_t* __restrict__ occ,
                                   uint32_t* __restrict__ brick) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int G = 1 << level;
    int c[3];
    if (!voxel_of_point(pts + i * 3, G, c)) return;
    const int64_t v = ((int64_t)c[0] * G + c[1]) * G + c[2];
    atomicOr(&occ[v >> 5], 1u << (v & 31));
    const int Gb = G >> 3 > 0 ? G >> 3 : 1;
    const int64_t b = ((int64_t)(c[0] >> 3) * Gb + (c[1] >> 3)) * Gb + (c[2] >> 3);
    atomicOr(&brick[b >> 5], 1u << (b & 31));
}

__global__ void ray_voxel_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int R, NcwCacheOctree tree,
                                 float* __restrict__ near_out, float* __restrict__ far_out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const float ro[3] = {rays_o[r * 3], rays_o[r * 3 + 1], rays_o[r * 3 + 2]};
    const float rd[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
    ray_voxel_near_far(ro, rd, tree, near_out[r], far_out[r]);
}

// kaolin.render.spc.unbatched_raytrace's contract (generate_voxel.py:358-368 is its one call site): EVERY (ray, occupied voxel)
// intersection -- a "nugget" -- ordered by ray, then by depth.  Two passes of the same walk: offsets == NULL counts the
// nuggets of each ray, otherwise ray r writes its nuggets from offsets[r] on.  Origins are already normalised to the cube
// [-1, 1]^3 and nothing is added to them (the caller's get_near_far does that, :332-345).
__global__ void ray_voxel_trace_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int R, int level,
                                       const uint32_t* __restrict__ occ, const uint32_t* __restrict__ brick,
                                       const int32_t* __restrict__ offsets, int32_t* __restrict__ counts,
                                       int32_t* __restrict__ nug_ray, int32_t* __restrict__ nug_voxel,
                                       float* __restrict__ nug_depth) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int G = 1 << level;
    const float half = 0.5f * (float)G;
    float u[3], du[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        u[a] = (rays_o[r * 3 + a] + 1.0f) * half;
        du[a] = rays_d[r * 3 + a] * half;
    }
    if (!offsets) {
        int n = 0;
        dda_walk(u, du, G, occ, brick, [&](float, float, int) { ++n; return false; });
        counts[r] = n;
    } else {
        int64_t at = offsets[r];
        dda_walk(u, du, G, occ, brick, [&](float t_in, float t_out, int v) {
            nug_ray[at] = r;
            nug_voxel[at] = v;
            nug_depth[2 * at] = t_in;
            nug_depth[2 * at + 1] = t_out;
            ++at;
            return false;
        });
    }
}

extern "C" int ncw_voxel_build(const float* pts_normalised, int64_t n, int level, uint32_t* occ, uint32_t* brick,
                               void* stream) {
    if (n <= 0) return 0;
    if (level < 3 || level > 10) return NCW_E_BADARG;
    hipLaunchKernelGGL(voxel_build_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       pts_normalised, n, level, occ, brick);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_ray_voxel_near_far(const float* rays_o_sfm, const float* rays_d, int R, const float* scene_origin_host,
                                      float scale, int level, const uint32_t* occ, const uint32_t* brick, float* near_sfm,
                                      float* far_sfm, void* stream) {
    if (R <= 0) return 0;
    if (level < 3 || level > 10 || !scene_origin_host) return NCW_E_BADARG;
    const NcwCacheOctree tree = {{scene_origin_host[0], scene_origin_host[1], scene_origin_host[2]}, scale, level, 0, occ, brick};
    hipLaunchKernelGGL(ray_voxel_kernel, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream, rays_o_sfm, rays_d, R, tree,
                       near_sfm, far_sfm);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_ray_voxel_trace(const float* rays_o_norm, const float* rays_d, int R, int level, const uint32_t* occ,
                                   const uint32_t* brick, const int32_t* offsets, int32_t* counts, int32_t* nug_ray,
                                   int32_t* nug_voxel, float* nug_depth, void* stream) {
    if (R <= 0) return 0;
    if (level < 3 || level > 10 || !rays_o_norm || !rays_d || !occ || !brick) return NCW_E_BADARG;
    if (offsets ? (!nug_ray || !nug_voxel || !nug_depth) : !counts) return NCW_E_BADARG;
    hipLaunchKernelGGL(ray_voxel_trace_kernel, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream, rays_o_norm, rays_d, R,
                       level, occ, brick, offsets, counts, nug_ray, nug_voxel, nug_depth);
    NCW_CHECK_LAUNCH();
    return 0;
}
