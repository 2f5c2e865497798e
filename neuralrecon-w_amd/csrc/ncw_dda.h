// The octree walk every ray / sparse-voxel kernel shares (ncw_voxel.hip: near-far and the nugget trace; ncw_cache.hip: the ray-cache
// rows; ncw_voxview.hip: the first-hit views): the 3-D DDA over the bit-packed occupancy of voxel.py (x index slowest, 8^3-voxel
// brick mask for empty-space skipping) and get_near_far's per-ray rule on top of it
// (tools/prepare_data/generate_voxel.py:311-439).
#pragma once
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

// The voxel of a point of the normalised cube: c = its integer coordinates at grid side G ((p + 1) (0.5f G), truncated); false for
// a point outside the cube (or NaN).  ncw_voxel_build and ncw_voxel_points_seen must agree on it to the bit: both call this.
__device__ __forceinline__ bool voxel_of_point(const float* p, int G, int (&c)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float u = (p[a] + 1.0f) * (0.5f * (float)G);
        if (!(u >= 0.f) || u >= (float)G) return false;
        c[a] = (int)u;
    }
    return true;
}

// The 3-D DDA every ray kernel shares: walks the level-`level` voxels a ray crosses inside the cube, in depth order, and calls
// hit(t_entry, t_exit, linear voxel index) for every OCCUPIED one; hit returns true to end the walk there (the first-hit views of
// ncw_voxview.hip), false to go on.  u = origin in grid coordinates, du = direction per unit depth.
template <class F>
__device__ __forceinline__ void dda_walk(const float (&u)[3], const float (&du)[3], int G, const uint32_t* __restrict__ occ,
                                         const uint32_t* __restrict__ brick, F&& hit) {
    const int Gb = G >> 3 > 0 ? G >> 3 : 1;
    // cube entry / exit
    float t0 = -3.0e38f, t1 = 3.0e38f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ta = (0.f - u[a]) / du[a], tb = ((float)G - u[a]) / du[a];
        t0 = fmaxf(t0, fminf(ta, tb));
        t1 = fminf(t1, fmaxf(ta, tb));
    }
    if (!(t1 >= fmaxf(t0, 0.f))) return;
    float t_entry = fmaxf(t0, 0.f);
    // The exit depth of the current voxel along axis a is computed FROM THE VOXEL INDEX at every step, (boundary - u) / du, not by
    // accumulating tmax += 1 / |du|: at level 10 a ray crosses up to 3072 voxels and the accumulated rounding (up to ~0.1 voxel at the
    // far side of the cube) let the walk visit voxels the ray does not touch (tests/test_gpu_voxel.py, level 10).
    int idx[3], step[3];
    float tmax[3], inv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pos = u[a] + du[a] * t_entry;
        int i = (int)floorf(pos);
        // a ray entering through a face sits exactly on the boundary: step into the cube
        if (du[a] > 0.f) i = min(max(i, 0), G - 1);
        else i = min(max((int)ceilf(pos) - 1, 0), G - 1);
        idx[a] = i;
        step[a] = du[a] > 0.f ? 1 : -1;
        inv[a] = 1.0f / du[a];
        tmax[a] = ((float)(i + (du[a] > 0.f ? 1 : 0)) - u[a]) * inv[a];
    }
    int cur_brick = -1;
    bool brick_on = false;
    for (int it = 0; it < 3 * G + 3; ++it) {
        int ax = 0;
        if (tmax[1] < tmax[ax]) ax = 1;
        if (tmax[2] < tmax[ax]) ax = 2;
        const int b = ((idx[0] >> 3) * Gb + (idx[1] >> 3)) * Gb + (idx[2] >> 3);
        if (b != cur_brick) {
            cur_brick = b;
            brick_on = (brick[b >> 5] >> (b & 31)) & 1u;
        }
        if (brick_on) {
            const int64_t v = ((int64_t)idx[0] * G + idx[1]) * G + idx[2];
            if (((occ[v >> 5] >> (v & 31)) & 1u) && hit(t_entry, tmax[ax], (int)v)) break;  // v < 2^30 at level 10
        }
        // advance to the next voxel along the ray
        t_entry = tmax[ax];
        if (ax == 0) { idx[0] += step[0]; tmax[0] = ((float)(idx[0] + (step[0] > 0 ? 1 : 0)) - u[0]) * inv[0]; }
        else if (ax == 1) { idx[1] += step[1]; tmax[1] = ((float)(idx[1] + (step[1] > 0 ? 1 : 0)) - u[1]) * inv[1]; }
        else { idx[2] += step[2]; tmax[2] = ((float)(idx[2] + (step[2] > 0 ? 1 : 0)) - u[2]) * inv[2]; }
        if (idx[0] < 0 || idx[0] >= G || idx[1] < 0 || idx[1] >= G || idx[2] < 0 || idx[2] >= G) break;
    }
}

// get_near_far for ONE ray (o, d in SfM space; the cube is t.origin +- t.scale): entry depth of the first and of the last occupied
// voxel in SfM units, 0 / 0 where the ray misses.
__device__ __forceinline__ void ray_voxel_near_far(const float (&ro)[3], const float (&rd)[3], const NcwCacheOctree& t,
                                                   float& near_out, float& far_out) {
    const int G = 1 << t.level;
    const float half = 0.5f * (float)G;
    const float scale = t.scale;
    float u[3], du[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d = rd[a] + 1e-7f;            // generate_voxel.py:332
        const float o = (ro[a] + 1e-7f - t.origin[a]) / scale;  // :333, :345
        u[a] = (o + 1.0f) * half;   // grid coordinates
        du[a] = d * half;           // per unit of depth (depth is along the un-normalised direction)
    }
    float near = 0.f, far = 0.f;
    bool found = false;
    dda_walk(u, du, G, t.occ, t.brick, [&](float t_in, float, int) {
        if (!found) { near = t_in; found = true; }
        far = t_in;
        return false;
    });
    const bool valid = found && near > 1e-4f;  // generate_voxel.py:397
    near_out = valid ? near * scale : 0.f;  // :436-439
    far_out = valid ? far * scale : 0.f;
}
