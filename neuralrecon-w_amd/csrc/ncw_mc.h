// Marching cubes: what the dense-lattice kernels (ncw_mesh.hip) and the brick-sparse kernels (ncw_mc_sparse.hip) share.
// Both compile THIS cube, THIS configuration test and THIS edge interpolation, so an edge between the same two grid values gets the
// same `t`, bit for bit, on either path.  The paths differ only in how a cube's eight corners are fetched and in the integer key
// they weld by, which is why edge_vertex returns the edge's two grid points and leaves the key to its caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ncw_mc {

// cube corners: bit0 = +x, bit1 = +y, bit2 = +z
struct Cube {
    float v[8];
    int64_t id[8];  // grid point id (x slowest) in the lattice the caller numbers its points in
    int x, y, z;    // minimum corner, grid-index coordinates
};

struct Vtx {
    float p[3];
    int64_t lo, hi;  // the edge's grid points, lo < hi
    int axis;        // the corner bit in which they differ: 1 = x, 2 = y, 4 = z
};

// zero crossing on the grid edge between cube corners a and b (ordered by grid point id: lo -> hi)
__device__ __forceinline__ Vtx edge_vertex(const Cube& q, int a, int b, float level) {
    if (q.id[a] > q.id[b]) { const int t = a; a = b; b = t; }
    const float va = q.v[a], vb = q.v[b];
    const float t = (level - va) / (vb - va);
    Vtx o;
    const float pa[3] = {(float)(q.x + (a & 1)), (float)(q.y + ((a >> 1) & 1)), (float)(q.z + ((a >> 2) & 1))};
    const float pb[3] = {(float)(q.x + (b & 1)), (float)(q.y + ((b >> 1) & 1)), (float)(q.z + ((b >> 2) & 1))};
#pragma unroll
    for (int i = 0; i < 3; ++i) o.p[i] = pa[i] + t * (pb[i] - pa[i]);
    o.lo = q.id[a];
    o.hi = q.id[b];
    o.axis = a ^ b;
    return o;
}

__device__ __forceinline__ int cube_config(const Cube& q, float level) {
    int cfg = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) cfg |= (q.v[k] < level ? 1 : 0) << k;
    return cfg;
}

}  // namespace ncw_mc
