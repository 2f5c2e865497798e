// Marching cubes straight on the brick-blocked sparse SDF values of `gen_grid_spc` (mesh.isosurface_sparse): no array of the
// size of the [dim]^3 lattice is ever made.  The occupied coarse voxels ("bricks", n of them, lexicographically ascending in a
// [G]^3 lattice) carry up^3 values each, brick-major, then local x, y, z with z fastest: K = n * up^3 values in all.
//
//   ncw_mcs_neighbors: nbr [n,7] int32.  One lane per (brick, offset o = 1..7; bit0 = +x, bit1 = +y, bit2 = +z, the corner
//                      bits of a cube): binary search of the brick at that offset among the bricks behind this one (the list is
//                      ascending), -1 where it is absent or outside the lattice.
//   ncw_mcs_count    : one lane per sub-voxel = per cube with that sub-voxel as its minimum corner.  A corner that leaves the
//                      brick across an upper face is read from the neighbour's block through the table (direct gathers: the
//                      seven other corners of most lanes are in lines their neighbours in the wave read too); a missing
//                      neighbour means no cube.  counts [K] uint8 triangles (0..5).
//   ncw_mcs_cube_ids : ids [M] int64 = the global grid point id (x slowest, side G * up) of the minimum corner of the M
//                      non-empty cubes the caller compacted out of counts.  The caller sorts by it: that is the dense path's
//                      cube order, so the faces come out in the dense path's order.
//   ncw_mcs_emit     : one lane per non-empty cube, in that order.  Same cube, same configuration test and same edge
//                      interpolation as ncw_mc_emit (ncw_mc.h); the weld key is lo_point * 3 + (0 for the z edge, 1 for y, 2 for x),
//                      which sorts exactly as the dense key lo_point * n_points + hi_point does and stays below 2^44.
// No atomics: every output element is written by one lane, so the result is bitwise reproducible.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_mc.h"

namespace {

using namespace ncw_mc;

struct Grid {
    const int32_t* bricks;  // [n,3]
    const int32_t* nbr;     // [n,7]
    int64_t n;
    int lg;                 // log2(up)
    int D;                  // G * up: side of the fine lattice
};

// the cube whose minimum corner is sub-voxel i (< K); false where one of its corners was not evaluated
__device__ __forceinline__ bool load_cube(const float* __restrict__ values, const Grid& g, int64_t i, Cube& q) {
    const int lg = g.lg, m = (1 << lg) - 1;
    const int64_t b = i >> (3 * lg);
    const int r = (int)(i & ((1 << (3 * lg)) - 1));
    const int lx = r >> (2 * lg), ly = (r >> lg) & m, lz = r & m;
    const int cross = (lx == m ? 1 : 0) | (ly == m ? 2 : 0) | (lz == m ? 4 : 0);  // axes on which the upper corners leave the brick
    int64_t base[8];  // first value of the brick that holds corner k
    base[0] = b << (3 * lg);
#pragma unroll
    for (int o = 1; o < 8; ++o) {
        base[o] = base[0];
        if ((o & cross) == o) {  // asked for only where every axis of o is crossed
            const int nb = g.nbr[b * 7 + (o - 1)];
            if (nb < 0 || nb >= g.n) return false;  // absent (an index past the list is never followed)
            base[o] = (int64_t)nb << (3 * lg);
        }
    }
    q.x = (g.bricks[3 * b] << lg) + lx;
    q.y = (g.bricks[3 * b + 1] << lg) + ly;
    q.z = (g.bricks[3 * b + 2] << lg) + lz;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cx = (k & 1) ? ((lx + 1) & m) : lx, cy = (k & 2) ? ((ly + 1) & m) : ly, cz = (k & 4) ? ((lz + 1) & m) : lz;
        q.v[k] = values[base[k & cross] + ((((cx << lg) | cy) << lg) | cz)];
        q.id[k] = ((int64_t)(q.x + (k & 1)) * g.D + (q.y + ((k >> 1) & 1))) * g.D + (q.z + ((k >> 2) & 1));
    }
    return true;
}

__global__ __launch_bounds__(256) void mcs_neighbors_kernel(const int32_t* __restrict__ bricks, int64_t n, int G,
                                                            int32_t* __restrict__ nbr) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * 7) return;
    const int64_t b = t / 7;
    const int o = (int)(t - b * 7) + 1;
    const int x = bricks[3 * b] + (o & 1), y = bricks[3 * b + 1] + ((o >> 1) & 1), z = bricks[3 * b + 2] + ((o >> 2) & 1);
    int32_t found = -1;
    if (x < G && y < G && z < G) {
        int64_t lo = b + 1, hi = n;  // the target is lexicographically above brick b
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const int mx = bricks[3 * mid], my = bricks[3 * mid + 1], mz = bricks[3 * mid + 2];
            const bool less = mx != x ? mx < x : (my != y ? my < y : mz < z);
            if (less) lo = mid + 1; else hi = mid;
        }
        if (lo < n && bricks[3 * lo] == x && bricks[3 * lo + 1] == y && bricks[3 * lo + 2] == z) found = (int32_t)lo;
    }
    nbr[t] = found;
}

__global__ __launch_bounds__(256) void mcs_count_kernel(const float* __restrict__ values, Grid g, int64_t K, float level,
                                                        const int32_t* __restrict__ ntri, uint8_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    Cube q;
    counts[i] = load_cube(values, g, i, q) ? (uint8_t)ntri[cube_config(q, level)] : (uint8_t)0;
}

__global__ __launch_bounds__(256) void mcs_cube_ids_kernel(const int32_t* __restrict__ bricks, int lg, int D, int64_t K,
                                                           const int64_t* __restrict__ sub, int64_t M,
                                                           int64_t* __restrict__ ids) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    int64_t i = sub[j];
    i = i < 0 ? 0 : (i >= K ? K - 1 : i);  // the caller's indices come from counts [K]; nothing else is ever read
    const int m = (1 << lg) - 1;
    const int64_t b = i >> (3 * lg);
    const int r = (int)(i & ((1 << (3 * lg)) - 1));
    const int x = (bricks[3 * b] << lg) + (r >> (2 * lg)), y = (bricks[3 * b + 1] << lg) + ((r >> lg) & m),
              z = (bricks[3 * b + 2] << lg) + (r & m);
    ids[j] = ((int64_t)x * D + y) * D + z;
}

__global__ __launch_bounds__(256) void mcs_emit_kernel(const float* __restrict__ values, Grid g, int64_t K, float level,
                                                       const int8_t* __restrict__ tri, const int32_t* __restrict__ ntri,
                                                       const int32_t* __restrict__ edges, const int64_t* __restrict__ sub,
                                                       const int64_t* __restrict__ offsets, int64_t M, int64_t T,
                                                       float* __restrict__ pos, int64_t* __restrict__ key) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int64_t i = sub[j];
    if (i < 0 || i >= K) return;
    Cube q;
    if (!load_cube(values, g, i, q)) return;
    const int cfg = cube_config(q, level);
    const int n = ntri[cfg];
    int64_t out = offsets[j];
    if (out < 0 || out + n > T) return;  // offsets that are not the scan of these counts: write nothing out of range
    for (int t = 0; t < n; ++t, ++out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {  // the table's winding: normal towards increasing values
            const int e = tri[cfg * 16 + 3 * t + c];
            const Vtx v = edge_vertex(q, edges[2 * e], edges[2 * e + 1], level);
            key[out * 3 + c] = v.lo * 3 + (v.axis == 1 ? 2 : (v.axis == 2 ? 1 : 0));
#pragma unroll
            for (int d = 0; d < 3; ++d) pos[(out * 3 + c) * 3 + d] = v.p[d];
        }
    }
}

// log2(up) for up = 1, 2, 4, 8, 16, 32; -1 for anything else
int log2_up(int up) {
    for (int lg = 0; lg <= 5; ++lg)
        if (up == (1 << lg)) return lg;
    return -1;
}

// K = n * up^3, or -1 for a shape every entry point refuses
int64_t shape_K(int64_t n, int up, int G) {
    const int lg = log2_up(up);
    if (lg < 0 || n < 0 || G < 1 || (int64_t)G * up > 16384) return -1;
    if (n > (INT64_C(0x7fffffff) >> (3 * lg))) return -1;  // K > 2^31 - 1
    return n << (3 * lg);
}

unsigned blocks(int64_t lanes) { return (unsigned)((lanes + 255) / 256); }

}  // namespace

extern "C" int ncw_mcs_neighbors(const int32_t* bricks, int64_t n, int G, int32_t* nbr, void* stream) {
    if (n < 0 || n > 0x7fffffff || G < 1 || G > 16384) return NCW_E_BADARG;
    if (n == 0) return 0;
    if (!bricks || !nbr) return NCW_E_BADARG;
    hipLaunchKernelGGL(mcs_neighbors_kernel, dim3(blocks(n * 7)), dim3(256), 0, (hipStream_t)stream, bricks, n, G, nbr);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mcs_count(const float* values, int64_t n_values, const int32_t* bricks, const int32_t* nbr, int64_t n, int up,
                             int G, float level, const int32_t* ntri, uint8_t* counts, void* stream) {
    const int64_t K = shape_K(n, up, G);
    if (K < 0 || n_values != K) return NCW_E_BADARG;
    if (K == 0) return 0;
    if (!values || !bricks || !nbr || !ntri || !counts) return NCW_E_BADARG;
    const Grid g = {bricks, nbr, n, log2_up(up), G * up};
    hipLaunchKernelGGL(mcs_count_kernel, dim3(blocks(K)), dim3(256), 0, (hipStream_t)stream, values, g, K, level, ntri, counts);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mcs_cube_ids(const int32_t* bricks, int64_t n, int up, int G, const int64_t* sub, int64_t M, int64_t* ids,
                                void* stream) {
    const int64_t K = shape_K(n, up, G);
    if (K < 0 || M < 0 || M > K) return NCW_E_BADARG;
    if (M == 0) return 0;
    if (!bricks || !sub || !ids) return NCW_E_BADARG;
    hipLaunchKernelGGL(mcs_cube_ids_kernel, dim3(blocks(M)), dim3(256), 0, (hipStream_t)stream, bricks, log2_up(up), G * up, K, sub,
                       M, ids);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mcs_emit(const float* values, int64_t n_values, const int32_t* bricks, const int32_t* nbr, int64_t n, int up,
                            int G, float level, const int8_t* tri, const int32_t* ntri, const int32_t* edges, const int64_t* sub,
                            const int64_t* offsets, int64_t M, int64_t T, float* tri_pos, int64_t* tri_key, void* stream) {
    const int64_t K = shape_K(n, up, G);
    if (K < 0 || n_values != K || M < 0 || M > K || T < 0 || T > 5 * M) return NCW_E_BADARG;
    if (M == 0) return 0;
    if (!values || !bricks || !nbr || !tri || !ntri || !edges || !sub || !offsets || !tri_pos || !tri_key) return NCW_E_BADARG;
    const Grid g = {bricks, nbr, n, log2_up(up), G * up};
    hipLaunchKernelGGL(mcs_emit_kernel, dim3(blocks(M)), dim3(256), 0, (hipStream_t)stream, values, g, K, level, tri, ntri, edges,
                       sub, offsets, M, T, tri_pos, tri_key);
    NCW_CHECK_LAUNCH();
    return 0;
}
