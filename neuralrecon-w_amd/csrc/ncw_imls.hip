// Implicit-moving-least-squares (IMLS) values of an oriented point cloud on a sparse lattice: what turns a cloud with normals
// back into a surface (cloudmesh.py feeds the values to the sparse marching cubes of ncw_mc_sparse.hip).
//
//   ncw_imls_values : f(x) = sum_i w_i n_i.(x - p_i) / sum_i w_i over every point of P within `radius` of the lattice point x
//                     (an all-within-R gather over the 1-NN grid of ncw_nn.hip), w = (1 - d2 / r2)^4, plus the number of
//                     admitted points and the smallest admitted d2.  One wave per block of 4 x 4 x 4 lattice points, one lane
//                     per lattice point.
//
// Rounding contract (include/neuconw_hip.h states it in full; tests/_imls_ref.py restates it in numpy bit for bit).  The file is
// compiled with -ffp-contract=off (build.py): no a * b + c -> fma, every operation below rounds once.
//   float32: x_a = lat_lo_a + float(i_a) * voxel;  dx = P.x - x.x (dy, dz alike);  d2 = dx*dx + dy*dy + dz*dz left to right -- the
//            expression of the 1-NN kernels;  admitted iff d2 <= r2, r2 = radius * radius formed by the entry.
//   float64, over the admitted points in ascending pts_sorted order:  t = 1 - double(d2) * inv_r2, inv_r2 = 1 / double(r2);
//            w = (t * t) * (t * t);  g = -((dx * nx + dy * ny) + dz * nz);  S += w * g;  W += w;  value = float(S / W).
//
// The walk.  A wave takes the cells [c0_a, c1_a] per axis, c0_a = cell_of(xlo_a - pad'), c1_a = cell_of(xhi_a + pad'), where xlo_a /
// xhi_a are the smallest / largest lattice coordinate of its block along a (the lanes' own float32 values) and cell_of is the
// expression ncw_nn_cell_keys assigned every point of P with, clamp included.  Why this is a superset of every point float32
// d2 <= r2 can admit:
//   (1) fl(d2) >= fl(dx*dx): the later terms are >= 0 and rounding is monotone; likewise for the y and z terms.  fl(dx*dx) >=
//       dx^2 (1 - u), u = 2^-24 (r2 is required to be a normal number, so an underflowing dx*dx belongs to |dx| << radius), and
//       dx = (P.x - x.x)(1 + e), |e| <= u.  With r2 <= radius^2 (1 + u): an admitted point has |P.a - x.a| <= radius (1 + 3u) on
//       every axis, in exact arithmetic.
//   (2) pad = radius (1 + 2^-20) + margin, rounded up by the entry; t = fl(xlo_a - pad) is within u |t| of xlo_a - pad, and
//       pad' widens it by a further 2^-22 |t| (itself rounded, error <= u |t|): the float the wave uses is <= xlo_a - radius (1 + 3u)
//       <= P.a for every admitted point of every lane, and symmetrically above.
//   (3) cell_of is monotone non-decreasing in its argument (a subtraction of a constant, a product with inv_h > 0, floor, the cast
//       and the clamp all are): cell_of(lower float) <= cell_of(P.a) <= cell_of(upper float), and cell_of(P.a) IS the cell P was
//       filed under -- for a point outside the grid box too, which the same clamp put into a boundary cell.  No face coordinate is
//       ever compared, so `margin` is only kept in hand.
// Within the box the cells are walked in ascending key order (x slowest), which is ascending pts_sorted order; the points of the
// consecutive cells of one (x, y) row are ONE contiguous run of pts_sorted.  64 rows at a time: lane r finds the run of row r,
// a wave scan lays the runs end to end, and the run points (32 B: position + index, normal) are staged through LDS in tiles of
// 256 -- a flat index is mapped back to (row, offset) by a binary search over the 64 prefix sums.  Every lane applies its own
// d2 <= r2 test to every staged point (an LDS broadcast read), so the order a lane sees is pts_sorted order restricted to its
// admitted set.  No atomics, no transcendental, no square root; a row of the output depends on its block's coordinates only, so
// any order or split of `blocks` into launches gives the same rows.
//
// Sizing: 8 KiB of tiles + 0.5 KiB of row tables per one-wave workgroup: the 160 KiB of LDS of a CU hold 18 such workgroups, 4 to 5
// waves per SIMD, fewer than the 8 the register count (54 VGPRs) would allow -- the inner loop is VALU work on LDS broadcasts, and
// the other waves only have to cover the staging loads and the barriers.  profiles/cloudmesh/README.md has the compiler's
// resource report.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

namespace {

constexpr int kTile = 256;  // staged points per tile: 4 per lane
constexpr int kRows = 64;   // (x, y) cell rows per pass: one per lane

struct Grid {
    float lo[3];
    float h, inv_h;
    int dim[3];
};

struct Lattice {
    float lo[3];
    float voxel;
    int side[3];
};

// ncw_nn.hip's cell_of -- clamp((int)floorf((x - lo) * inv_h), 0, dim - 1) -- with the clamp taken on the float, so that a bound
// that overflowed the int range (or is a NaN: cell 0) is never cast; the same cell for every argument whose cast is defined
__device__ __forceinline__ int cell_of(float x, float lo, float inv_h, int dim) {
    const float f = floorf((x - lo) * inv_h);
    return f >= (float)dim ? dim - 1 : (f > 0.f ? (int)f : 0);
}

__global__ __launch_bounds__(64) void imls_values_kernel(const float4* __restrict__ ps, const float4* __restrict__ ns,
                                                         const int2* __restrict__ range, int m,
                                                         const int32_t* __restrict__ blocks, Grid g, Lattice lat, float pad,
                                                         float r2, double inv_r2, float* __restrict__ value,
                                                         int32_t* __restrict__ count, float* __restrict__ d2min,
                                                         int32_t* __restrict__ work) {
    __shared__ float4 s_p[kTile];
    __shared__ float4 s_n[kTile];
    __shared__ int s_start[kRows];
    __shared__ int s_pre[kRows + 1];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const float inf = __int_as_float(0x7f800000);
    const float qnan = __int_as_float(0x7fc00000);
    const int bi[3] = {blocks[b * 3 + 0], blocks[b * 3 + 1], blocks[b * 3 + 2]};
    const int la[3] = {lane >> 4, (lane >> 2) & 3, lane & 3};
    bool block_in = true, lane_in = true;
    float x[3];
    int c0[3], c1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool in = bi[a] >= 0 && 4 * (int64_t)bi[a] < lat.side[a];  // side <= 16384: 4 * bi + 3 cannot overflow below
        block_in = block_in && in;
        const int i0 = in ? 4 * bi[a] : 0;
        const int il = i0 + la[a];
        lane_in = lane_in && in && il < lat.side[a];
        const int i1 = min(i0 + 3, lat.side[a] - 1);
        x[a] = lat.lo[a] + (float)il * lat.voxel;
        const float xlo = lat.lo[a] + (float)i0 * lat.voxel, xhi = lat.lo[a] + (float)i1 * lat.voxel;
        float t0 = xlo - pad, t1 = xhi + pad;
        t0 = t0 - fabsf(t0) * 0x1p-22f;
        t1 = t1 + fabsf(t1) * 0x1p-22f;
        c0[a] = cell_of(t0, g.lo[a], g.inv_h, g.dim[a]);
        c1[a] = cell_of(t1, g.lo[a], g.inv_h, g.dim[a]);
        if (c1[a] < c0[a]) c1[a] = c0[a];  // a NaN bound (a non-finite lattice): one cell; nothing is admitted there anyway
    }
    const int64_t row_out = b * 64 + lane;
    if (!block_in) {  // wave-uniform: no lattice point of this block exists
        value[row_out] = qnan; count[row_out] = 0; d2min[row_out] = inf;
        if (work && lane == 0) work[b] = 0;
        return;
    }
    const int ny = c1[1] - c0[1] + 1, nz = c1[2] - c0[2] + 1;
    const int nrows = (c1[0] - c0[0] + 1) * ny;  // < 2^30: the cell table has at most 2^30 entries
    const int DY = g.dim[1], DZ = g.dim[2];
    double S = 0.0, W = 0.0;
    int cnt = 0, staged = 0;
    float dmin = inf;
    for (int rb = 0; rb < nrows; rb += kRows) {
        // the run of pts_sorted this lane's row holds: first non-empty cell's start .. last non-empty cell's end
        const int r = rb + lane;
        int start = 0, end = 0;
        if (r < nrows) {
            const int rx = c0[0] + r / ny, ry = c0[1] + r % ny;
            const int2* rg = range + ((int64_t)rx * DY + ry) * DZ + c0[2];
            bool any = false;
            for (int k = 0; k < nz; ++k) {
                const int2 v = rg[k];
                if (v.y > v.x) {
                    if (!any) start = v.x;
                    any = true;
                    end = v.y;
                }
            }
            if (start < 0 || end > m || end < start) { start = 0; end = 0; }  // a table that does not belong to P: read nothing
        }
        int incl = end - start;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        __syncthreads();  // the previous pass has finished with the tables and the tiles
        s_start[lane] = start;
        s_pre[lane + 1] = incl;
        if (lane == 0) s_pre[0] = 0;
        const int total = __shfl(incl, 63, 64);
        staged += total;
        for (int base = 0; base < total; base += kTile) {
            __syncthreads();  // tables written / the previous tile consumed
#pragma unroll
            for (int j = 0; j < kTile / 64; ++j) {
                const int f = base + j * 64 + lane;
                if (f < total) {
                    int lo = 0, hi = kRows;  // the largest row with s_pre[row] <= f: rows of length 0 are stepped over
#pragma unroll
                    for (int s = 0; s < 6; ++s) {
                        const int mid = (lo + hi) >> 1;
                        if (s_pre[mid] <= f) lo = mid; else hi = mid;
                    }
                    const int src = s_start[lo] + (f - s_pre[lo]);
                    s_p[j * 64 + lane] = ps[src];
                    s_n[j * 64 + lane] = ns[src];
                }
            }
            __syncthreads();
            const int n = min(kTile, total - base);
            for (int i = 0; i < n; ++i) {
                const float4 p = s_p[i];
                const float dx = p.x - x[0], dy = p.y - x[1], dz = p.z - x[2];
                const float d2 = dx * dx + dy * dy + dz * dz;
                if (d2 <= r2) {  // false for a NaN; r2 is finite, so false for an infinite d2 too
                    const float4 nn = s_n[i];
                    const double t = 1.0 - (double)d2 * inv_r2;
                    const double w = (t * t) * (t * t);
                    const double gd = -(((double)dx * (double)nn.x + (double)dy * (double)nn.y) + (double)dz * (double)nn.z);
                    S = S + w * gd;
                    W = W + w;
                    ++cnt;
                    dmin = fminf(dmin, d2);
                }
            }
        }
    }
    if (lane_in) {
        value[row_out] = (cnt > 0 && W > 0.0) ? (float)(S / W) : qnan;
        count[row_out] = cnt;
        d2min[row_out] = dmin;
    } else {
        value[row_out] = qnan; count[row_out] = 0; d2min[row_out] = inf;
    }
    if (work && lane == 0) work[b] = staged;
}

bool grid_ok(const NcwNnGrid* g) {
    if (!g || !(g->h > 0.f) || !(g->inv_h > 0.f)) return false;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (g->dim[a] < 1) return false;
        cells *= g->dim[a];
        if (cells > (int64_t)1 << 30) return false;
    }
    return true;
}

}  // namespace

extern "C" int ncw_imls_values(const float* pts_sorted, const float* nrm_sorted, const int32_t* cell_range, int64_t m,
                               const NcwNnGrid* grid, float margin, const int32_t* blocks, int64_t nb, const float* lat_lo,
                               float voxel, const int32_t* side, float radius, float* value, int32_t* count, float* d2min,
                               int32_t* work, void* stream) {
    if (nb <= 0) return 0;
    if (!pts_sorted || !nrm_sorted || !cell_range || !blocks || !lat_lo || !side || !value || !count || !d2min || !grid_ok(grid) ||
        !(voxel > 0.f) || !(radius > 0.f) || !(margin >= 0.f) || m < 1 || m > 0x7fffffffll || nb > 0x7fffffffll / 64)
        return NCW_E_BADARG;
    const float inf = __builtin_inff();
    const float r2 = radius * radius;  // rounded once, here
    if (!(r2 >= 1.17549435e-38f) || !(r2 < inf) || !(voxel < inf) || !(margin < inf)) return NCW_E_BADARG;  // r2 normal and finite
    Lattice lat;
    Grid g;
    for (int a = 0; a < 3; ++a) {
        if (side[a] < 1 || side[a] > 16384) return NCW_E_BADARG;
        lat.lo[a] = lat_lo[a];
        lat.side[a] = side[a];
        g.lo[a] = grid->lo[a];
        g.dim[a] = grid->dim[a];
    }
    lat.voxel = voxel;
    g.h = grid->h;
    g.inv_h = grid->inv_h;
    const double padd = (double)radius * (1.0 + 0x1p-20) + (double)margin;
    float pad = (float)padd;
    if ((double)pad < padd) pad = __builtin_nextafterf(pad, inf);  // rounded up
    hipLaunchKernelGGL(imls_values_kernel, dim3((unsigned)nb), dim3(64), 0, (hipStream_t)stream, (const float4*)pts_sorted,
                       (const float4*)nrm_sorted, (const int2*)cell_range, (int)m, blocks, g, lat, pad, r2, 1.0 / (double)r2, value,
                       count, d2min, work);
    NCW_CHECK_LAUNCH();
    return 0;
}
