// Exact point-to-triangle-mesh distances on the GPU (mesh evaluation): the recall side measured to the
// predicted SURFACE instead of to K |GT| samples of it.  The design of ncw_nn.hip carried from points to triangles:
//
//   ncw_ptm_pack      : gather verts / faces into tri[F][9] (recentred, float64) and valid[F];
//   ncw_ptm_count     : cells of every triangle's axis-aligned box (clamped into the grid, as ncw_nn clamps points); a
//                       triangle over more than max_cells_per_tri cells stays out of the grid and goes to the large list;
//   (caller)          : inclusive prefix sum of the counts -- plumbing (torch.cumsum);
//   ncw_ptm_emit      : (cell key, triangle id) pairs;
//   (caller)          : stable sort of the pairs by key -- plumbing (torch.sort);
//   ncw_ptm_ranges    : [start, end) of every non-empty cell in a dense table, ids in cell order;
//   ncw_ptm_cell_keys : cell key of every query;
//   ncw_ptm_query     : one lane per query (queries visited in cell order): the large list first, staged through LDS per
//                       workgroup (as the large-triangle list of ncw_raster.hip), then Chebyshev shells r = 0, 1, 2, ..
//                       around the query's cell, best (d^2, index) kept; after shell r the search stops once
//                       best d^2 < (b - margin)^2, b = distance from the query to the faces of the (2r+1)^3 block that are
//                       not on the grid boundary, or once the block covers the grid.  EXACT: an unvisited triangle's box does
//                       not overlap the block, so the whole triangle lies beyond one face plane of the block; clamped
//                       triangles lie beyond a boundary face, and boundary faces never enter b.  A triangle met in several
//                       cells is evaluated again (min is idempotent).  Queries open after max_shell shells escape;
//   ncw_ptm_brute     : the escaped queries against all valid triangles (LDS tiles, triangles split over blocks); the
//                       per-query minimum without order dependence: a 64-bit atomicMin of the bits of d^2, then an atomicMin
//                       of the index among the triangles at that minimum, then a finish pass.
//
// The distance contract (face term, three segment terms with canonically ordered endpoints, first minimal term, ties to
// the smaller triangle index) is stated in include/neuconw_hip.h and restated in numpy by tests/_ptm_ref.py.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

// products and sums are rounded one by one (no fused multiply-add): d^2 of a (query, triangle) pair is then the same bits
// in the query kernel, in both brute passes and in the finish pass, whatever the compiler would choose to contract, and
// the numpy restatement is the same arithmetic
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kLargeTile = 64;   // triangles per LDS tile of the large list
constexpr int kBruteTile = 128;  // triangles per LDS tile of the escape kernel
constexpr int kNone = 0x7fffffff;

struct Grid {
    double lo[3];
    double h, inv_h;
    int dim[3];
};

struct Box {
    int on;
    double lo[3], hi[3];
};

__device__ __forceinline__ double inf64() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ int cell_of(double x, double lo, double inv_h, int dim) {
    const double c = floor((x - lo) * inv_h);
    return c >= (double)dim ? dim - 1 : (c > 0.0 ? (int)c : 0);  // NaN: cell 0
}

__device__ __forceinline__ bool in_box(const Box& b, double x, double y, double z) {
    return x >= b.lo[0] && x <= b.hi[0] && y >= b.lo[1] && y <= b.hi[1] && z >= b.lo[2] && z <= b.hi[2];  // NaN: outside
}

__device__ __forceinline__ bool better(double d2, int i, double bd2, int bi) { return d2 < bd2 || (d2 == bd2 && i < bi); }

// one segment term: endpoints in canonical (lexicographic) order, exact endpoints at s <= 0 / s >= 1
template <bool CP>
__device__ __forceinline__ void seg_term(double px, double py, double pz, double ax, double ay, double az, double bx, double by,
                                         double bz, double& d2m, double& mx, double& my, double& mz) {
    const bool sw = bx < ax || (bx == ax && (by < ay || (by == ay && bz < az)));
    const double ux = sw ? bx : ax, uy = sw ? by : ay, uz = sw ? bz : az;
    const double vx = sw ? ax : bx, vy = sw ? ay : by, vz = sw ? az : bz;
    const double wx = vx - ux, wy = vy - uy, wz = vz - uz;
    const double l = wx * wx + wy * wy + wz * wz;
    double s = 0.0;
    if (l > 0.0) {
        s = ((px - ux) * wx + (py - uy) * wy + (pz - uz) * wz) / l;
        s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    }
    double cx, cy, cz;
    if (s <= 0.0) { cx = ux; cy = uy; cz = uz; }
    else if (s >= 1.0) { cx = vx; cy = vy; cz = vz; }
    else { cx = ux + s * wx; cy = uy + s * wy; cz = uz + s * wz; }
    const double dx = px - cx, dy = py - cy, dz = pz - cz;
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < d2m) {
        d2m = d2;
        if (CP) { mx = cx; my = cy; mz = cz; }
    }
}

// d^2 of query P to triangle t[9] = (A, B, C), +inf when no term answers; with CP the closest point of the first minimal term
template <bool CP>
__device__ __forceinline__ double tri_dist(double px, double py, double pz, const double* t, double& mx, double& my, double& mz) {
    const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
    double d2m = inf64();
    if (CP) { mx = nan64(); my = nan64(); mz = nan64(); }
    const double e1x = bx - ax, e1y = by - ay, e1z = bz - az;
    const double e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double nn = nx * nx + ny * ny + nz * nz;
    if (nn > 0.0 && nn < inf64()) {
        const double pax = px - ax, pay = py - ay, paz = pz - az;
        const double pbx = px - bx, pby = py - by, pbz = pz - bz;
        const double pcx = px - cx, pcy = py - cy, pcz = pz - cz;
        const double e3x = cx - bx, e3y = cy - by, e3z = cz - bz;  // C - B
        const double e4x = ax - cx, e4y = ay - cy, e4z = az - cz;  // A - C
        const double f1 = (e1y * paz - e1z * pay) * nx + (e1z * pax - e1x * paz) * ny + (e1x * pay - e1y * pax) * nz;
        const double f2 = (e3y * pbz - e3z * pby) * nx + (e3z * pbx - e3x * pbz) * ny + (e3x * pby - e3y * pbx) * nz;
        const double f3 = (e4y * pcz - e4z * pcy) * nx + (e4z * pcx - e4x * pcz) * ny + (e4x * pcy - e4y * pcx) * nz;
        if (f1 >= 0.0 && f2 >= 0.0 && f3 >= 0.0) {
            const double tt = nx * pax + ny * pay + nz * paz;
            const double d2 = tt * tt / nn;
            if (d2 < d2m) {
                d2m = d2;
                if (CP) {
                    const double k = tt / nn;
                    mx = px - k * nx; my = py - k * ny; mz = pz - k * nz;
                }
            }
        }
    }
    seg_term<CP>(px, py, pz, ax, ay, az, bx, by, bz, d2m, mx, my, mz);
    seg_term<CP>(px, py, pz, bx, by, bz, cx, cy, cz, d2m, mx, my, mz);
    seg_term<CP>(px, py, pz, cx, cy, cz, ax, ay, az, d2m, mx, my, mz);
    return d2m;
}

__device__ __forceinline__ double tri_d2(double px, double py, double pz, const double* t) {
    double x, y, z;
    return tri_dist<false>(px, py, pz, t, x, y, z);
}

__global__ __launch_bounds__(kBlock) void ptm_pack_kernel(const double* __restrict__ verts, int64_t n_verts,
                                                           const int32_t* __restrict__ faces, int64_t n_faces, double c0, double c1,
                                                           double c2, Box box, double* __restrict__ tri, uint8_t* __restrict__ valid) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    const int64_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    double t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = 0.0;
    bool ok = false;
    if (a >= 0 && a < n_verts && b >= 0 && b < n_verts && c >= 0 && c < n_verts) {
        const double ax = verts[a * 3 + 0], ay = verts[a * 3 + 1], az = verts[a * 3 + 2];
        const double bx = verts[b * 3 + 0], by = verts[b * 3 + 1], bz = verts[b * 3 + 2];
        const double cx = verts[c * 3 + 0], cy = verts[c * 3 + 1], cz = verts[c * 3 + 2];
        ok = isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(bx) && isfinite(by) && isfinite(bz) && isfinite(cx) &&
             isfinite(cy) && isfinite(cz);
        if (box.on) ok = ok && in_box(box, ax, ay, az) && in_box(box, bx, by, bz) && in_box(box, cx, cy, cz);
        if (ok) {
            t[0] = ax - c0; t[1] = ay - c1; t[2] = az - c2;
            t[3] = bx - c0; t[4] = by - c1; t[5] = bz - c2;
            t[6] = cx - c0; t[7] = cy - c1; t[8] = cz - c2;
#pragma unroll
            for (int k = 0; k < 9; ++k) ok = ok && isfinite(t[k]);
            if (!ok) {
#pragma unroll
                for (int k = 0; k < 9; ++k) t[k] = 0.0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) tri[f * 9 + k] = t[k];
    valid[f] = ok ? 1 : 0;
}

// clamped cell range [c0, c1] per axis of the triangle's box
__device__ __forceinline__ void tri_cells(const double* __restrict__ t, const Grid& g, int& x0, int& x1, int& y0, int& y1, int& z0,
                                          int& z1) {
    x0 = cell_of(fmin(t[0], fmin(t[3], t[6])), g.lo[0], g.inv_h, g.dim[0]);
    x1 = cell_of(fmax(t[0], fmax(t[3], t[6])), g.lo[0], g.inv_h, g.dim[0]);
    y0 = cell_of(fmin(t[1], fmin(t[4], t[7])), g.lo[1], g.inv_h, g.dim[1]);
    y1 = cell_of(fmax(t[1], fmax(t[4], t[7])), g.lo[1], g.inv_h, g.dim[1]);
    z0 = cell_of(fmin(t[2], fmin(t[5], t[8])), g.lo[2], g.inv_h, g.dim[2]);
    z1 = cell_of(fmax(t[2], fmax(t[5], t[8])), g.lo[2], g.inv_h, g.dim[2]);
}

__global__ __launch_bounds__(kBlock) void ptm_count_kernel(const double* __restrict__ tri, const uint8_t* __restrict__ valid,
                                                            int64_t n_faces, Grid g, int64_t max_cells, int32_t* __restrict__ count,
                                                            uint8_t* __restrict__ large) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    int32_t cnt = 0;
    uint8_t lg = 0;
    if (valid[f]) {
        int x0, x1, y0, y1, z0, z1;
        tri_cells(tri + f * 9, g, x0, x1, y0, y1, z0, z1);
        const int64_t n = (int64_t)(x1 - x0 + 1) * (y1 - y0 + 1) * (z1 - z0 + 1);  // >= 1, <= cells of the grid <= 2^30
        if (n > max_cells) lg = 1; else cnt = (int32_t)n;
    }
    count[f] = cnt;
    large[f] = lg;
}

__global__ __launch_bounds__(kBlock) void ptm_emit_kernel(const double* __restrict__ tri, const int32_t* __restrict__ count,
                                                           const int64_t* __restrict__ cum, int64_t n_faces, Grid g, int64_t n_pairs,
                                                           int32_t* __restrict__ keys, int32_t* __restrict__ ids) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    const int64_t cnt = count[f];
    if (cnt <= 0) return;
    const int64_t end = cum[f];
    int64_t p = end - cnt;
    if (p < 0 || end > n_pairs) return;  // a table that does not belong to these counts: write nothing
    int x0, x1, y0, y1, z0, z1;
    tri_cells(tri + f * 9, g, x0, x1, y0, y1, z0, z1);
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy)
            for (int iz = z0; iz <= z1; ++iz) {
                if (p >= end) return;  // never more than the count pass promised
                keys[p] = (ix * g.dim[1] + iy) * g.dim[2] + iz;
                ids[p] = (int32_t)f;
                ++p;
            }
}

__global__ __launch_bounds__(kBlock) void ptm_ranges_kernel(const int32_t* __restrict__ skeys, const int64_t* __restrict__ order,
                                                             const int32_t* __restrict__ ids, int64_t m, int64_t n_cells,
                                                             int2* __restrict__ range, int32_t* __restrict__ sorted_ids) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int32_t k = skeys[i];
    if (k >= 0 && k < n_cells) {
        if (i == 0 || skeys[i - 1] != k) range[k].x = (int)i;
        if (i == m - 1 || skeys[i + 1] != k) range[k].y = (int)(i + 1);
    }
    const int64_t j = order[i];
    sorted_ids[i] = (j >= 0 && j < m) ? ids[j] : -1;
}

__global__ __launch_bounds__(kBlock) void ptm_cell_keys_kernel(const double* __restrict__ q, int64_t n, Grid g,
                                                                int32_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int cx = cell_of(q[i * 3 + 0], g.lo[0], g.inv_h, g.dim[0]);
    const int cy = cell_of(q[i * 3 + 1], g.lo[1], g.inv_h, g.dim[1]);
    const int cz = cell_of(q[i * 3 + 2], g.lo[2], g.inv_h, g.dim[2]);
    keys[i] = (cx * g.dim[1] + cy) * g.dim[2] + cz;
}

__device__ __forceinline__ void scan_cell(const int2* __restrict__ range, const int32_t* __restrict__ sids,
                                          const double* __restrict__ tri, int n_faces, int key, double qx, double qy, double qz,
                                          double& bd2, int& bi) {
    const int2 r = range[key];
    for (int p = r.x; p < r.y; ++p) {
        const int id = sids[p];
        if ((unsigned)id >= (unsigned)n_faces) continue;
        const double d2 = tri_d2(qx, qy, qz, tri + (int64_t)id * 9);
        if (better(d2, id, bd2, bi)) { bd2 = d2; bi = id; }
    }
}

// outputs of one answered query at its original position j
__device__ __forceinline__ void write_out(const double* __restrict__ tri, int64_t j, double qx, double qy, double qz, double bd2,
                                          int bi, double* __restrict__ dist, int64_t* __restrict__ idx,
                                          double* __restrict__ closest) {
    dist[j] = sqrt(bd2);
    idx[j] = bi == kNone ? (int64_t)-1 : (int64_t)bi;
    if (closest) {
        double mx = nan64(), my = nan64(), mz = nan64();
        if (bi != kNone) tri_dist<true>(qx, qy, qz, tri + (int64_t)bi * 9, mx, my, mz);
        closest[j * 3 + 0] = mx;
        closest[j * 3 + 1] = my;
        closest[j * 3 + 2] = mz;
    }
}

__global__ __launch_bounds__(kBlock) void ptm_query_kernel(const double* __restrict__ tri, int n_faces,
                                                            const int2* __restrict__ range, const int32_t* __restrict__ sids,
                                                            const int32_t* __restrict__ large_ids, int n_large,
                                                            const double* __restrict__ q, const int64_t* __restrict__ q_order,
                                                            int64_t n, Grid g, int max_shell, double margin,
                                                            double* __restrict__ dist, int64_t* __restrict__ idx,
                                                            double* __restrict__ closest, int32_t* __restrict__ escaped,
                                                            int32_t* __restrict__ n_escaped) {
    __shared__ double ltile[kLargeTile * 9];
    __shared__ int lid[kLargeTile];
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t j = t < n ? q_order[t] : -1;
    if (j >= n) j = -1;
    const bool live = j >= 0;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (live) { qx = q[j * 3 + 0]; qy = q[j * 3 + 1]; qz = q[j * 3 + 2]; }
    double bd2 = inf64();
    int bi = kNone;
    // the large list first: every lane of the workgroup against the same LDS tile
    for (int base = 0; base < n_large; base += kLargeTile) {
        const int cnt = min(kLargeTile, n_large - base);
        __syncthreads();
        if (threadIdx.x < cnt) {
            const int id = large_ids[base + threadIdx.x];
            lid[threadIdx.x] = (unsigned)id < (unsigned)n_faces ? id : -1;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < cnt * 9; k += kBlock) {
            const int id = lid[k / 9];
            ltile[k] = id >= 0 ? tri[(int64_t)id * 9 + k % 9] : 0.0;
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k < cnt; ++k) {
                const int id = lid[k];
                if (id < 0) continue;
                const double d2 = tri_d2(qx, qy, qz, ltile + k * 9);
                if (better(d2, id, bd2, bi)) { bd2 = d2; bi = id; }
            }
        }
    }
    if (!live) return;
    const int cx = cell_of(qx, g.lo[0], g.inv_h, g.dim[0]);
    const int cy = cell_of(qy, g.lo[1], g.inv_h, g.dim[1]);
    const int cz = cell_of(qz, g.lo[2], g.inv_h, g.dim[2]);
    const int DX = g.dim[0], DY = g.dim[1], DZ = g.dim[2];
    bool done = false;
    for (int r = 0; r <= max_shell; ++r) {
        const int x0 = max(cx - r, 0), x1 = min(cx + r, DX - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, DY - 1);
        const int z0 = max(cz - r, 0), z1 = min(cz + r, DZ - 1);
        for (int ix = x0; ix <= x1; ++ix) {
            const bool xs = ix == cx - r || ix == cx + r;
            for (int iy = y0; iy <= y1; ++iy) {
                const int row = (ix * DY + iy) * DZ;
                if (xs || iy == cy - r || iy == cy + r) {  // a face row of the shell: every z
                    for (int iz = z0; iz <= z1; ++iz) scan_cell(range, sids, tri, n_faces, row + iz, qx, qy, qz, bd2, bi);
                } else {                                   // interior row: the two z caps only
                    if (cz - r >= 0) scan_cell(range, sids, tri, n_faces, row + cz - r, qx, qy, qz, bd2, bi);
                    if (cz + r <= DZ - 1) scan_cell(range, sids, tri, n_faces, row + cz + r, qx, qy, qz, bd2, bi);
                }
            }
        }
        // distance to the faces of the block [c - r, c + r + 1) that are not on the grid boundary
        double b = inf64();
        bool open = false;
        const double qa[3] = {qx, qy, qz};
        const int ca[3] = {cx, cy, cz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (ca[a] - r > 0) { b = fmin(b, qa[a] - (g.lo[a] + (double)(ca[a] - r) * g.h)); open = true; }
            if (ca[a] + r + 1 < g.dim[a]) { b = fmin(b, (g.lo[a] + (double)(ca[a] + r + 1) * g.h) - qa[a]); open = true; }
        }
        if (!open) { done = true; break; }  // the block covers the whole grid: every triangle was visited
        const double bm = b - margin;
        if (bm > 0.0 && bd2 < bm * bm) { done = true; break; }
    }
    if (done) {
        write_out(tri, j, qx, qy, qz, bd2, bi, dist, idx, closest);
    } else {
        const int slot = atomicAdd(n_escaped, 1);
        if (slot >= 0 && slot < n) escaped[slot] = (int32_t)j;
    }
}

// escaped queries x a slice of the triangles: grid (ceil(n_esc / 256), n_split).  PASS 1: best[e] = min of the bits of d^2
// (d^2 >= 0, so its bits order like the value).  PASS 2: best[n_esc + e] = min index among the triangles whose d^2 has
// exactly those bits.  Both passes scan with the same (d^2, index) rule, so a slice's local winner is its smallest index
// at the slice's minimum.
template <int PASS>
__global__ __launch_bounds__(kBlock) void ptm_brute_kernel(const double* __restrict__ tri, const uint8_t* __restrict__ valid,
                                                            int64_t n_faces, int64_t per_split, const double* __restrict__ q,
                                                            int64_t n, const int32_t* __restrict__ escaped, int64_t n_esc,
                                                            unsigned long long* __restrict__ best) {
    __shared__ double tile[kBruteTile * 9];
    __shared__ uint8_t tvalid[kBruteTile];
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t j = e < n_esc ? escaped[e] : -1;
    if (j >= n) j = -1;
    const bool live = j >= 0;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (live) { qx = q[j * 3 + 0]; qy = q[j * 3 + 1]; qz = q[j * 3 + 2]; }
    const int64_t p0 = (int64_t)blockIdx.y * per_split;
    const int64_t p1 = min(n_faces, p0 + per_split);
    double bd2 = inf64();
    int bi = kNone;
    for (int64_t base = p0; base < p1; base += kBruteTile) {
        const int cnt = (int)min((int64_t)kBruteTile, p1 - base);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt * 9; k += kBlock) tile[k] = tri[base * 9 + k];
        if (threadIdx.x < cnt) tvalid[threadIdx.x] = valid[base + threadIdx.x];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            if (!tvalid[k]) continue;
            const double d2 = tri_d2(qx, qy, qz, tile + k * 9);
            const int id = (int)(base + k);
            if (better(d2, id, bd2, bi)) { bd2 = d2; bi = id; }
        }
    }
    if (!live || p1 <= p0) return;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(bd2);
    if (PASS == 1) {
        atomicMin(&best[e], bits);
    } else {
        if (bi != kNone && bits == best[e]) atomicMin(&best[n_esc + e], (unsigned long long)(unsigned)bi);
    }
}

__global__ __launch_bounds__(kBlock) void ptm_brute_finish_kernel(const double* __restrict__ tri, int64_t n_faces,
                                                                   const double* __restrict__ q, int64_t n,
                                                                   const int32_t* __restrict__ escaped, int64_t n_esc,
                                                                   const unsigned long long* __restrict__ best,
                                                                   double* __restrict__ dist, int64_t* __restrict__ idx,
                                                                   double* __restrict__ closest) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_esc) return;
    const int64_t j = escaped[e];
    if (j < 0 || j >= n) return;
    const unsigned long long bits = best[e], w = best[n_esc + e];
    const bool none = bits == ~0ull || w >= (unsigned long long)n_faces;
    const double bd2 = none ? inf64() : __longlong_as_double((long long)bits);
    write_out(tri, j, q[j * 3 + 0], q[j * 3 + 1], q[j * 3 + 2], bd2, none ? kNone : (int)w, dist, idx, closest);
}

constexpr int64_t kMaxCount = 0x7fffffffll;

bool grid_ok(const NcwPtmGrid* g) {
    if (!g || !(g->h > 0.0) || !(g->inv_h > 0.0)) return false;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (g->dim[a] < 1 || !(g->lo[a] == g->lo[a])) return false;
        cells *= g->dim[a];
        if (cells > (int64_t)1 << 30) return false;
    }
    return true;
}

Grid to_grid(const NcwPtmGrid* g) {
    Grid o;
    for (int a = 0; a < 3; ++a) { o.lo[a] = g->lo[a]; o.dim[a] = g->dim[a]; }
    o.h = g->h;
    o.inv_h = g->inv_h;
    return o;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" int ncw_ptm_pack(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const double* centre,
                            const double* box, double* tri, uint8_t* valid, void* stream) {
    if (n_faces == 0) return 0;
    if (!faces || !centre || !tri || !valid || n_faces < 0 || n_faces > kMaxCount || n_verts < 0 || (n_verts > 0 && !verts))
        return NCW_E_BADARG;
    Box b;
    b.on = box != nullptr;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = box ? box[a] : 0.0;
        b.hi[a] = box ? box[3 + a] : 0.0;
    }
    hipLaunchKernelGGL(ptm_pack_kernel, dim3(blocks_of(n_faces)), dim3(kBlock), 0, (hipStream_t)stream, verts, n_verts, faces,
                       n_faces, centre[0], centre[1], centre[2], b, tri, valid);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_ptm_count(const double* tri, const uint8_t* valid, int64_t n_faces, const NcwPtmGrid* grid,
                             int64_t max_cells_per_tri, int32_t* count, uint8_t* large, void* stream) {
    if (n_faces == 0) return 0;
    if (!tri || !valid || !count || !large || !grid_ok(grid) || n_faces < 0 || n_faces > kMaxCount || max_cells_per_tri < 1 ||
        max_cells_per_tri > (int64_t)1 << 30)
        return NCW_E_BADARG;
    hipLaunchKernelGGL(ptm_count_kernel, dim3(blocks_of(n_faces)), dim3(kBlock), 0, (hipStream_t)stream, tri, valid, n_faces,
                       to_grid(grid), max_cells_per_tri, count, large);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_ptm_emit(const double* tri, const int32_t* count, const int64_t* cum, int64_t n_faces, const NcwPtmGrid* grid,
                            int64_t n_pairs, int32_t* keys, int32_t* ids, void* stream) {
    if (n_faces == 0 || n_pairs == 0) return 0;
    if (!tri || !count || !cum || !keys || !ids || !grid_ok(grid) || n_faces < 0 || n_faces > kMaxCount || n_pairs < 0 ||
        n_pairs > kMaxCount)
        return NCW_E_BADARG;
    hipLaunchKernelGGL(ptm_emit_kernel, dim3(blocks_of(n_faces)), dim3(kBlock), 0, (hipStream_t)stream, tri, count, cum, n_faces,
                       to_grid(grid), n_pairs, keys, ids);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_ptm_ranges(const int32_t* sorted_keys, const int64_t* order, const int32_t* ids, int64_t n_pairs, int64_t n_cells,
                              int32_t* cell_range, int32_t* sorted_ids, void* stream) {
    if (n_pairs == 0) return 0;
    if (!sorted_keys || !order || !ids || !cell_range || !sorted_ids || n_pairs < 0 || n_pairs > kMaxCount || n_cells < 1 ||
        n_cells > (int64_t)1 << 30)
        return NCW_E_BADARG;
    hipLaunchKernelGGL(ptm_ranges_kernel, dim3(blocks_of(n_pairs)), dim3(kBlock), 0, (hipStream_t)stream, sorted_keys, order, ids,
                       n_pairs, n_cells, (int2*)cell_range, sorted_ids);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_ptm_cell_keys(const double* q, int64_t n, const NcwPtmGrid* grid, int32_t* keys, void* stream) {
    if (n == 0) return 0;
    if (!q || !keys || !grid_ok(grid) || n < 0 || n > kMaxCount) return NCW_E_BADARG;
    hipLaunchKernelGGL(ptm_cell_keys_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, q, n, to_grid(grid), keys);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_ptm_query(const double* tri, int64_t n_faces, const int32_t* cell_range, const int32_t* sorted_ids,
                             const int32_t* large_ids, int64_t n_large, const double* q, const int64_t* q_order, int64_t n,
                             const NcwPtmGrid* grid, int max_shell, double margin, double* dist, int64_t* idx, double* closest,
                             int32_t* escaped, int32_t* n_escaped, void* stream) {
    if (n == 0) return 0;
    // sorted_ids may be NULL only when no pair exists (every cell range is then empty)
    if (!tri || !cell_range || !q || !q_order || !dist || !idx || !escaped || !n_escaped || !grid_ok(grid) || n < 0 ||
        n > kMaxCount || n_faces < 1 || n_faces > kMaxCount || n_large < 0 || n_large > n_faces || (n_large > 0 && !large_ids) ||
        max_shell < 0 || !(margin >= 0.0))
        return NCW_E_BADARG;
    hipLaunchKernelGGL(ptm_query_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, tri, (int)n_faces,
                       (const int2*)cell_range, sorted_ids, large_ids, (int)n_large, q, q_order, n, to_grid(grid), max_shell, margin,
                       dist, idx, closest, escaped, n_escaped);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_ptm_brute(const double* tri, const uint8_t* valid, int64_t n_faces, const double* q, int64_t n,
                             const int32_t* escaped, int64_t n_esc, uint64_t* scratch, double* dist, int64_t* idx, double* closest,
                             void* stream) {
    if (n_esc == 0) return 0;
    if (!tri || !valid || !q || !escaped || !scratch || !dist || !idx || n_faces < 1 || n_faces > kMaxCount || n < 1 ||
        n > kMaxCount || n_esc < 0 || n_esc > n)
        return NCW_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(scratch, 0xff, (size_t)n_esc * 2 * sizeof(uint64_t), s) != hipSuccess) return NCW_E_BADARG;
    const int64_t qblocks = (n_esc + kBlock - 1) / kBlock;
    // split the triangles so that about 2048 blocks are in flight, each slice at least 4 tiles long
    int64_t n_split = 2048 / qblocks;
    n_split = max((int64_t)1, min(n_split, (n_faces + 4 * kBruteTile - 1) / (4 * kBruteTile)));
    n_split = min(n_split, (int64_t)65535);
    const int64_t per_split = (n_faces + n_split - 1) / n_split;
    unsigned long long* best = (unsigned long long*)scratch;
    hipLaunchKernelGGL(ptm_brute_kernel<1>, dim3((unsigned)qblocks, (unsigned)n_split), dim3(kBlock), 0, s, tri, valid, n_faces,
                       per_split, q, n, escaped, n_esc, best);
    NCW_CHECK_LAUNCH();
    hipLaunchKernelGGL(ptm_brute_kernel<2>, dim3((unsigned)qblocks, (unsigned)n_split), dim3(kBlock), 0, s, tri, valid, n_faces,
                       per_split, q, n, escaped, n_esc, best);
    NCW_CHECK_LAUNCH();
    hipLaunchKernelGGL(ptm_brute_finish_kernel, dim3(blocks_of(n_esc)), dim3(kBlock), 0, s, tri, n_faces, q, n, escaped, n_esc,
                       (const unsigned long long*)best, dist, idx, closest);
    NCW_CHECK_LAUNCH();
    return 0;
}
