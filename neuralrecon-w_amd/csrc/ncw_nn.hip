// Exact 1-nearest-neighbour search between point clouds on the GPU (mesh evaluation): replaces the
// per-point `scipy.spatial.KDTree.query` loop of utils/eval_utils.py:126-154 (`nn_correspondance`, use_o3d=False).
//
// Uniform grid over a box chosen by the caller (evalmesh.NNGrid: P's box without its 0.1 % tails); points and queries
// outside it are clamped into the boundary cells, which keeps the search exact (a point in a cell beyond a block face lies
// beyond that face, clamped or not, and faces on the grid boundary never enter the stop bound):
//   ncw_nn_cell_keys   : linear cell key of every point (x slowest);
//   (caller)           : stable sort of (key, index) -- plumbing (torch.sort);
//   ncw_nn_cell_ranges : [start, end) of every non-empty cell in a dense table, plus P reordered by cell as float4
//                        (x, y, z, original index as int bits) so that a cell's points are one contiguous run;
//   ncw_nn_query       : one lane per query (queries visited in cell order, so a wavefront walks neighbouring cells):
//                        Chebyshev shells r = 0, 1, 2, ... around the query's cell, best (d^2, index) kept; after shell r
//                        the search stops once best d^2 < (b - margin)^2, b = distance from the query to the faces of the
//                        (2r+1)^3 block that are not on the grid boundary (every unvisited point lies beyond one of those
//                        faces), or once the block covers the whole grid.  A query still open after `max_shell` shells is
//                        appended to an escape list;
//   ncw_nn_brute       : the escaped queries against all of P (P staged through LDS, P split over blocks, the per-query
//                        minimum formed by a 64-bit atomicMin of (d^2 bits, index) -- exact and order-independent).
// "The nearest point within R, or nothing" (the ICP gate of align.py, the marking threshold of reproj.py) needs neither the
// escape list nor the brute-force pass:
//   ncw_nn_coarse      : points per block of B^3 cells (B a power of two), from the cell table alone -- a second, coarse level;
//   ncw_nn_query_within: one lane per query in cell order, ONE launch: fine shells 0..2 as above, then Chebyshev shells of
//                        coarse blocks around the query's block.  A block or a cell is skipped without a lookup when the
//                        squared distance to its box, each axis gap less the margin, is STRICTLY above min(best d^2, r^2); an
//                        empty block costs one lookup; a non-empty one is opened cell by cell with `scan_cell`.  The box of
//                        a boundary cell extends to infinity on its outward sides (that is where the clamped points are), so
//                        faces on the grid boundary give no gap -- the same rule as the stop bound.  The walk ends when the
//                        faces of the visited blocks are farther than min(best, r) or the blocks cover the grid.  The answer is
//                        the unbounded one if d^2 <= r^2 (inclusive), else +inf / -1; r = +inf gives the unbounded answer.
//                        No atomics; the same d^2 expression (and, in the ISA, the same fma form) as the two kernels above,
//                        so a qualifying query has their bits.
// d^2 is formed from coordinate differences (dx*dx + dy*dy + dz*dz), never as |a|^2 + |b|^2 - 2 a.b, which cancels where the
// F-score thresholds live.  Ties on equal d^2 go to the smaller index (= argmin of a brute-force distance matrix), so the
// result is deterministic and exact for every input.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kBruteTile = 256;  // P points per LDS tile of the escape kernel

struct Grid {
    float lo[3];
    float h, inv_h;
    int dim[3];
};

__device__ __forceinline__ int cell_of(float x, float lo, float inv_h, int dim) {
    const int c = (int)floorf((x - lo) * inv_h);
    return c < 0 ? 0 : (c >= dim ? dim - 1 : c);
}

__device__ __forceinline__ bool better(float d2, int i, float bd2, int bi) { return d2 < bd2 || (d2 == bd2 && i < bi); }

__global__ __launch_bounds__(kBlock) void nn_cell_keys_kernel(const float* __restrict__ pts, int64_t n, Grid g,
                                                               int32_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int cx = cell_of(pts[i * 3 + 0], g.lo[0], g.inv_h, g.dim[0]);
    const int cy = cell_of(pts[i * 3 + 1], g.lo[1], g.inv_h, g.dim[1]);
    const int cz = cell_of(pts[i * 3 + 2], g.lo[2], g.inv_h, g.dim[2]);
    keys[i] = (cx * g.dim[1] + cy) * g.dim[2] + cz;
}

__global__ __launch_bounds__(kBlock) void nn_cell_ranges_kernel(const float* __restrict__ pts, const int32_t* __restrict__ skeys,
                                                                 const int64_t* __restrict__ order, int64_t m,
                                                                 int2* __restrict__ range, float4* __restrict__ psorted) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int32_t k = skeys[i];
    if (i == 0 || skeys[i - 1] != k) range[k].x = (int)i;
    if (i == m - 1 || skeys[i + 1] != k) range[k].y = (int)(i + 1);
    const int64_t j = order[i];
    psorted[i] = make_float4(pts[j * 3 + 0], pts[j * 3 + 1], pts[j * 3 + 2], __int_as_float((int)j));
}

__device__ __forceinline__ void scan_cell(const int2* __restrict__ range, const float4* __restrict__ ps, int key, float qx,
                                          float qy, float qz, float& bd2, int& bi) {
    const int2 r = range[key];
    for (int p = r.x; p < r.y; ++p) {
        const float4 v = ps[p];
        const float dx = v.x - qx, dy = v.y - qy, dz = v.z - qz;
        const float d2 = dx * dx + dy * dy + dz * dz;
        const int id = __float_as_int(v.w);
        if (better(d2, id, bd2, bi)) { bd2 = d2; bi = id; }
    }
}

__global__ __launch_bounds__(kBlock) void nn_query_kernel(const float4* __restrict__ ps, const int2* __restrict__ range,
                                                           const float* __restrict__ q, const int64_t* __restrict__ q_order,
                                                           int64_t n, Grid g, int max_shell, float margin,
                                                           float* __restrict__ dist, int64_t* __restrict__ idx,
                                                           int32_t* __restrict__ escaped, int32_t* __restrict__ n_escaped) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const int64_t j = q_order[t];
    const float qx = q[j * 3 + 0], qy = q[j * 3 + 1], qz = q[j * 3 + 2];
    const int cx = cell_of(qx, g.lo[0], g.inv_h, g.dim[0]);
    const int cy = cell_of(qy, g.lo[1], g.inv_h, g.dim[1]);
    const int cz = cell_of(qz, g.lo[2], g.inv_h, g.dim[2]);
    const int DX = g.dim[0], DY = g.dim[1], DZ = g.dim[2];
    float bd2 = __int_as_float(0x7f800000);  // +inf
    int bi = 0x7fffffff;
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
                    for (int iz = z0; iz <= z1; ++iz) scan_cell(range, ps, row + iz, qx, qy, qz, bd2, bi);
                } else {                                   // interior row: the two z caps only
                    if (cz - r >= 0) scan_cell(range, ps, row + cz - r, qx, qy, qz, bd2, bi);
                    if (cz + r <= DZ - 1) scan_cell(range, ps, row + cz + r, qx, qy, qz, bd2, bi);
                }
            }
        }
        // distance to the faces of the block [c - r, c + r + 1) that are not on the grid boundary
        float b = __int_as_float(0x7f800000);
        bool open = false;
        const float qa[3] = {qx, qy, qz};
        const int ca[3] = {cx, cy, cz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (ca[a] - r > 0) { b = fminf(b, qa[a] - (g.lo[a] + (float)(ca[a] - r) * g.h)); open = true; }
            if (ca[a] + r + 1 < g.dim[a]) { b = fminf(b, (g.lo[a] + (float)(ca[a] + r + 1) * g.h) - qa[a]); open = true; }
        }
        if (!open) { done = true; break; }  // the block covers the whole grid: every point was visited
        const float bm = b - margin;
        if (bm > 0.f && bd2 < bm * bm) { done = true; break; }
    }
    if (done) {
        dist[j] = sqrtf(bd2);
        idx[j] = bi;
    } else {
        escaped[atomicAdd(n_escaped, 1)] = (int32_t)j;
    }
}

// escaped queries x a slice of P: grid (ceil(n_esc / 256), n_split); per-query minimum over the slices by a 64-bit atomicMin
// of (d^2 bits << 32 | index) -- d^2 >= 0 so its bits order like the value, and the low word breaks ties to the smaller index
__global__ __launch_bounds__(kBlock) void nn_brute_kernel(const float4* __restrict__ ps, int64_t m, int64_t per_split,
                                                           const float* __restrict__ q, const int32_t* __restrict__ escaped,
                                                           int64_t n_esc, unsigned long long* __restrict__ best) {
    __shared__ float4 tile[kBruteTile];
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = e < n_esc;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) {
        const int64_t j = escaped[e];
        qx = q[j * 3 + 0]; qy = q[j * 3 + 1]; qz = q[j * 3 + 2];
    }
    const int64_t p0 = (int64_t)blockIdx.y * per_split;
    const int64_t p1 = min(m, p0 + per_split);
    float bd2 = __int_as_float(0x7f800000);
    int bi = 0x7fffffff;
    for (int64_t base = p0; base < p1; base += kBruteTile) {
        const int cnt = (int)min((int64_t)kBruteTile, p1 - base);
        __syncthreads();
        if (threadIdx.x < cnt) tile[threadIdx.x] = ps[base + threadIdx.x];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const float4 v = tile[k];
            const float dx = v.x - qx, dy = v.y - qy, dz = v.z - qz;
            const float d2 = dx * dx + dy * dy + dz * dz;
            const int id = __float_as_int(v.w);
            if (better(d2, id, bd2, bi)) { bd2 = d2; bi = id; }
        }
    }
    if (live && p1 > p0)
        atomicMin(&best[e], ((unsigned long long)__float_as_uint(bd2) << 32) | (unsigned long long)(unsigned)bi);
}

__global__ __launch_bounds__(kBlock) void nn_brute_finish_kernel(const int32_t* __restrict__ escaped, int64_t n_esc,
                                                                  const unsigned long long* __restrict__ best,
                                                                  float* __restrict__ dist, int64_t* __restrict__ idx) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_esc) return;
    const unsigned long long v = best[e];
    const int64_t j = escaped[e];
    dist[j] = sqrtf(__uint_as_float((unsigned)(v >> 32)));
    idx[j] = (int64_t)(unsigned)(v & 0xffffffffull);
}

// ---- nearest point within a radius: fine shells, then shells of coarse blocks (no escape list, no brute-force pass) ----
constexpr int kFineShells = 2;  // fine Chebyshev shells walked before the coarse blocks take over (a 5^3 block of cells)

// points per block of B^3 fine cells (B = 1 << shift), from the cell table alone
__global__ __launch_bounds__(kBlock) void nn_coarse_kernel(const int2* __restrict__ range, Grid g, int shift, int CX, int CY, int CZ,
                                                            int32_t* __restrict__ coarse) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (int64_t)CX * CY * CZ) return;
    const int bz = (int)(k % CZ), by = (int)((k / CZ) % CY), bx = (int)(k / ((int64_t)CZ * CY));
    const int B = 1 << shift;
    const int x0 = bx << shift, x1 = min(x0 + B, g.dim[0]);
    const int y0 = by << shift, y1 = min(y0 + B, g.dim[1]);
    const int z0 = bz << shift, z1 = min(z0 + B, g.dim[2]);
    int cnt = 0;
    for (int ix = x0; ix < x1; ++ix)
        for (int iy = y0; iy < y1; ++iy) {
            const int row = (ix * g.dim[1] + iy) * g.dim[2];
            for (int iz = z0; iz < z1; ++iz) {
                const int2 r = range[row + iz];
                cnt += r.y - r.x;
            }
        }
    coarse[k] = cnt;
}

// squared lower bound, along one axis, of the distance from q to any point bucketed in the cells [c0, c1) of that axis, less
// the margin.  Points outside the grid box are clamped into the boundary cells, so the box of a boundary cell extends to
// infinity on its outward side: a face on the grid boundary gives no bound.
__device__ __forceinline__ float axis_gap2(float q, float lo, float h, int c0, int c1, int dim, float margin) {
    float a = 0.f;
    if (c0 > 0) a = fmaxf(a, (lo + (float)c0 * h) - q);
    if (c1 < dim) a = fmaxf(a, q - (lo + (float)c1 * h));
    a = fmaxf(a - margin, 0.f);
    return a * a;
}

struct Walk {
    const float4* __restrict__ ps;
    const int2* __restrict__ range;
    const int32_t* __restrict__ coarse;
    Grid g;
    int shift, CY, CZ;
    int cx, cy, cz;
    float qx, qy, qz, margin, r2;
};

// one coarse block (jx, jy, jz); gxy = the squared gaps of its x and y slabs.  A block or a cell is skipped when its bound is
// STRICTLY above min(best d^2, r^2): a point at equal d^2 (a tie to a smaller index, or d^2 == r^2) is never lost.  The
// cells of the fine shells already walked are skipped too (visiting one again would change nothing: `better` is strict).
__device__ __forceinline__ void visit_block(const Walk& w, int jx, int jy, int jz, float gxy, float& bd2, int& bi) {
    const int DX = w.g.dim[0], DY = w.g.dim[1], DZ = w.g.dim[2];
    const int B = 1 << w.shift;
    const int z0 = jz << w.shift, z1 = min(z0 + B, DZ);
    if (gxy + axis_gap2(w.qz, w.g.lo[2], w.g.h, z0, z1, DZ, w.margin) > fminf(bd2, w.r2)) return;
    if (w.coarse[(jx * w.CY + jy) * w.CZ + jz] == 0) return;  // an empty block: one lookup
    const int x0 = jx << w.shift, x1 = min(x0 + B, DX);
    const int y0 = jy << w.shift, y1 = min(y0 + B, DY);
    for (int ix = x0; ix < x1; ++ix) {
        const float fx = axis_gap2(w.qx, w.g.lo[0], w.g.h, ix, ix + 1, DX, w.margin);
        if (fx > fminf(bd2, w.r2)) continue;
        const bool nx = abs(ix - w.cx) <= kFineShells;
        for (int iy = y0; iy < y1; ++iy) {
            const float fxy = fx + axis_gap2(w.qy, w.g.lo[1], w.g.h, iy, iy + 1, DY, w.margin);
            if (fxy > fminf(bd2, w.r2)) continue;
            const bool nxy = nx && abs(iy - w.cy) <= kFineShells;
            const int row = (ix * DY + iy) * DZ;
            for (int iz = z0; iz < z1; ++iz) {
                if (nxy && abs(iz - w.cz) <= kFineShells) continue;
                if (fxy + axis_gap2(w.qz, w.g.lo[2], w.g.h, iz, iz + 1, DZ, w.margin) > fminf(bd2, w.r2)) continue;
                scan_cell(w.range, w.ps, row + iz, w.qx, w.qy, w.qz, bd2, bi);
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void nn_within_kernel(const float4* __restrict__ ps, const int2* __restrict__ range,
                                                            const int32_t* __restrict__ coarse, int shift,
                                                            const float* __restrict__ q, const int64_t* __restrict__ q_order,
                                                            int64_t n, Grid g, float margin, float r2, float* __restrict__ dist,
                                                            int64_t* __restrict__ idx) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const int64_t j = q_order[t];
    const float qx = q[j * 3 + 0], qy = q[j * 3 + 1], qz = q[j * 3 + 2];
    const float inf = __int_as_float(0x7f800000);
    if (!(qx == qx && qy == qy && qz == qz)) {  // NaN: every comparison below is false and the walk would cover the grid
        dist[j] = inf;
        idx[j] = -1;
        return;
    }
    if (fabsf(qx) == inf || fabsf(qy) == inf || fabsf(qz) == inf) {  // every d^2 is +inf: the tie goes to index 0
        dist[j] = inf;
        idx[j] = r2 == inf ? 0 : -1;
        return;
    }
    const int cx = cell_of(qx, g.lo[0], g.inv_h, g.dim[0]);
    const int cy = cell_of(qy, g.lo[1], g.inv_h, g.dim[1]);
    const int cz = cell_of(qz, g.lo[2], g.inv_h, g.dim[2]);
    const int DX = g.dim[0], DY = g.dim[1], DZ = g.dim[2];
    const float qa[3] = {qx, qy, qz};
    float bd2 = inf;
    int bi = 0x7fffffff;
    bool done = false;
    // fine shells, as nn_query_kernel walks them; the stop test also closes on the radius
    for (int r = 0; r <= kFineShells; ++r) {
        const int x0 = max(cx - r, 0), x1 = min(cx + r, DX - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, DY - 1);
        const int z0 = max(cz - r, 0), z1 = min(cz + r, DZ - 1);
        for (int ix = x0; ix <= x1; ++ix) {
            const bool xs = ix == cx - r || ix == cx + r;
            for (int iy = y0; iy <= y1; ++iy) {
                const int row = (ix * DY + iy) * DZ;
                if (xs || iy == cy - r || iy == cy + r) {
                    for (int iz = z0; iz <= z1; ++iz) scan_cell(range, ps, row + iz, qx, qy, qz, bd2, bi);
                } else {
                    if (cz - r >= 0) scan_cell(range, ps, row + cz - r, qx, qy, qz, bd2, bi);
                    if (cz + r <= DZ - 1) scan_cell(range, ps, row + cz + r, qx, qy, qz, bd2, bi);
                }
            }
        }
        float b = inf;
        bool open = false;
        const int ca[3] = {cx, cy, cz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (ca[a] - r > 0) { b = fminf(b, qa[a] - (g.lo[a] + (float)(ca[a] - r) * g.h)); open = true; }
            if (ca[a] + r + 1 < g.dim[a]) { b = fminf(b, (g.lo[a] + (float)(ca[a] + r + 1) * g.h) - qa[a]); open = true; }
        }
        if (!open) { done = true; break; }
        const float bm = b - margin;
        if (bm > 0.f && fminf(bd2, r2) < bm * bm) { done = true; break; }
    }
    if (!done) {
        // shells of coarse blocks around the query's block: R = 0 holds the rest of its own block
        Walk w;
        w.ps = ps; w.range = range; w.coarse = coarse; w.g = g; w.shift = shift;
        w.cx = cx; w.cy = cy; w.cz = cz; w.qx = qx; w.qy = qy; w.qz = qz; w.margin = margin; w.r2 = r2;
        const int B = 1 << shift;
        const int CX = (DX + B - 1) >> shift, CY = (DY + B - 1) >> shift, CZ = (DZ + B - 1) >> shift;
        w.CY = CY; w.CZ = CZ;
        const int ba[3] = {cx >> shift, cy >> shift, cz >> shift};
        const int Ca[3] = {CX, CY, CZ};
        for (int R = 0;; ++R) {
            const int x0 = max(ba[0] - R, 0), x1 = min(ba[0] + R, CX - 1);
            const int y0 = max(ba[1] - R, 0), y1 = min(ba[1] + R, CY - 1);
            const int z0 = max(ba[2] - R, 0), z1 = min(ba[2] + R, CZ - 1);
            for (int jx = x0; jx <= x1; ++jx) {
                const bool xs = jx == ba[0] - R || jx == ba[0] + R;
                const float gx = axis_gap2(qx, g.lo[0], g.h, jx << shift, min((jx + 1) << shift, DX), DX, margin);
                if (gx > fminf(bd2, r2)) continue;
                for (int jy = y0; jy <= y1; ++jy) {
                    const float gxy = gx + axis_gap2(qy, g.lo[1], g.h, jy << shift, min((jy + 1) << shift, DY), DY, margin);
                    if (gxy > fminf(bd2, r2)) continue;
                    if (xs || jy == ba[1] - R || jy == ba[1] + R) {
                        for (int jz = z0; jz <= z1; ++jz) visit_block(w, jx, jy, jz, gxy, bd2, bi);
                    } else {
                        if (ba[2] - R >= 0) visit_block(w, jx, jy, ba[2] - R, gxy, bd2, bi);
                        if (R > 0 && ba[2] + R <= CZ - 1) visit_block(w, jx, jy, ba[2] + R, gxy, bd2, bi);
                    }
                }
            }
            // every unvisited point lies beyond a face, not on the grid boundary, of the blocks [b - R, b + R + 1)
            float b = inf;
            bool open = false;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int f0 = max(ba[a] - R, 0) << shift;
                const int f1 = min(ba[a] + R + 1, Ca[a]) << shift;
                if (f0 > 0) { b = fminf(b, qa[a] - (g.lo[a] + (float)f0 * g.h)); open = true; }
                if (f1 < g.dim[a]) { b = fminf(b, (g.lo[a] + (float)f1 * g.h) - qa[a]); open = true; }
            }
            if (!open) break;  // the blocks cover the whole grid
            const float bm = b - margin;
            if (bm > 0.f && fminf(bd2, r2) < bm * bm) break;
        }
    }
    const bool hit = bd2 <= r2;  // inclusive
    dist[j] = hit ? sqrtf(bd2) : inf;
    idx[j] = hit ? (int64_t)bi : (int64_t)-1;
}

bool grid_ok(const NcwNnGrid* g) {
    if (!g || !(g->h > 0.f) || !(g->inv_h > 0.f)) return false;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (g->dim[a] < 1) return false;
        cells *= g->dim[a];
    }
    return cells <= (int64_t)1 << 30;
}

Grid to_grid(const NcwNnGrid* g) {
    Grid o;
    for (int a = 0; a < 3; ++a) { o.lo[a] = g->lo[a]; o.dim[a] = g->dim[a]; }
    o.h = g->h;
    o.inv_h = g->inv_h;
    return o;
}

}  // namespace

extern "C" int ncw_nn_cell_keys(const float* pts, int64_t n, const NcwNnGrid* grid, int32_t* keys, void* stream) {
    if (n <= 0) return 0;
    if (!pts || !keys || !grid_ok(grid)) return NCW_E_BADARG;
    hipLaunchKernelGGL(nn_cell_keys_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       pts, n, to_grid(grid), keys);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_nn_cell_ranges(const float* pts, const int32_t* sorted_keys, const int64_t* order, int64_t m,
                                  int32_t* cell_range, float* pts_sorted, void* stream) {
    if (m <= 0) return 0;
    if (!pts || !sorted_keys || !order || !cell_range || !pts_sorted || m > 0x7fffffffll) return NCW_E_BADARG;
    hipLaunchKernelGGL(nn_cell_ranges_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       pts, sorted_keys, order, m, (int2*)cell_range, (float4*)pts_sorted);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_nn_query(const float* pts_sorted, const int32_t* cell_range, const float* q, const int64_t* q_order, int64_t n,
                            const NcwNnGrid* grid, int max_shell, float margin, float* dist, int64_t* idx, int32_t* escaped,
                            int32_t* n_escaped, void* stream) {
    if (n <= 0) return 0;
    if (!pts_sorted || !cell_range || !q || !q_order || !dist || !idx || !escaped || !n_escaped || !grid_ok(grid) ||
        max_shell < 0 || !(margin >= 0.f))
        return NCW_E_BADARG;
    hipLaunchKernelGGL(nn_query_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)pts_sorted, (const int2*)cell_range, q, q_order, n, to_grid(grid), max_shell, margin, dist,
                       idx, escaped, n_escaped);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_nn_brute(const float* pts_sorted, int64_t m, const float* q, const int32_t* escaped, int64_t n_esc,
                            uint64_t* scratch, float* dist, int64_t* idx, void* stream) {
    if (n_esc <= 0) return 0;
    if (!pts_sorted || !q || !escaped || !scratch || !dist || !idx || m <= 0 || m > 0x7fffffffll) return NCW_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(scratch, 0xff, (size_t)n_esc * sizeof(uint64_t), s) != hipSuccess) return NCW_E_BADARG;
    const int64_t qblocks = (n_esc + kBlock - 1) / kBlock;
    // split P so that about 2048 blocks are in flight, each slice at least 4 tiles long
    int64_t n_split = 2048 / qblocks;
    n_split = max((int64_t)1, min(n_split, (m + 4 * kBruteTile - 1) / (4 * kBruteTile)));
    n_split = min(n_split, (int64_t)65535);
    const int64_t per_split = (m + n_split - 1) / n_split;
    hipLaunchKernelGGL(nn_brute_kernel, dim3((unsigned)qblocks, (unsigned)n_split), dim3(kBlock), 0, s, (const float4*)pts_sorted, m,
                       per_split, q, escaped, n_esc, (unsigned long long*)scratch);
    NCW_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_brute_finish_kernel, dim3((unsigned)qblocks), dim3(kBlock), 0, s, escaped, n_esc,
                       (const unsigned long long*)scratch, dist, idx);
    NCW_CHECK_LAUNCH();
    return 0;
}

namespace {
// B = 1 << shift for a power of two in [1, 65536]; -1 otherwise
int block_shift(int B) {
    if (B < 1 || B > 65536 || (B & (B - 1)) != 0) return -1;
    int s = 0;
    while ((1 << s) < B) ++s;
    return s;
}
}  // namespace

extern "C" int ncw_nn_coarse(const int32_t* cell_range, const NcwNnGrid* grid, int B, int32_t* coarse, void* stream) {
    const int shift = block_shift(B);
    if (!cell_range || !coarse || !grid_ok(grid) || shift < 0) return NCW_E_BADARG;
    const int CX = (grid->dim[0] + B - 1) >> shift, CY = (grid->dim[1] + B - 1) >> shift, CZ = (grid->dim[2] + B - 1) >> shift;
    const int64_t nc = (int64_t)CX * CY * CZ;
    hipLaunchKernelGGL(nn_coarse_kernel, dim3((unsigned)((nc + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const int2*)cell_range, to_grid(grid), shift, CX, CY, CZ, coarse);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_nn_query_within(const float* pts_sorted, const int32_t* cell_range, const int32_t* coarse, int B, const float* q,
                                   const int64_t* q_order, int64_t n, const NcwNnGrid* grid, float margin, float max_dist,
                                   float* dist, int64_t* idx, void* stream) {
    if (n <= 0) return 0;
    const int shift = block_shift(B);
    if (!pts_sorted || !cell_range || !coarse || !q || !q_order || !dist || !idx || !grid_ok(grid) || shift < 0 ||
        !(margin >= 0.f) || !(max_dist > 0.f))
        return NCW_E_BADARG;
    const float r2 = max_dist * max_dist;  // rounded once, here; +inf stays +inf
    hipLaunchKernelGGL(nn_within_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)pts_sorted, (const int2*)cell_range, coarse, shift, q, q_order, n, to_grid(grid), margin, r2,
                       dist, idx);
    NCW_CHECK_LAUNCH();
    return 0;
}
