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
