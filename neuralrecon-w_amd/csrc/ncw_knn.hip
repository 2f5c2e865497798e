// Exact k nearest neighbours on the 1-NN grid of ncw_nn.hip (k <= 32), and the per-point PCA that turns a neighbour list into
// a normal: what a point cloud needs to get normals, to lose its stray points and to report normal consistency.
//
//   ncw_knn_query : one lane per query in cell order, ONE launch, over the tables of ncw_nn.hip (pts_sorted, cell_range, the
//                   coarse occupancy level).  The walk is nn_within_kernel's: fine Chebyshev shells 0..2 around the query's
//                   cell, then shells of coarse blocks; a block or a cell is skipped when the squared distance to its box is
//                   STRICTLY above min(kth, r2), kth = the current k-th best d2 (+inf while the list is short).  No escape
//                   list, no brute-force pass, no atomics.
//                   Two things matter here that cannot go wrong at k = 1:
//                     (a) a cell visited twice would enter the list twice.  The fine shells are disjoint, the coarse shells are
//                         disjoint, and the coarse phase skips the 5^3 fine cells already walked (it only runs when all three
//                         fine shells were walked): every cell is scanned at most once;
//                     (b) every bound is taken against kth, never against the best.
//                   The candidate list lives in LDS as [k][lanes of the workgroup] (d2, index) pairs -- a runtime-indexed
//                   private array would go to scratch -- so the lanes of a wave touch consecutive 8-byte words at one rank.  It is
//                   kept sorted by insertion ((d2, index) ascending); kth sits in registers, so a candidate that does not
//                   enter costs one compare and no LDS access.
//   ncw_knn_pca   : one lane per point: float64 mean and covariance of its members, cyclic Jacobi with a fixed operation
//                   sequence, normal / eigenvalues / curvature / validity.
// The file is compiled with -ffp-contract=off (build.py): d2 = dx*dx + dy*dy + dz*dz and every float64 operation below round
// once each, so tests/_knn_ref.py restates both kernels in numpy bit for bit.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

namespace {

constexpr int kFineShells = 2;  // as ncw_nn.hip: fine Chebyshev shells walked before the coarse blocks take over
constexpr int kMaxK = 32;

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

// see ncw_nn.hip: the squared lower bound along one axis, less the margin; faces on the grid boundary give no bound
__device__ __forceinline__ float axis_gap2(float q, float lo, float h, int c0, int c1, int dim, float margin) {
    float a = 0.f;
    if (c0 > 0) a = fmaxf(a, (lo + (float)c0 * h) - q);
    if (c1 < dim) a = fmaxf(a, q - (lo + (float)c1 * h));
    a = fmaxf(a - margin, 0.f);
    return a * a;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));  // (d2, index bits): a plain vector type, so it can sit in address space 3
typedef __attribute__((address_space(3))) f32x2 lds_pair;

// the sorted candidate list of one lane: rank r at lst[r * wg] (lst already offset by the lane)
struct List {
    lds_pair* lst;
    int wg, k, cnt;
    int excl;
    float r2;
    float kd2;  // (kd2, ki): the k-th best once the list is full, (+inf, INT_MAX) before
    int ki;
    int evals, inserts;
};

__device__ __forceinline__ void offer(List& L, float d2, int id) {
    ++L.evals;
    if (!better(d2, id, L.kd2, L.ki)) return;  // the common case: one compare (NaN d2 never enters)
    if (!(d2 <= L.r2) || id == L.excl) return;
    ++L.inserts;
    int p = L.cnt < L.k ? L.cnt : L.k - 1;  // the slot that opens: a new last rank, or the k-th best drops out
    if (L.cnt < L.k) ++L.cnt;
    while (p > 0) {
        const f32x2 u = L.lst[(p - 1) * L.wg];
        if (!better(d2, id, u.x, __float_as_int(u.y))) break;
        L.lst[p * L.wg] = u;
        --p;
    }
    L.lst[p * L.wg] = f32x2{d2, __int_as_float(id)};
    if (L.cnt == L.k) {
        const f32x2 u = L.lst[(L.k - 1) * L.wg];
        L.kd2 = u.x;
        L.ki = __float_as_int(u.y);
    }
}

__device__ __forceinline__ void scan_cell(const int2* __restrict__ range, const float4* __restrict__ ps, int key, float qx,
                                          float qy, float qz, List& L) {
    const int2 r = range[key];
    for (int p = r.x; p < r.y; ++p) {
        const float4 v = ps[p];
        const float dx = v.x - qx, dy = v.y - qy, dz = v.z - qz;
        const float d2 = dx * dx + dy * dy + dz * dz;
        offer(L, d2, __float_as_int(v.w));
    }
}

struct Walk {
    const float4* __restrict__ ps;
    const int2* __restrict__ range;
    const int32_t* __restrict__ coarse;
    Grid g;
    int shift, CY, CZ;
    int cx, cy, cz;
    float qx, qy, qz, margin;
};

// one coarse block, as ncw_nn.hip's visit_block with min(best, r2) -> min(kth, r2).  The skip of the fine cells already walked
// is load-bearing here: a second visit would enter the cell's points a second time.
__device__ __forceinline__ void visit_block(const Walk& w, int jx, int jy, int jz, float gxy, List& L) {
    const int DX = w.g.dim[0], DY = w.g.dim[1], DZ = w.g.dim[2];
    const int B = 1 << w.shift;
    const int z0 = jz << w.shift, z1 = min(z0 + B, DZ);
    if (gxy + axis_gap2(w.qz, w.g.lo[2], w.g.h, z0, z1, DZ, w.margin) > fminf(L.kd2, L.r2)) return;
    if (w.coarse[(jx * w.CY + jy) * w.CZ + jz] == 0) return;  // an empty block: one lookup
    const int x0 = jx << w.shift, x1 = min(x0 + B, DX);
    const int y0 = jy << w.shift, y1 = min(y0 + B, DY);
    for (int ix = x0; ix < x1; ++ix) {
        const float fx = axis_gap2(w.qx, w.g.lo[0], w.g.h, ix, ix + 1, DX, w.margin);
        if (fx > fminf(L.kd2, L.r2)) continue;
        const bool nx = abs(ix - w.cx) <= kFineShells;
        for (int iy = y0; iy < y1; ++iy) {
            const float fxy = fx + axis_gap2(w.qy, w.g.lo[1], w.g.h, iy, iy + 1, DY, w.margin);
            if (fxy > fminf(L.kd2, L.r2)) continue;
            const bool nxy = nx && abs(iy - w.cy) <= kFineShells;
            const int row = (ix * DY + iy) * DZ;
            for (int iz = z0; iz < z1; ++iz) {
                if (nxy && abs(iz - w.cz) <= kFineShells) continue;
                if (fxy + axis_gap2(w.qz, w.g.lo[2], w.g.h, iz, iz + 1, DZ, w.margin) > fminf(L.kd2, L.r2)) continue;
                scan_cell(w.range, w.ps, row + iz, w.qx, w.qy, w.qz, L);
            }
        }
    }
}

template <int WG>
__global__ __launch_bounds__(WG) void knn_query_kernel(const float4* __restrict__ ps, const int2* __restrict__ range,
                                                        const int32_t* __restrict__ coarse, int shift,
                                                        const float* __restrict__ q, const int64_t* __restrict__ q_order,
                                                        const int32_t* __restrict__ exclude, int64_t n, Grid g, float margin,
                                                        float r2, int k, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                        int32_t* __restrict__ count, int32_t* __restrict__ work) {
    extern __shared__ f32x2 knn_lds[];  // [k][WG] (d2, index bits)
    const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (t >= n) return;  // no barrier below: a lane owns its column of the list
    const int64_t j = q_order[t];
    const float qx = q[j * 3 + 0], qy = q[j * 3 + 1], qz = q[j * 3 + 2];
    const float inf = __int_as_float(0x7f800000);
    int32_t* orow = idx + j * k;
    float* drow = dist + j * k;
    const bool finite = fabsf(qx) < inf && fabsf(qy) < inf && fabsf(qz) < inf;  // false for a NaN too
    List L;
    L.lst = (lds_pair*)knn_lds + threadIdx.x;
    L.wg = WG; L.k = k; L.cnt = 0;
    L.excl = exclude ? exclude[j] : -1;
    L.r2 = r2; L.kd2 = inf; L.ki = 0x7fffffff;
    L.evals = 0; L.inserts = 0;
    if (finite) {
        const int cx = cell_of(qx, g.lo[0], g.inv_h, g.dim[0]);
        const int cy = cell_of(qy, g.lo[1], g.inv_h, g.dim[1]);
        const int cz = cell_of(qz, g.lo[2], g.inv_h, g.dim[2]);
        const int DX = g.dim[0], DY = g.dim[1], DZ = g.dim[2];
        const float qa[3] = {qx, qy, qz};
        bool done = false;
        for (int r = 0; r <= kFineShells; ++r) {
            const int x0 = max(cx - r, 0), x1 = min(cx + r, DX - 1);
            const int y0 = max(cy - r, 0), y1 = min(cy + r, DY - 1);
            const int z0 = max(cz - r, 0), z1 = min(cz + r, DZ - 1);
            for (int ix = x0; ix <= x1; ++ix) {
                const bool xs = ix == cx - r || ix == cx + r;
                for (int iy = y0; iy <= y1; ++iy) {
                    const int row = (ix * DY + iy) * DZ;
                    if (xs || iy == cy - r || iy == cy + r) {
                        for (int iz = z0; iz <= z1; ++iz) scan_cell(range, ps, row + iz, qx, qy, qz, L);
                    } else {
                        if (cz - r >= 0) scan_cell(range, ps, row + cz - r, qx, qy, qz, L);
                        if (r > 0 && cz + r <= DZ - 1) scan_cell(range, ps, row + cz + r, qx, qy, qz, L);
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
            if (!open) { done = true; break; }  // the block covers the whole grid
            const float bm = b - margin;
            if (bm > 0.f && fminf(L.kd2, r2) < bm * bm) { done = true; break; }  // against the k-th best, not the best
        }
        if (!done) {
            Walk w;
            w.ps = ps; w.range = range; w.coarse = coarse; w.g = g; w.shift = shift;
            w.cx = cx; w.cy = cy; w.cz = cz; w.qx = qx; w.qy = qy; w.qz = qz; w.margin = margin;
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
                    if (gx > fminf(L.kd2, r2)) continue;
                    for (int jy = y0; jy <= y1; ++jy) {
                        const float gxy = gx + axis_gap2(qy, g.lo[1], g.h, jy << shift, min((jy + 1) << shift, DY), DY, margin);
                        if (gxy > fminf(L.kd2, r2)) continue;
                        if (xs || jy == ba[1] - R || jy == ba[1] + R) {
                            for (int jz = z0; jz <= z1; ++jz) visit_block(w, jx, jy, jz, gxy, L);
                        } else {
                            if (ba[2] - R >= 0) visit_block(w, jx, jy, ba[2] - R, gxy, L);
                            if (R > 0 && ba[2] + R <= CZ - 1) visit_block(w, jx, jy, ba[2] + R, gxy, L);
                        }
                    }
                }
                float b = inf;
                bool open = false;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int f0 = max(ba[a] - R, 0) << shift;
                    const int f1 = min(ba[a] + R + 1, Ca[a]) << shift;
                    if (f0 > 0) { b = fminf(b, qa[a] - (g.lo[a] + (float)f0 * g.h)); open = true; }
                    if (f1 < g.dim[a]) { b = fminf(b, (g.lo[a] + (float)f1 * g.h) - qa[a]); open = true; }
                }
                if (!open) break;
                const float bm = b - margin;
                if (bm > 0.f && fminf(L.kd2, r2) < bm * bm) break;
            }
        }
    }
    for (int r = 0; r < k; ++r) {
        if (r < L.cnt) {
            const f32x2 u = L.lst[r * WG];
            orow[r] = __float_as_int(u.y);
            drow[r] = sqrtf(u.x);
        } else {
            orow[r] = -1;
            drow[r] = inf;
        }
    }
    count[j] = L.cnt;
    if (work) { work[j * 2 + 0] = L.evals; work[j * 2 + 1] = L.inserts; }
}

// ---- PCA of a neighbour list: float64, a fixed operation sequence (tests/_knn_ref.py: pca_ref) ----
constexpr int kJacobiSweeps = 8;

// one Jacobi rotation in the (p, q) plane of the symmetric matrix; app, aqq, apq its entries, arp / arq the two entries of the
// third row; v?p / v?q the two columns of the eigenvector matrix.  Skipped where the off-diagonal is exactly 0.
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                           double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = fabs(theta);
    const double tm = 1.0 / (at + sqrt(theta * theta + 1.0));
    const double t = theta < 0.0 ? -tm : tm;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double tap = t * apq;
    app = app - tap;
    aqq = aqq + tap;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    v0p = a0; v0q = b0;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    v1p = a1; v1q = b1;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v2p = a2; v2q = b2;
}

__global__ __launch_bounds__(256) void knn_pca_kernel(const float* __restrict__ pts, const float* __restrict__ ref, int64_t nref,
                                                       const int32_t* __restrict__ idx, const int32_t* __restrict__ count,
                                                       int64_t n, int k, int with_query, int has_toward, float tx, float ty,
                                                       float tz, float* __restrict__ normal, double* __restrict__ eig,
                                                       float* __restrict__ curvature, uint8_t* __restrict__ valid) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int cnt = min(max(count[j], 0), k);
    const int32_t* row = idx + j * k;
    for (int r = 0; r < cnt; ++r)
        if ((uint64_t)(int64_t)row[r] >= (uint64_t)nref) cnt = r;  // an index outside the cloud ends the list: nothing is read there
    const int m = cnt + (with_query ? 1 : 0);
    const double px = (double)pts[j * 3 + 0], py = (double)pts[j * 3 + 1], pz = (double)pts[j * 3 + 2];
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
    if (m > 0) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        if (with_query) { sx = sx + px; sy = sy + py; sz = sz + pz; }
        for (int r = 0; r < cnt; ++r) {
            const int64_t i = row[r];
            sx = sx + (double)ref[i * 3 + 0]; sy = sy + (double)ref[i * 3 + 1]; sz = sz + (double)ref[i * 3 + 2];
        }
        const double dn = (double)m;
        const double mx = sx / dn, my = sy / dn, mz = sz / dn;
        double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
        for (int r = (with_query ? -1 : 0); r < cnt; ++r) {
            double ax, ay, az;
            if (r < 0) { ax = px; ay = py; az = pz; }
            else {
                const int64_t i = row[r];
                ax = (double)ref[i * 3 + 0]; ay = (double)ref[i * 3 + 1]; az = (double)ref[i * 3 + 2];
            }
            const double dx = ax - mx, dy = ay - my, dz = az - mz;
            cxx = cxx + dx * dx; cxy = cxy + dx * dy; cxz = cxz + dx * dz;
            cyy = cyy + dy * dy; cyz = cyz + dy * dz; czz = czz + dz * dz;
        }
        double a00 = cxx / dn, a01 = cxy / dn, a02 = cxz / dn, a11 = cyy / dn, a12 = cyz / dn, a22 = czz / dn;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
        for (int s = 0; s < kJacobiSweeps; ++s) {
            jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1); third row 2
            jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2); third row 1
            jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2); third row 0
        }
        // ascending by three compare-swaps (strict: equal eigenvalues keep their column order)
        l0 = a00; l1 = a11; l2 = a22;
        double e0x = v00, e0y = v10, e0z = v20, e1x = v01, e1y = v11, e1z = v21, e2x = v02, e2y = v12, e2z = v22;
#define NCW_KNN_SWAP(la, lb, ax, ay, az, bx, by, bz) \
    if (lb < la) { double t_; t_ = la; la = lb; lb = t_; t_ = ax; ax = bx; bx = t_; t_ = ay; ay = by; by = t_; t_ = az; az = bz; bz = t_; }
        NCW_KNN_SWAP(l0, l1, e0x, e0y, e0z, e1x, e1y, e1z)
        NCW_KNN_SWAP(l1, l2, e1x, e1y, e1z, e2x, e2y, e2z)
        NCW_KNN_SWAP(l0, l1, e0x, e0y, e0z, e1x, e1y, e1z)
#undef NCW_KNN_SWAP
        const double len = sqrt(e0x * e0x + e0y * e0y + e0z * e0z);
        nx = e0x / len; ny = e0y / len; nz = e0z / len;
    }
    const bool ok = m >= 3 && l1 > 1e-10 * l2;
    if (ok) {
        bool flip;
        if (has_toward) {
            const double s = nx * ((double)tx - px) + ny * ((double)ty - py) + nz * ((double)tz - pz);
            flip = s < 0.0;
        } else {
            double big = nx;
            if (fabs(ny) > fabs(big)) big = ny;
            if (fabs(nz) > fabs(big)) big = nz;
            flip = big < 0.0;
        }
        if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    } else {
        nx = 0.0; ny = 0.0; nz = 0.0;
    }
    normal[j * 3 + 0] = (float)nx; normal[j * 3 + 1] = (float)ny; normal[j * 3 + 2] = (float)nz;
    eig[j * 3 + 0] = l0; eig[j * 3 + 1] = l1; eig[j * 3 + 2] = l2;
    const double sum = l0 + l1 + l2;
    curvature[j] = sum == 0.0 ? 0.f : (float)(l0 / sum);
    valid[j] = ok ? 1 : 0;
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

int block_shift(int B) {
    if (B < 1 || B > 65536 || (B & (B - 1)) != 0) return -1;
    int s = 0;
    while ((1 << s) < B) ++s;
    return s;
}

template <int WG>
int launch_query(const float* pts_sorted, const int32_t* cell_range, const int32_t* coarse, int shift, const float* q,
                 const int64_t* q_order, const int32_t* exclude, int64_t n, const NcwNnGrid* grid, float margin, float r2, int k,
                 int32_t* idx, float* dist, int32_t* count, int32_t* work, hipStream_t s) {
    const size_t lds = (size_t)k * WG * sizeof(f32x2);
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute((const void*)knn_query_kernel<WG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return NCW_E_BADARG;
    hipLaunchKernelGGL(knn_query_kernel<WG>, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), lds, s, (const float4*)pts_sorted,
                       (const int2*)cell_range, coarse, shift, q, q_order, exclude, n, to_grid(grid), margin, r2, k, idx, dist,
                       count, work);
    NCW_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int ncw_knn_query(const float* pts_sorted, const int32_t* cell_range, const int32_t* coarse, int B, const float* q,
                             const int64_t* q_order, const int32_t* exclude, int64_t n, const NcwNnGrid* grid, float margin,
                             float max_dist, int k, int wg, int32_t* idx, float* dist, int32_t* count, int32_t* work,
                             void* stream) {
    if (n <= 0) return 0;
    const int shift = block_shift(B);
    if (!pts_sorted || !cell_range || !coarse || !q || !q_order || !idx || !dist || !count || !grid_ok(grid) || shift < 0 ||
        !(margin >= 0.f) || !(max_dist > 0.f) || k < 1 || k > kMaxK || n > 0x7fffffffll / kMaxK)
        return NCW_E_BADARG;
    const float r2 = max_dist * max_dist;  // rounded once, here; +inf stays +inf
    hipStream_t s = (hipStream_t)stream;
    switch (wg) {
        case 0:
        case 64: return launch_query<64>(pts_sorted, cell_range, coarse, shift, q, q_order, exclude, n, grid, margin, r2, k, idx, dist, count, work, s);
        case 128: return launch_query<128>(pts_sorted, cell_range, coarse, shift, q, q_order, exclude, n, grid, margin, r2, k, idx, dist, count, work, s);
        case 256: return launch_query<256>(pts_sorted, cell_range, coarse, shift, q, q_order, exclude, n, grid, margin, r2, k, idx, dist, count, work, s);
        default: return NCW_E_BADARG;
    }
}

extern "C" int ncw_knn_pca(const float* pts, const float* ref, int64_t m, const int32_t* idx, const int32_t* count, int64_t n,
                           int k, int with_query, const float* toward, float* normal, double* eig, float* curvature,
                           uint8_t* valid, void* stream) {
    if (n <= 0) return 0;
    if (!pts || !ref || !idx || !count || !normal || !eig || !curvature || !valid || k < 1 || k > kMaxK || m < 0) return NCW_E_BADARG;
    hipLaunchKernelGGL(knn_pca_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pts, ref, m, idx, count, n,
                       k, with_query ? 1 : 0, toward ? 1 : 0, toward ? toward[0] : 0.f, toward ? toward[1] : 0.f,
                       toward ? toward[2] : 0.f, normal, eig, curvature, valid);
    NCW_CHECK_LAUNCH();
    return 0;
}
