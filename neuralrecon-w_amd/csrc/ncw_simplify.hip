// Mesh simplification on the GPU: uniform-grid vertex clustering with a quadric-optimal representative per cell (Lindstrom's
// out-of-core simplification), meshops.simplify.  The reference has no such mode (it leaves decimation to an external tool);
// the contract -- participation, grid, cluster numbering, summation orders, the regularised solve and its fall-back to the
// member mean, the face rule -- is stated once in include/neuconw_hip.h and restated in numpy by tests/_simplify_ref.py.
//
//   ncw_mesh_sc_keys  : one lane per vertex: the int64 cell key of a used vertex, -1 for an unused one;
//   (caller)          : the distinct keys in ascending order number the clusters (torch.unique); cluster [V] int32;
//   ncw_mesh_sc_faces : one lane per face: the rotated cluster triple, the survive flag and, per corner, the cluster the face
//                       contributes its quadric to (-1 where the corner's cluster repeats an earlier corner's);
//   (caller)          : CSR lists per cluster by stable sorts (torch.sort): members (used vertices, ascending v) and incident
//                       faces (ascending f) -- plumbing;
//   ncw_mesh_sc_place : one lane per cluster: walks its member list (mean, colour sums), then its incidence list (quadric),
//                       solves, tests, writes centre + p and the placed-at-the-mean flag.  SEQUENTIAL PER-LANE ACCUMULATION IS
//                       THE CONTRACT: the sums run in list order, one lane, no atomics, so the result is a function of the
//                       mesh and the same bits on every run.
//
// No float atomics, no LDS, no cross-lane traffic.  Every index read from a list is range-checked before it is used.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

// every product and sum is rounded on its own (no fused multiply-add): the numpy restatement is then the same arithmetic
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxCount = 0x7fffffffll;
constexpr int64_t kMaxCells = 1ll << 62;

struct ScGrid {
    double lo[3];
    double h;
    int64_t n[3];
};

__device__ __forceinline__ bool face_valid(int a, int b, int c, int n_verts) {
    const unsigned v = (unsigned)n_verts;  // negative indices wrap above 2^31 > V
    return (unsigned)a < v && (unsigned)b < v && (unsigned)c < v && a != b && b != c && a != c;
}

// clamp(floor((x - lo) / h), 0, n - 1): a division, not a product with 1 / h (a coordinate with x - lo = k h lands in cell k)
__device__ __forceinline__ int64_t cell_of(double x, double lo, double h, int64_t n) {
    const double c = floor((x - lo) / h);
    if (!(c > 0.0)) return 0;  // NaN: cell 0
    if (c >= 4611686018427387904.0) return n - 1;  // 2^62 > any n
    const int64_t i = (int64_t)c;
    return i > n - 1 ? n - 1 : i;
}

__global__ __launch_bounds__(kBlock) void sc_keys_kernel(const double* __restrict__ verts, const uint8_t* __restrict__ used,
                                                         int n_verts, ScGrid g, int64_t* __restrict__ keys) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n_verts) return;
    int64_t key = -1;
    if (used[v]) {
        const int64_t ix = cell_of(verts[v * 3 + 0], g.lo[0], g.h, g.n[0]);
        const int64_t iy = cell_of(verts[v * 3 + 1], g.lo[1], g.h, g.n[1]);
        const int64_t iz = cell_of(verts[v * 3 + 2], g.lo[2], g.h, g.n[2]);
        key = (ix * g.n[1] + iy) * g.n[2] + iz;
    }
    keys[v] = key;
}

__global__ __launch_bounds__(kBlock) void sc_faces_kernel(const int32_t* __restrict__ faces, int n_faces, int n_verts,
                                                          const int32_t* __restrict__ cluster, int n_clusters,
                                                          int32_t* __restrict__ tri, uint8_t* __restrict__ survive,
                                                          int32_t* __restrict__ inc) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    int t0 = -1, t1 = -1, t2 = -1, i0 = -1, i1 = -1, i2 = -1;
    bool s = false;
    if (face_valid(a, b, c, n_verts)) {
        const int ca = cluster[a], cb = cluster[b], cc = cluster[c];
        const unsigned nc = (unsigned)n_clusters;
        if ((unsigned)ca < nc && (unsigned)cb < nc && (unsigned)cc < nc) {  // always, for the cluster map of this mesh
            i0 = ca;
            i1 = cb != ca ? cb : -1;
            i2 = (cc != ca && cc != cb) ? cc : -1;
            s = ca != cb && cb != cc && ca != cc;
            if (s) {  // rotated, not reflected: the smallest cluster first
                if (ca < cb && ca < cc) {
                    t0 = ca, t1 = cb, t2 = cc;
                } else if (cb < cc) {
                    t0 = cb, t1 = cc, t2 = ca;
                } else {
                    t0 = cc, t1 = ca, t2 = cb;
                }
            }
        }
    }
    tri[f * 3 + 0] = t0;
    tri[f * 3 + 1] = t1;
    tri[f * 3 + 2] = t2;
    inc[f * 3 + 0] = i0;
    inc[f * 3 + 1] = i1;
    inc[f * 3 + 2] = i2;
    survive[f] = s ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void sc_place_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                          int n_verts, int n_faces, const int64_t* __restrict__ keys,
                                                          int n_clusters, const int64_t* __restrict__ mem_off,
                                                          const int32_t* __restrict__ mem, int64_t n_mem,
                                                          const int64_t* __restrict__ inc_off, const int32_t* __restrict__ inc,
                                                          int64_t n_inc, ScGrid g, double eps, const uint8_t* __restrict__ colors,
                                                          double* __restrict__ out_verts, uint8_t* __restrict__ at_mean,
                                                          uint8_t* __restrict__ out_colors) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_clusters) return;
    // cell centre c = lo + (i + 0.5) h from the key
    int64_t key = keys[k];
    if (key < 0) key = 0;
    const int64_t iz = key % g.n[2];
    const int64_t r = key / g.n[2];
    const int64_t iy = r % g.n[1];
    const int64_t ix = r / g.n[1];
    const double cx = g.lo[0] + ((double)ix + 0.5) * g.h;
    const double cy = g.lo[1] + ((double)iy + 0.5) * g.h;
    const double cz = g.lo[2] + ((double)iz + 0.5) * g.h;

    // member mean, ascending v; colour sums (integers: exact in any order)
    int64_t m0 = mem_off[k], m1 = mem_off[k + 1];
    if (m0 < 0) m0 = 0;
    if (m1 > n_mem) m1 = n_mem;
    double mx = 0.0, my = 0.0, mz = 0.0;
    int64_t cnt = 0, sr = 0, sg = 0, sb = 0;
    for (int64_t j = m0; j < m1; ++j) {
        const int v = mem[j];
        if ((unsigned)v >= (unsigned)n_verts) continue;
        mx = mx + (verts[(int64_t)v * 3 + 0] - cx);
        my = my + (verts[(int64_t)v * 3 + 1] - cy);
        mz = mz + (verts[(int64_t)v * 3 + 2] - cz);
        if (colors) {
            sr += colors[(int64_t)v * 3 + 0];
            sg += colors[(int64_t)v * 3 + 1];
            sb += colors[(int64_t)v * 3 + 2];
        }
        ++cnt;
    }
    if (cnt > 0) {
        const double n = (double)cnt;
        mx = mx / n;
        my = my / n;
        mz = mz / n;
    }
    if (colors && out_colors) {  // floor(sum / count + 0.5) in integers
        const int64_t d = cnt > 0 ? cnt : 1;
        out_colors[k * 3 + 0] = (uint8_t)((2 * sr + d) / (2 * d));
        out_colors[k * 3 + 1] = (uint8_t)((2 * sg + d) / (2 * d));
        out_colors[k * 3 + 2] = (uint8_t)((2 * sb + d) / (2 * d));
    }

    // quadric, ascending face
    int64_t q0 = inc_off[k], q1 = inc_off[k + 1];
    if (q0 < 0) q0 = 0;
    if (q1 > n_inc) q1 = n_inc;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int64_t j = q0; j < q1; ++j) {
        const int f = inc[j];
        if ((unsigned)f >= (unsigned)n_faces) continue;
        const int va = faces[(int64_t)f * 3 + 0], vb = faces[(int64_t)f * 3 + 1], vc = faces[(int64_t)f * 3 + 2];
        if (!face_valid(va, vb, vc, n_verts)) continue;
        const double p0x = verts[(int64_t)va * 3 + 0] - cx, p0y = verts[(int64_t)va * 3 + 1] - cy, p0z = verts[(int64_t)va * 3 + 2] - cz;
        const double p1x = verts[(int64_t)vb * 3 + 0] - cx, p1y = verts[(int64_t)vb * 3 + 1] - cy, p1z = verts[(int64_t)vb * 3 + 2] - cz;
        const double p2x = verts[(int64_t)vc * 3 + 0] - cx, p2y = verts[(int64_t)vc * 3 + 1] - cy, p2z = verts[(int64_t)vc * 3 + 2] - cz;
        const double ux = p1x - p0x, uy = p1y - p0y, uz = p1z - p0z;
        const double wx = p2x - p0x, wy = p2y - p0y, wz = p2z - p0z;
        const double nx = uy * wz - uz * wy;
        const double ny = uz * wx - ux * wz;
        const double nz = ux * wy - uy * wx;
        const double d = (nx * p0x + ny * p0y) + nz * p0z;
        a00 = a00 + nx * nx;
        a01 = a01 + nx * ny;
        a02 = a02 + nx * nz;
        a11 = a11 + ny * ny;
        a12 = a12 + ny * nz;
        a22 = a22 + nz * nz;
        b0 = b0 + d * nx;
        b1 = b1 + d * ny;
        b2 = b2 + d * nz;
    }

    // placement
    double px = mx, py = my, pz = mz;
    bool mean = true;
    const double t = (a00 + a11) + a22;
    if (t != 0.0) {
        const double lam = (eps * t) / 3.0;
        const double M00 = a00 + lam, M11 = a11 + lam, M22 = a22 + lam, M01 = a01, M02 = a02, M12 = a12;
        const double r0 = b0 + lam * mx, r1 = b1 + lam * my, r2 = b2 + lam * mz;
        const double c00 = M11 * M22 - M12 * M12;
        const double c01 = M02 * M12 - M01 * M22;
        const double c02 = M01 * M12 - M02 * M11;
        const double c11 = M00 * M22 - M02 * M02;
        const double c12 = M01 * M02 - M00 * M12;
        const double c22 = M00 * M11 - M01 * M01;
        const double det = (M00 * c00 + M01 * c01) + M02 * c02;
        if (det > 0.0 && det < __longlong_as_double(0x7ff0000000000000ll)) {
            const double qx = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
            const double qy = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
            const double qz = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
            const double half = g.h / 2.0;
            if (fabs(qx) <= half && fabs(qy) <= half && fabs(qz) <= half) {  // false for NaN
                px = qx, py = qy, pz = qz;
                mean = false;
            }
        }
    }
    out_verts[k * 3 + 0] = cx + px;
    out_verts[k * 3 + 1] = cy + py;
    out_verts[k * 3 + 2] = cz + pz;
    at_mean[k] = mean ? 1 : 0;
}

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// h finite and > 0, lo finite, n >= 1 per axis and n_x n_y n_z < 2^62 (no overflow on the way: each factor is tested first)
inline bool grid_ok(const double* lo, double h, const int64_t* n, ScGrid* g) {
    if (!lo || !n || !(h > 0.0) || !__builtin_isfinite(h)) return false;
    for (int a = 0; a < 3; ++a) {
        if (!__builtin_isfinite(lo[a]) || n[a] < 1 || n[a] >= kMaxCells) return false;
        g->lo[a] = lo[a];
        g->n[a] = n[a];
    }
    if (n[0] > (kMaxCells - 1) / n[1]) return false;
    if (n[0] * n[1] > (kMaxCells - 1) / n[2]) return false;
    g->h = h;
    return true;
}

}  // namespace

extern "C" int ncw_mesh_sc_keys(const double* verts, const uint8_t* used, int64_t n_verts, const double* lo, double h,
                                const int64_t* n, int64_t* keys, void* stream) {
    ScGrid g;
    if (n_verts < 0 || n_verts > kMaxCount || !grid_ok(lo, h, n, &g)) return NCW_E_BADARG;
    if (n_verts == 0) return 0;
    if (!verts || !used || !keys) return NCW_E_BADARG;
    hipLaunchKernelGGL(sc_keys_kernel, grid_for(n_verts), dim3(kBlock), 0, (hipStream_t)stream, verts, used, (int)n_verts, g, keys);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mesh_sc_faces(const int32_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* cluster,
                                 int64_t n_clusters, int32_t* tri, uint8_t* survive, int32_t* inc, void* stream) {
    if (n_faces < 0 || n_faces > kMaxCount || n_verts < 0 || n_verts > kMaxCount || n_clusters < 0 || n_clusters > n_verts)
        return NCW_E_BADARG;
    if (n_faces == 0) return 0;
    if (!faces || !cluster || !tri || !survive || !inc) return NCW_E_BADARG;
    hipLaunchKernelGGL(sc_faces_kernel, grid_for(n_faces), dim3(kBlock), 0, (hipStream_t)stream, faces, (int)n_faces, (int)n_verts,
                       cluster, (int)n_clusters, tri, survive, inc);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mesh_sc_place(const double* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const int64_t* keys,
                                 int64_t n_clusters, const int64_t* mem_off, const int32_t* mem, int64_t n_mem,
                                 const int64_t* inc_off, const int32_t* inc, int64_t n_inc, const double* lo, double h,
                                 const int64_t* n, double eps, const uint8_t* colors, double* out_verts, uint8_t* at_mean,
                                 uint8_t* out_colors, void* stream) {
    ScGrid g;
    if (n_faces < 0 || n_faces > kMaxCount || n_verts < 0 || n_verts > kMaxCount || n_clusters < 0 || n_clusters > n_verts ||
        n_mem < 0 || n_mem > n_verts || n_inc < 0 || n_inc > 3 * n_faces || !grid_ok(lo, h, n, &g) || !(eps >= 0.0) ||
        !__builtin_isfinite(eps) || (colors != nullptr) != (out_colors != nullptr))
        return NCW_E_BADARG;
    if (n_clusters == 0) return 0;
    if (!verts || !faces || !keys || !mem_off || !mem || !inc_off || !out_verts || !at_mean || (n_inc > 0 && !inc))
        return NCW_E_BADARG;
    hipLaunchKernelGGL(sc_place_kernel, grid_for(n_clusters), dim3(kBlock), 0, (hipStream_t)stream, verts, faces, (int)n_verts,
                       (int)n_faces, keys, (int)n_clusters, mem_off, mem, n_mem, inc_off, inc, n_inc, g, eps, colors, out_verts,
                       at_mean, out_colors);
    NCW_CHECK_LAUNCH();
    return 0;
}
