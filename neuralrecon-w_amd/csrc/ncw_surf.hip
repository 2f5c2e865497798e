// Area-weighted sampling of a triangle mesh's surface on the GPU (mesh evaluation): what the open3d branch
// of the reference's evaluation does to a predicted MESH (utils/eval_utils.py:20-61, `o3d_load` with is_mesh): crop the
// triangles to the evaluation box (`TriangleMesh.crop`, :39) and draw 10 |GT| points uniformly by area
// (`sample_points_uniformly`, :42).  Neither open3d's crop rule nor its Mersenne-twister stream is pinned (its source is not
// at hand, and the reference does not seed it): the rule below follows open3d's documentation, the stream is our own.
//
//   ncw_surf_weights : one lane per triangle: 0.5 |(B - A) x (C - A)|, or exactly 0 for a triangle that must never be drawn
//                      (corner index out of range -- never read --, non-finite area, a corner outside the closed box);
//   (caller)         : cdf = inclusive prefix sum of the weights in float64 -- plumbing (torch.cumsum), like the sort of the
//                      1-NN grid;
//   ncw_surf_pick    : the binary search on its own (one lane per value);
//   ncw_surf_sample  : one lane per sample: Philox4x32-10 of (sample index, seed) -> (xi, r1, r2), triangle = search of
//                      u cdf[F-1], point = (1 - s) A + s (1 - r2) B + s r2 C with s = sqrt(r1) (open3d's formula).  The
//                      generator keeps no state, so any range [i0, i0 + n) of the N samples can be drawn by any launch.
//
// Everything is float64: GT coordinates are metres far from the origin and the triangles are millimetres, so f32 vertices
// would cost 1e-4 m.  No atomics, no reductions: every output is a function of its own index, bitwise reproducible.  The
// kernel is latency- and bandwidth-bound (about 21 dependent 8-byte loads of the search, three 24-byte gathers, 24-40 bytes
// written per sample); in stratified mode u grows with the lane index, so a wavefront's searches share their cache lines
// and its gathers hit neighbouring triangles.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_philox.h"  // philox4x32_10

// the products and sums below are rounded one by one (no fused multiply-add): the restatement in tests/_surf_ref.py is then
// the same arithmetic, and the result does not depend on what the compiler chooses to contract
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;

struct Box {
    int on;
    double lo[3], hi[3];
};

__device__ __forceinline__ bool in_box(const Box& b, double x, double y, double z) {
    return x >= b.lo[0] && x <= b.hi[0] && y >= b.lo[1] && y <= b.hi[1] && z >= b.lo[2] && z <= b.hi[2];  // NaN: outside
}

__global__ __launch_bounds__(kBlock) void surf_weights_kernel(const double* __restrict__ verts, int64_t n_verts,
                                                               const int32_t* __restrict__ faces, int64_t n_faces, Box box,
                                                               double* __restrict__ weight) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    const int64_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    double w = 0.0;
    if (a >= 0 && a < n_verts && b >= 0 && b < n_verts && c >= 0 && c < n_verts) {
        const double ax = verts[a * 3 + 0], ay = verts[a * 3 + 1], az = verts[a * 3 + 2];
        const double bx = verts[b * 3 + 0], by = verts[b * 3 + 1], bz = verts[b * 3 + 2];
        const double cx = verts[c * 3 + 0], cy = verts[c * 3 + 1], cz = verts[c * 3 + 2];
        const double ux = bx - ax, uy = by - ay, uz = bz - az;
        const double vx = cx - ax, vy = cy - ay, vz = cz - az;
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double area = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
        const bool keep = !box.on || (in_box(box, ax, ay, az) && in_box(box, bx, by, bz) && in_box(box, cx, cy, cz));
        if (keep && isfinite(area)) w = area;
    }
    weight[f] = w;
}

// The smallest k with cdf[k] > x; when there is none (x >= cdf[F-1]) the smallest k with cdf[k] == cdf[F-1], which is the
// last triangle of positive weight.  NaN or negative x counts as 0.  cdf is non-decreasing, F >= 1.
__device__ __forceinline__ int surf_pick(const double* __restrict__ cdf, int n_faces, double x) {
    if (!(x > 0.0)) x = 0.0;
    int lo = 0, hi = n_faces;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (cdf[mid] > x) hi = mid; else lo = mid + 1;
    }
    if (lo < n_faces) return lo;
    const double last = cdf[n_faces - 1];
    lo = 0;
    hi = n_faces - 1;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (cdf[mid] >= last) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void surf_pick_kernel(const double* __restrict__ cdf, int n_faces,
                                                            const double* __restrict__ x, int64_t n, int32_t* __restrict__ tri) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    tri[i] = surf_pick(cdf, n_faces, x[i]);
}

__global__ __launch_bounds__(kBlock) void surf_sample_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                              const double* __restrict__ cdf, int n_faces, uint32_t k0, uint32_t k1,
                                                              int64_t i0, int64_t n, int64_t n_total, int mode,
                                                              double* __restrict__ pts, int32_t* __restrict__ tri,
                                                              double* __restrict__ urr) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const uint64_t i = (uint64_t)i0 + (uint64_t)t;
    uint32_t w[4] = {(uint32_t)i, (uint32_t)(i >> 32), 0u, 0u};
    philox4x32_10(w, k0, k1);
    const double xi = (double)((((uint64_t)w[0] << 32) | (uint64_t)w[1]) >> 11) * 0x1p-53;
    const double r1 = ((double)w[2] + 0.5) * 0x1p-32;
    const double r2 = ((double)w[3] + 0.5) * 0x1p-32;
    const double u = mode == 1 ? ((double)i + xi) / (double)n_total : xi;
    const double total = cdf[n_faces - 1];
    if (!(total > 0.0)) {  // nothing to draw from: no triangle may be read
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
        for (int d = 0; d < 3; ++d) pts[t * 3 + d] = nan;
        if (tri) tri[t] = -1;
        if (urr) {
            urr[t * 3 + 0] = u;
            urr[t * 3 + 1] = r1;
            urr[t * 3 + 2] = r2;
        }
        return;
    }
    const int k = surf_pick(cdf, n_faces, u * total);
    const int64_t a = faces[(int64_t)k * 3 + 0], b = faces[(int64_t)k * 3 + 1], c = faces[(int64_t)k * 3 + 2];
    const double s = sqrt(r1);
    const double wa = 1.0 - s, wb = s * (1.0 - r2), wc = s * r2;
#pragma unroll
    for (int d = 0; d < 3; ++d) pts[t * 3 + d] = wa * verts[a * 3 + d] + wb * verts[b * 3 + d] + wc * verts[c * 3 + d];
    if (tri) tri[t] = k;
    if (urr) {
        urr[t * 3 + 0] = u;
        urr[t * 3 + 1] = r1;
        urr[t * 3 + 2] = r2;
    }
}

constexpr int64_t kMaxFaces = 0x7fffffffll;
constexpr int64_t kMaxLaunch = (int64_t)0x7fffffffll * kBlock;  // lanes of one launch (grid.x < 2^31)

}  // namespace

extern "C" int ncw_surf_weights(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const double* box,
                                double* weight, void* stream) {
    if (n_faces <= 0) return 0;
    if (!faces || !weight || n_verts < 0 || (n_verts > 0 && !verts) || n_faces > kMaxFaces) return NCW_E_BADARG;
    Box b;
    b.on = box != nullptr;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = box ? box[a] : 0.0;
        b.hi[a] = box ? box[3 + a] : 0.0;
    }
    hipLaunchKernelGGL(surf_weights_kernel, dim3((unsigned)((n_faces + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, verts, n_verts, faces, n_faces, b, weight);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_surf_pick(const double* cdf, int64_t n_faces, const double* x, int64_t n, int32_t* tri, void* stream) {
    if (n <= 0) return 0;
    if (!cdf || !x || !tri || n_faces < 1 || n_faces > kMaxFaces || n > kMaxLaunch) return NCW_E_BADARG;
    hipLaunchKernelGGL(surf_pick_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, cdf,
                       (int)n_faces, x, n, tri);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_surf_sample(const double* verts, const int32_t* faces, const double* cdf, int64_t n_faces, uint64_t seed,
                               int64_t i0, int64_t n, int64_t n_total, int mode, double* pts, int32_t* tri, double* urr,
                               void* stream) {
    if (n <= 0) return 0;
    if (!verts || !faces || !cdf || !pts || n_faces < 1 || n_faces > kMaxFaces || n > kMaxLaunch || i0 < 0 ||
        (mode != 0 && mode != 1) || (mode == 1 && (n_total < 1 || i0 > n_total - n)))
        return NCW_E_BADARG;
    hipLaunchKernelGGL(surf_sample_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, verts,
                       faces, cdf, (int)n_faces, (uint32_t)seed, (uint32_t)(seed >> 32), i0, n, n_total, mode, pts, tri, urr);
    NCW_CHECK_LAUNCH();
    return 0;
}
