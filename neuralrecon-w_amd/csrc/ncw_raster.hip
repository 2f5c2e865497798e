// Triangle depth rasterizer for the reprojection visibility filter: replaces the pyrender / OpenGL depth
// render of utils/pyrender_renderer.py:16-24 (called from utils/reproj_filter.py:208) and the per-pixel back-projection
// of utils/reproj_filter.py:133-152 (`reproject`), plus the marking of :229-232.
//
// One view of an indexed triangle mesh, linear eye-space depth, deterministic:
//   ncw_raster_small      : one lane per face: transform by the 3x4 view, drop faces with an out-of-range index, faces
//                           entirely in front of znear or entirely beyond zfar; clip to the near plane (0, 1 or 2
//                           sub-triangles, as OpenGL); project (pixel (r, c) samples the image point (c + 0.5, r + 0.5));
//                           drop degenerate (zero signed area) and, with cull, back-facing sub-triangles (signed area > 0
//                           in pixel coordinates, x right, y down); then rasterize in the lane when the pixel bounding box
//                           holds at most `small_max` samples, else append (face, sub-triangle) to the large list;
//   ncw_raster_large      : one workgroup per large-list entry (grid-stride over the list), the threads stride over the
//                           bounding box -- no lane ever walks a big triangle alone;
//   ncw_raster_resolve    : per pixel depth (f32, 0 = empty) and, optionally, the winning face (-1 = empty);
//   ncw_raster_backproject: the listed pixels p = M[:, :3] (c d, r d, d) + M[:, 3] (INTEGER pixel coordinates, the reference's
//                           own half-pixel offset against the sample);
//   ncw_raster_mark       : flags[idx[i]] = 1 where dist[i] < thr (the 1-NN result of the back-projected points).
// Coverage: a sample is covered when all three edge functions are >= 0 (inclusive on every edge).  Each edge function is
// evaluated with its two endpoints in a canonical order and negated for the other direction, and contraction is off, so
// the two faces on a shared edge see bitwise opposite values: a sample on the edge is covered by both, never by neither.
// Depth: perspective-correct, 1/z interpolated with the screen barycentrics; samples with z > zfar (or z < znear after the
// clip's rounding) are dropped.  The z-buffer is a 64-bit atomicMin of (float bits of z << 32 | face id): positive floats
// order like their bits, so the nearest sample wins and equal depths go to the smaller face id, whatever the launch order.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kLargeBlocks = 1024;  // grid of the large-triangle kernel (grid-stride over the device-side list)

struct View {
    float m[12];  // camera = m[:, :3] v + m[:, 3], row-major 3x4
    float fx, fy, cx, cy, znear, zfar;
    int h, w, cull, small_max;
};

struct Tri {
    float x0, y0, x1, y1, x2, y2;  // pixel coordinates, wound so that the covered side is >= 0
    float iz0, iz1, iz2;           // 1 / z
    int c0, c1, r0, r1;            // inclusive sample box, clipped to the image (empty when c0 > c1 or r0 > r1)
};

struct Vc {
    float x, y, z;
};

__device__ __forceinline__ Vc to_cam(const float* __restrict__ verts, int64_t i, const View& v) {
#pragma clang fp contract(off)
    const float px = verts[i * 3 + 0], py = verts[i * 3 + 1], pz = verts[i * 3 + 2];
    Vc o;
    o.x = v.m[0] * px + v.m[1] * py + v.m[2] * pz + v.m[3];
    o.y = v.m[4] * px + v.m[5] * py + v.m[6] * pz + v.m[7];
    o.z = v.m[8] * px + v.m[9] * py + v.m[10] * pz + v.m[11];
    return o;
}

// the point of segment (out -> in) on z = znear; the parameter always runs from the vertex in front of the near plane,
// so the two faces on a clipped edge produce the same vertex bit for bit
__device__ __forceinline__ Vc clip_near(Vc out, Vc in, float znear) {
#pragma clang fp contract(off)
    const float t = (znear - out.z) / (in.z - out.z);
    Vc o;
    o.x = out.x + t * (in.x - out.x);
    o.y = out.y + t * (in.y - out.y);
    o.z = znear;
    return o;
}

// edge function of (a -> b) at p, antisymmetric bit for bit: e(a, b, p) == -e(b, a, p)
__device__ __forceinline__ float edge_fn(float ax, float ay, float bx, float by, float px, float py) {
#pragma clang fp contract(off)
    const bool sw = bx < ax || (bx == ax && by < ay);
    const float x0 = sw ? bx : ax, y0 = sw ? by : ay, x1 = sw ? ax : bx, y1 = sw ? ay : by;
    const float e = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0);
    return sw ? -e : e;
}

// samples k + 0.5 inside [lo_f, hi_f]: k in [ceil(lo_f - 0.5), floor(hi_f - 0.5)], clipped to [0, n - 1]; returns the last
__device__ __forceinline__ int clamp_box(float lo_f, float hi_f, int n, int& lo) {
    const float a = fminf(fmaxf(ceilf(lo_f - 0.5f), 0.f), (float)n);
    const float b = fminf(fmaxf(floorf(hi_f - 0.5f), -1.f), (float)(n - 1));
    lo = (int)a;
    return (int)b;
}

// projects one (clipped) sub-triangle; false when it is degenerate, culled or covers no sample of the image
__device__ __forceinline__ bool make_tri(Vc a, Vc b, Vc c, const View& v, Tri& t) {
#pragma clang fp contract(off)
    const float x0 = v.fx * (a.x / a.z) + v.cx, y0 = v.fy * (a.y / a.z) + v.cy;
    float x1 = v.fx * (b.x / b.z) + v.cx, y1 = v.fy * (b.y / b.z) + v.cy;
    float x2 = v.fx * (c.x / c.z) + v.cx, y2 = v.fy * (c.y / c.z) + v.cy;
    const float iz0 = 1.f / a.z;
    float iz1 = 1.f / b.z, iz2 = 1.f / c.z;
    const float area = edge_fn(x0, y0, x1, y1, x2, y2);  // twice the signed area: < 0 = front facing
    if (!(area != 0.f) || !isfinite(area)) return false;  // degenerate (or not finite)
    if (area > 0.f) {
        if (v.cull) return false;  // back face
    } else {  // wind front faces the other way round so that the covered side is >= 0 for every triangle
        float s = x1; x1 = x2; x2 = s;
        s = y1; y1 = y2; y2 = s;
        s = iz1; iz1 = iz2; iz2 = s;
    }
    t.x0 = x0; t.y0 = y0; t.x1 = x1; t.y1 = y1; t.x2 = x2; t.y2 = y2;
    t.iz0 = iz0; t.iz1 = iz1; t.iz2 = iz2;
    t.c1 = clamp_box(fminf(x0, fminf(x1, x2)), fmaxf(x0, fmaxf(x1, x2)), v.w, t.c0);
    t.r1 = clamp_box(fminf(y0, fminf(y1, y2)), fmaxf(y0, fmaxf(y1, y2)), v.h, t.r0);
    return t.c0 <= t.c1 && t.r0 <= t.r1;
}

// sub-triangle `sub` (0 / 1) of face f after the near clip; n_sub = how many the face has (0, 1 or 2); false when that
// sub-triangle does not exist or is dropped
__device__ __forceinline__ bool face_tri(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces,
                                         int64_t f, int sub, const View& v, Tri& t, int& n_sub) {
    n_sub = 0;
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_verts || i1 >= n_verts || i2 >= n_verts) return false;
    const Vc p0 = to_cam(verts, i0, v), p1 = to_cam(verts, i1, v), p2 = to_cam(verts, i2, v);
    if (!(isfinite(p0.z) && isfinite(p1.z) && isfinite(p2.z))) return false;
    const bool in0 = p0.z >= v.znear, in1 = p1.z >= v.znear, in2 = p2.z >= v.znear;
    const int n_in = (int)in0 + (int)in1 + (int)in2;
    if (n_in == 0) return false;
    if (p0.z > v.zfar && p1.z > v.zfar && p2.z > v.zfar) return false;
    if (n_in == 3) {
        n_sub = 1;
        return sub == 0 && make_tri(p0, p1, p2, v, t);
    }
    // rotate the cyclic order (a, b, c) to start at the odd vertex out (the one in front for n_in == 1, the one behind the
    // near plane for n_in == 2); the winding is kept
    const int k = n_in == 1 ? (in0 ? 0 : in1 ? 1 : 2) : (!in0 ? 0 : !in1 ? 1 : 2);
    const Vc a = k == 0 ? p0 : k == 1 ? p1 : p2;
    const Vc b = k == 0 ? p1 : k == 1 ? p2 : p0;
    const Vc c = k == 0 ? p2 : k == 1 ? p0 : p1;
    if (n_in == 1) {  // a in front: (a, ab, ac)
        n_sub = 1;
        return sub == 0 && make_tri(a, clip_near(b, a, v.znear), clip_near(c, a, v.znear), v, t);
    }
    // a behind, b and c in front: the quad (b, c, ca, ab) as (b, c, ca) + (b, ca, ab)
    n_sub = 2;
    const Vc ab = clip_near(a, b, v.znear), ca = clip_near(a, c, v.znear);
    return sub == 0 ? make_tri(b, c, ca, v, t) : make_tri(b, ca, ab, v, t);
}

__device__ __forceinline__ void shade(const Tri& t, int r, int c, uint32_t face, const View& v,
                                      unsigned long long* __restrict__ zbuf) {
#pragma clang fp contract(off)
    const float px = (float)c + 0.5f, py = (float)r + 0.5f;
    const float e0 = edge_fn(t.x1, t.y1, t.x2, t.y2, px, py);  // opposite vertex 0
    const float e1 = edge_fn(t.x2, t.y2, t.x0, t.y0, px, py);
    const float e2 = edge_fn(t.x0, t.y0, t.x1, t.y1, px, py);
    if (e0 < 0.f || e1 < 0.f || e2 < 0.f) return;
    const float den = e0 * t.iz0 + e1 * t.iz1 + e2 * t.iz2;
    const float z = (e0 + e1 + e2) / den;
    if (!(den > 0.f) || !(z >= v.znear) || !(z <= v.zfar)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)face;
    unsigned long long* dst = zbuf + (int64_t)r * v.w + c;
    if (key < *dst) atomicMin(dst, key);  // early-z: the stored key only ever decreases
}

__global__ __launch_bounds__(kBlock) void raster_small_kernel(const float* __restrict__ verts, int64_t n_verts,
                                                              const int32_t* __restrict__ faces, int64_t n_faces, View v,
                                                              unsigned long long* __restrict__ zbuf, int32_t* __restrict__ large,
                                                              int32_t* __restrict__ n_large) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    int n_sub = 1;
    for (int sub = 0; sub < n_sub; ++sub) {
        Tri t;
        if (!face_tri(verts, n_verts, faces, f, sub, v, t, n_sub)) continue;
        const int64_t cnt = (int64_t)(t.c1 - t.c0 + 1) * (int64_t)(t.r1 - t.r0 + 1);
        if (cnt > v.small_max) {
            large[atomicAdd(n_large, 1)] = (int32_t)(f * 2 + sub);  // capacity 2 n_faces: every sub-triangle fits
            continue;
        }
        for (int r = t.r0; r <= t.r1; ++r)
            for (int c = t.c0; c <= t.c1; ++c) shade(t, r, c, (uint32_t)f, v, zbuf);
    }
}

__global__ __launch_bounds__(kBlock) void raster_large_kernel(const float* __restrict__ verts, int64_t n_verts,
                                                              const int32_t* __restrict__ faces, View v,
                                                              const int32_t* __restrict__ large,
                                                              const int32_t* __restrict__ n_large, int64_t max_large,
                                                              unsigned long long* __restrict__ zbuf) {
    const int64_t n = min((int64_t)*n_large, max_large);
    for (int64_t e = blockIdx.x; e < n; e += gridDim.x) {
        const int32_t item = large[e];
        const int64_t f = item >> 1;
        Tri t;
        int n_sub;
        // every thread sets the triangle up from the same inputs (uniform loads), bit-identical to the small path's setup
        if (!face_tri(verts, n_verts, faces, f, item & 1, v, t, n_sub)) continue;
        const int bw = t.c1 - t.c0 + 1;
        const int cnt = bw * (t.r1 - t.r0 + 1);  // <= height * width < 2^31
        for (int k = threadIdx.x; k < cnt; k += kBlock) shade(t, t.r0 + k / bw, t.c0 + k % bw, (uint32_t)f, v, zbuf);
    }
}

__global__ __launch_bounds__(kBlock) void raster_resolve_kernel(const unsigned long long* __restrict__ zbuf, int64_t n_pix,
                                                                float* __restrict__ depth, int32_t* __restrict__ face) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pix) return;
    const unsigned long long k = zbuf[p];
    const bool hit = k != ~0ull;
    depth[p] = hit ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
    if (face) face[p] = hit ? (int32_t)(unsigned)(k & 0xffffffffull) : -1;
}

struct Mat34 {
    float m[12];
};

__global__ __launch_bounds__(kBlock) void raster_backproject_kernel(const float* __restrict__ depth,
                                                                    const int64_t* __restrict__ pix, int64_t n, int w, Mat34 M,
                                                                    float* __restrict__ pts) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pix[i];
    const float d = depth[p];
    const float X = (float)(p % w) * d, Y = (float)(p / w) * d;
    pts[i * 3 + 0] = M.m[0] * X + M.m[1] * Y + M.m[2] * d + M.m[3];
    pts[i * 3 + 1] = M.m[4] * X + M.m[5] * Y + M.m[6] * d + M.m[7];
    pts[i * 3 + 2] = M.m[8] * X + M.m[9] * Y + M.m[10] * d + M.m[11];
}

__global__ __launch_bounds__(kBlock) void raster_mark_kernel(const float* __restrict__ dist, const int64_t* __restrict__ idx,
                                                             int64_t n, float thr, int64_t m, uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t j = idx[i];
    if (dist[i] < thr && j >= 0 && j < m) flags[j] = 1;
}

bool view_ok(const NcwRasterView* r) {
    return r && r->height > 0 && r->width > 0 && (int64_t)r->height * r->width < ((int64_t)1 << 31) && r->fx > 0.f &&
           r->fy > 0.f && r->znear > 0.f && r->zfar > r->znear && r->small_max >= 0 && (r->cull == 0 || r->cull == 1);
}

View to_view(const NcwRasterView* r) {
    View v;
    for (int i = 0; i < 12; ++i) v.m[i] = r->view[i];
    v.fx = r->fx; v.fy = r->fy; v.cx = r->cx; v.cy = r->cy;
    v.znear = r->znear; v.zfar = r->zfar;
    v.h = r->height; v.w = r->width; v.cull = r->cull; v.small_max = r->small_max;
    return v;
}

}  // namespace

extern "C" int ncw_raster_small(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                const NcwRasterView* view, uint64_t* zbuf, int32_t* large, int32_t* n_large, void* stream) {
    if (n_faces <= 0) return 0;
    if (!verts || !faces || !zbuf || !large || !n_large || !view_ok(view) || n_verts <= 0 || n_faces > 0x3fffffffll)
        return NCW_E_BADARG;
    hipLaunchKernelGGL(raster_small_kernel, dim3((unsigned)((n_faces + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, verts, n_verts, faces, n_faces, to_view(view), (unsigned long long*)zbuf, large,
                       n_large);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_raster_large(const float* verts, int64_t n_verts, const int32_t* faces, const NcwRasterView* view,
                                const int32_t* large, const int32_t* n_large, int64_t max_large, uint64_t* zbuf, void* stream) {
    if (max_large <= 0) return 0;
    if (!verts || !faces || !zbuf || !large || !n_large || !view_ok(view) || n_verts <= 0) return NCW_E_BADARG;
    hipLaunchKernelGGL(raster_large_kernel, dim3(kLargeBlocks), dim3(kBlock), 0, (hipStream_t)stream, verts, n_verts, faces,
                       to_view(view), large, n_large, max_large, (unsigned long long*)zbuf);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_raster_resolve(const uint64_t* zbuf, int64_t n_pix, float* depth, int32_t* face, void* stream) {
    if (n_pix <= 0) return 0;
    if (!zbuf || !depth) return NCW_E_BADARG;
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)((n_pix + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, (const unsigned long long*)zbuf, n_pix, depth, face);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_raster_backproject(const float* depth, const int64_t* pix, int64_t n, int32_t width, const float* M,
                                      float* pts, void* stream) {
    if (n <= 0) return 0;
    if (!depth || !pix || !M || !pts || width <= 0) return NCW_E_BADARG;
    Mat34 m;
    for (int i = 0; i < 12; ++i) m.m[i] = M[i];
    hipLaunchKernelGGL(raster_backproject_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, depth, pix, n, (int)width, m, pts);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_raster_mark(const float* dist, const int64_t* idx, int64_t n, float thr, int64_t m, uint8_t* flags,
                               void* stream) {
    if (n <= 0) return 0;
    if (!dist || !idx || !flags || m <= 0) return NCW_E_BADARG;
    hipLaunchKernelGGL(raster_mark_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       dist, idx, n, thr, m, flags);
    NCW_CHECK_LAUNCH();
    return 0;
}
