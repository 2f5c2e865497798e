// Ground-truth reprojection error of SfM tracks (include/neuconw_hip.h, "Checking the alignment"): the two device passes of
// tools/reproj_error.py.
//   ncw_pixel_nearest   reproj_error.py:21-51   (get_gt_point: project the WHOLE cloud into a view, keep what lands on one pixel,
//                                                take the nearest), for all queries in one pass over the cloud
//   ncw_reproj_errors   reproj_error.py:120-138, 233-236   (per-observation reprojection error and its per-segment sums)
//
// ncw_pixel_nearest.  The reference makes about 15 torch ops over [batch, n_points, 4] tensors, two queries at a time.  Here
// the points live in registers (one lane owns PPL points, a workgroup WG_POINTS consecutive ones) and the workgroup walks ALL
// queries for them: a tile of QT queries is staged in LDS (with X, Y and the prefilter's half-widths precomputed), and every
// wave reads query after query from it at a wave-uniform address (a broadcast, no bank conflict).  Per pair the contract's
// c_0, c_1, c_2 and the two numerators are computed exactly as written below -- these ARE the values of the exact test -- and
// a division-free bound decides whether the pair can hit; about one pair in (width x height) survives and only those pay the
// two IEEE divisions and the two rintf.  Survivors that hit issue their 64-bit integer atomicMin directly (hits are rare).
// An integer min does not depend on arrival order: the result is bitwise reproducible and the same for any split of the cloud
// into launches.  No float atomics.
//
// The prefilter is a superset of the exact predicate.  Notation: eps = 2^-24, fl() = round to nearest float32, nu = the
// float32 numerator fx c_0 + cx c_2 AS COMPUTED (the exact test divides this very value), c = c_2, 2^-95 <= c < 2^97 (outside
// that range, and for c = +-0, the pair goes to the exact test without the bound; c < 0 or NaN can never hit).
//   exact hit        =>  rintf(u) == X with u = fl(nu / c)  =>  |u - X| <= 0.5
//   u = (nu / c)(1 + d0), |d0| <= eps (or u subnormal: X = 0 and the error is below 2^-149)
//                    =>  |nu / c - X| <= 0.5 + eps |nu / c|  and  |nu / c| <= (|X| + 0.5) / (1 - eps)
//                    =>  |nu - X c| <= (0.5 + a) c,   a = eps (|X| + 0.5)(1 + 2 eps)
//   the bound computes t = fl(X c) = X c (1 + d1), d = fl(nu - t) = (nu - t)(1 + d2), r = fl(h c) >= h c (1 - eps)
//   (no overflow or underflow in the range of c above for |X| < 2^24; a subnormal difference is exact), so
//                        |d| <= (1 + eps)(|nu - X c| + eps |X| c) <= (1 + eps)(0.5 + a + eps |X|) c
//   and |d| <= r holds whenever h (1 - eps) >= (1 + eps)(0.5 + a + eps |X|), i.e. m = h - 0.5 >= eps (2 |X| + 1.5) + O(eps^2).
//   The kernel takes m = 2^-22 (|X| + 1) = eps (4 |X| + 4): more than twice that, which also covers the rounding of m itself
//   (relative eps) and of h = fl(0.5 + m) (at most 2^-25 absolute while h < 1; above, m >= 0.5 and the slack is larger still).
// The same holds in v with fy, c_1, cy, Y.  |X| >= 2^24 (no real key-point): m >= 4 and the bound is still a bound, since
// every step above only used |X| through eps |X|.  A NaN anywhere fails the bound and fails the exact test alike.
//
// ncw_reproj_errors.  One wave per segment: every lane walks the segment's observations with stride 64, writes err and keeps a
// float64 partial in sequence; a fixed xor butterfly (32, 16, .. 1) then sums the 64 partials, so the sum's order is fixed by
// the segment alone and the result is bitwise reproducible.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

namespace {

constexpr int RB = 256;               // threads per workgroup
constexpr int PPL = 8;                // points per lane, in registers
constexpr int WG_POINTS = RB * PPL;   // consecutive points of one workgroup (NCW_PIXNN_WG_POINTS)
constexpr int QT = 256;               // queries per LDS tile (NCW_PIXNN_QUERY_TILE): one per thread when the tile is staged
constexpr int QF = 20;                // floats per staged query

static_assert(WG_POINTS == NCW_PIXNN_WG_POINTS && QT == NCW_PIXNN_QUERY_TILE, "the header's tile constants are the tests' shape edges");
static_assert(QT == RB, "one query per thread when a tile is staged");

// a staged query is five float4: w2c rows 0, 1, 2, (fx, fy, cx, cy), (X, Y, hu, hv)

NCW_DEV float half_width(float X) {
#pragma clang fp contract(off)
    return 0.5f + 0x1p-22f * (fabsf(X) + 1.0f);
}

__global__ __launch_bounds__(RB) void pixel_nearest_kernel(const NcwPixelQuery* __restrict__ queries, int n_queries,
                                                           const float* __restrict__ xyz, uint32_t p0, int64_t n,
                                                           unsigned long long* __restrict__ best) {
#pragma clang fp contract(off)
    __shared__ float4 tile[QT * (QF / 4)];
    const int64_t base = (int64_t)blockIdx.x * WG_POINTS + threadIdx.x;
    float px[PPL], py[PPL], pz[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        const int64_t i = base + (int64_t)k * RB;
        const bool in = i < n;
        const float nan = __uint_as_float(0x7fc00000u);  // a lane past the end: NaN fails every compare below
        px[k] = in ? xyz[3 * i + 0] : nan;
        py[k] = in ? xyz[3 * i + 1] : nan;
        pz[k] = in ? xyz[3 * i + 2] : nan;
    }
    for (int q0 = 0; q0 < n_queries; q0 += QT) {
        __syncthreads();  // the previous tile is no longer read
        const int nq = n_queries - q0 < QT ? n_queries - q0 : QT;
        if ((int)threadIdx.x < nq) {
            const NcwPixelQuery& g = queries[q0 + threadIdx.x];
            const float X = rintf(g.qx), Y = rintf(g.qy);
            float4* s = &tile[threadIdx.x * (QF / 4)];
            s[0] = make_float4(g.w2c[0], g.w2c[1], g.w2c[2], g.w2c[3]);
            s[1] = make_float4(g.w2c[4], g.w2c[5], g.w2c[6], g.w2c[7]);
            s[2] = make_float4(g.w2c[8], g.w2c[9], g.w2c[10], g.w2c[11]);
            s[3] = make_float4(g.fx, g.fy, g.cx, g.cy);
            s[4] = make_float4(X, Y, half_width(X), half_width(Y));
        }
        __syncthreads();
        for (int q = 0; q < nq; ++q) {
            const float4* s = &tile[q * (QF / 4)];  // wave-uniform address: a broadcast read
            const float4 w0 = s[0], w1 = s[1], w2 = s[2], kk = s[3], t = s[4];
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
                const float x = px[k], y = py[k], z = pz[k];
                const float c0 = ((w0.x * x + w0.y * y) + w0.z * z) + w0.w;
                const float c1 = ((w1.x * x + w1.y * y) + w1.z * z) + w1.w;
                const float c2 = ((w2.x * x + w2.y * y) + w2.z * z) + w2.w;
                const float nu = kk.x * c0 + kk.z * c2;
                const float nv = kk.y * c1 + kk.w * c2;
                const float du = nu - t.x * c2;
                const float dv = nv - t.y * c2;
                const bool near_pixel = (fabsf(du) <= t.z * c2) & (fabsf(dv) <= t.w * c2);
                // the bound is argued for 2^-95 <= c2 < 2^97 (bit patterns 0x10000000 .. 0x6fffffff): any other c2 >= 0 goes to
                // the exact test whatever the bound says (negative and NaN patterns wrap round to "inside": they never hit)
                const bool unbounded = (__float_as_uint(c2) - 0x10000000u >= 0x60000000u) & (c2 >= 0.f);
                const bool survivor = near_pixel | unbounded;
                if (survivor) {
                    // the divisor passes through an empty asm statement, so that the compiler cannot move a division out of
                    // this rare branch (it did: one speculated division per pair)
                    float cd = c2;
                    asm volatile("" : "+v"(cd));
                    const float u = __fdiv_rn(nu, cd), v = __fdiv_rn(nv, cd);
                    if (rintf(u) == t.x && rintf(v) == t.y && c2 >= 0.f) {
                        const int64_t i = base + (int64_t)k * RB;
                        const unsigned long long key =
                            ((unsigned long long)__float_as_uint(c2 + 0.0f) << 32) | (unsigned long long)(p0 + (uint32_t)i);
                        atomicMin(&best[q0 + q], key);
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(RB) void reproj_errors_kernel(const float* __restrict__ proj, int n_cams, const float* __restrict__ xyz,
                                                           int64_t n_pts, const int32_t* __restrict__ cam_idx,
                                                           const int32_t* __restrict__ pt_idx, const float* __restrict__ xy, int64_t n_obs,
                                                           const int64_t* __restrict__ seg_start, int64_t n_seg,
                                                           float* __restrict__ err, double* __restrict__ seg_sum) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * (RB / 64) + (threadIdx.x >> 6);
    if (seg >= n_seg) return;  // uniform over the wave
    int64_t i0 = seg_start[seg], i1 = seg_start[seg + 1];
    i0 = i0 < 0 ? 0 : i0;
    i1 = i1 > n_obs ? n_obs : i1;
    double part = 0.0;
    for (int64_t i = i0 + lane; i < i1; i += 64) {
        const int c = cam_idx[i];
        const int64_t p = pt_idx[i];
        float e = __uint_as_float(0x7fc00000u);  // an index outside its table reads nothing and gives NaN
        if (c >= 0 && c < n_cams && p >= 0 && p < n_pts) {
            const float* P = proj + 12 * (int64_t)c;
            const float x = xyz[3 * p + 0], y = xyz[3 * p + 1], z = xyz[3 * p + 2];
            const float h0 = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
            const float h1 = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
            const float h2 = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
            const float dx = __fdiv_rn(h0, h2) - xy[2 * i + 0];
            const float dy = __fdiv_rn(h1, h2) - xy[2 * i + 1];
            e = sqrtf(dx * dx + dy * dy);  // correctly rounded (the compiler's default for sqrtf; __fsqrt_rn is the 1-ulp instruction)
        }
        err[i] = e;
        part += (double)e;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
    if (lane == 0) seg_sum[seg] = part;
}

}  // namespace

extern "C" int ncw_pixel_nearest(const NcwPixelQuery* queries_dev, int n_queries, const float* xyz_dev, int64_t p0, int64_t n,
                                 int clear, uint64_t* best_dev, void* stream) {
    if (queries_dev == nullptr || xyz_dev == nullptr || best_dev == nullptr || n_queries < 1 || n < 0 || p0 < 0 ||
        p0 > 0xffffffffLL || p0 + n > 0xffffffffLL)
        return NCW_E_BADARG;
    if (clear != 0) {
        hipError_t e = hipMemsetAsync(best_dev, 0xff, (size_t)n_queries * sizeof(uint64_t), (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    if (n == 0) return 0;
    const int64_t grid = (n + WG_POINTS - 1) / WG_POINTS;  // at most 2^32 / 2048 workgroups
    hipLaunchKernelGGL(pixel_nearest_kernel, dim3((unsigned)grid), dim3(RB), 0, (hipStream_t)stream, queries_dev, n_queries, xyz_dev,
                       (uint32_t)p0, n, reinterpret_cast<unsigned long long*>(best_dev));
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_reproj_errors(const float* proj_dev, int n_cams, const float* xyz_dev, int64_t n_pts, const int32_t* cam_idx_dev,
                                 const int32_t* pt_idx_dev, const float* xy_dev, int64_t n_obs, const int64_t* seg_start_dev,
                                 int64_t n_seg, float* err_dev, double* seg_sum_dev, void* stream) {
    if (proj_dev == nullptr || xyz_dev == nullptr || cam_idx_dev == nullptr || pt_idx_dev == nullptr || xy_dev == nullptr ||
        seg_start_dev == nullptr || err_dev == nullptr || seg_sum_dev == nullptr || n_cams < 1 || n_pts < 1 || n_obs < 0 || n_seg < 0 ||
        n_seg > 0x7fffffffLL)
        return NCW_E_BADARG;
    if (n_seg == 0) return 0;
    const int64_t grid = (n_seg + RB / 64 - 1) / (RB / 64);
    hipLaunchKernelGGL(reproj_errors_kernel, dim3((unsigned)grid), dim3(RB), 0, (hipStream_t)stream, proj_dev, n_cams, xyz_dev, n_pts,
                       cam_idx_dev, pt_idx_dev, xy_dev, n_obs, seg_start_dev, n_seg, err_dev, seg_sum_dev);
    NCW_CHECK_LAUNCH();
    return 0;
}
