// Estimating sfm2gt: the two kernels of the gated similarity ICP of align.icp_similarity (the reference has no such tool: it
// ships the matrices).  The contract -- the rounding order of the transform, the inside test, which pairs take part, the 20 sums
// and the order they are added in -- is stated once in include/neuconw_hip.h and restated in numpy by tests/_align_ref.py.
//
//   ncw_align_transform : one lane per source point: x = T [p, 1] in float64, the float32 query x - centre for evalmesh.NNGrid
//                         and the flag "inside the target's box grown by the gate";
//   (caller)            : compacts the inside points (torch), NNGrid.query, scatters idx / dist back (idx = -1 elsewhere);
//   ncw_align_sums      : the correspondence reduction.  Block b owns NCW_ALIGN_BLOCK consecutive points, lane l adds the points
//                         b BLOCK + j LANES + l in ascending j, the lanes are folded by a fixed tree, one row of partials per block;
//                         a second launch of ONE workgroup adds the rows (lane l: rows l, l + LANES, ...) and folds by the same
//                         tree.  THE ORDER IS THE CONTRACT: a function of N and the data, the same bits on every run.
//
// No float atomics.  Every index read from idx is range-checked before it is used.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

// every product and sum is rounded on its own (no fused multiply-add): the numpy restatement is then the same arithmetic
#pragma clang fp contract(off)

namespace {

constexpr int kLanes = NCW_ALIGN_LANES;
constexpr int kBlock = NCW_ALIGN_BLOCK;
constexpr int kPerLane = kBlock / kLanes;
constexpr int kWaves = kLanes / 64;
constexpr int kSums = NCW_ALIGN_SUMS;
constexpr int64_t kMaxCount = 0x7fffffffll;
static_assert(kBlock % kLanes == 0 && kLanes % 64 == 0 && kWaves == 4, "the tree below is written for 4 waves of 64");

struct Mat34 {
    double m[12];
};
struct Vec3d {
    double v[3];
};
struct Box3f {
    float lo[3], hi[3];
};

// ((T0 x + T1 y) + T2 z) + T3
__device__ __forceinline__ double row_apply(const double* t, double x, double y, double z) {
    return ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
}

__global__ __launch_bounds__(256) void align_transform_kernel(const double* __restrict__ src, int64_t n, Mat34 T, Vec3d centre,
                                                               Box3f box, float gate, float* __restrict__ q32,
                                                               uint8_t* __restrict__ inside) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = src[i * 3 + 0], y = src[i * 3 + 1], z = src[i * 3 + 2];
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = (float)(row_apply(T.m + 4 * a, x, y, z) - centre.v[a]);
        q32[i * 3 + a] = q;
        in = in && (q >= box.lo[a] - gate) && (q <= box.hi[a] + gate);  // float32; false for NaN
    }
    inside[i] = in ? 1 : 0;
}

// v[l] = v[l] + v[l + s] for s = 32 .. 1 inside each wave, then (w0 + w1) + (w2 + w3) over the four wave sums; the result is
// valid on thread 0.  `lds`: kWaves doubles per value.
__device__ __forceinline__ void fold_lanes(double (&acc)[kSums], long long& cnt, long long& mx, double* lds, long long* ilds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = acc[k] + __shfl_down(acc[k], s, 64);
        cnt += __shfl_down(cnt, s, 64);
        const long long o = __shfl_down(mx, s, 64);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) lds[k * kWaves + wave] = acc[k];
        ilds[wave] = cnt;
        ilds[kWaves + wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = (lds[k * kWaves + 0] + lds[k * kWaves + 1]) + (lds[k * kWaves + 2] + lds[k * kWaves + 3]);
        cnt = (ilds[0] + ilds[1]) + (ilds[2] + ilds[3]);
        long long m = ilds[kWaves];
        for (int w = 1; w < kWaves; ++w) m = ilds[kWaves + w] > m ? ilds[kWaves + w] : m;
        mx = m;
    }
}

__global__ __launch_bounds__(kLanes) void align_sums_kernel(const double* __restrict__ src, int64_t n, Vec3d cp,
                                                            const double* __restrict__ dst, int64_t m, Vec3d cq,
                                                            const int64_t* __restrict__ idx, const float* __restrict__ dist,
                                                            float gate, Mat34 T, double* __restrict__ part,
                                                            long long* __restrict__ ipart) {
    __shared__ double lds[kSums * kWaves];
    __shared__ long long ilds[2 * kWaves];
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    long long cnt = 0, mx = 0;
    const int64_t base = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int j = 0; j < kPerLane; ++j) {
        const int64_t i = base + (int64_t)j * kLanes;
        if (i >= n) break;
        const int64_t t = idx[i];
        if (t < 0 || t >= m || !(dist[i] <= gate)) continue;  // float32, inclusive; NaN takes no part
        const double X = src[i * 3 + 0], Y = src[i * 3 + 1], Z = src[i * 3 + 2];
        const double U = dst[t * 3 + 0], V = dst[t * 3 + 1], W = dst[t * 3 + 2];
        const double p[3] = {X - cp.v[0], Y - cp.v[1], Z - cp.v[2]};
        const double q[3] = {U - cq.v[0], V - cq.v[1], W - cq.v[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[a] = acc[a] + p[a];
            acc[3 + a] = acc[3 + a] + q[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[6 + 3 * a + b] = acc[6 + 3 * a + b] + p[a] * q[b];
        }
        acc[15] = acc[15] + ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
        acc[16] = acc[16] + ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
        const double d0 = row_apply(T.m + 0, X, Y, Z) - U;
        const double d1 = row_apply(T.m + 4, X, Y, Z) - V;
        const double d2 = row_apply(T.m + 8, X, Y, Z) - W;
        const double r2 = (d0 * d0 + d1 * d1) + d2 * d2;
        acc[17] = acc[17] + r2;
        acc[18] = acc[18] + (double)dist[i];
        acc[19] = acc[19] + (double)dist[i] * (double)dist[i];
        if (r2 == r2) {  // a non-negative double orders like its bit pattern
            const long long bits = __double_as_longlong(r2);
            mx = bits > mx ? bits : mx;
        }
        ++cnt;
    }
    fold_lanes(acc, cnt, mx, lds, ilds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) part[(int64_t)blockIdx.x * kSums + k] = acc[k];
        ipart[(int64_t)blockIdx.x * 2 + 0] = cnt;
        ipart[(int64_t)blockIdx.x * 2 + 1] = mx;
    }
}

__global__ __launch_bounds__(kLanes) void align_fold_kernel(const double* __restrict__ part, const long long* __restrict__ ipart,
                                                            int64_t n_blocks, double* __restrict__ sums,
                                                            long long* __restrict__ counts) {
    __shared__ double lds[kSums * kWaves];
    __shared__ long long ilds[2 * kWaves];
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    long long cnt = 0, mx = 0;
    for (int64_t r = threadIdx.x; r < n_blocks; r += kLanes) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = acc[k] + part[r * kSums + k];
        cnt += ipart[r * 2 + 0];
        const long long o = ipart[r * 2 + 1];
        mx = o > mx ? o : mx;
    }
    fold_lanes(acc, cnt, mx, lds, ilds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) sums[k] = acc[k];
        counts[0] = cnt;
        counts[1] = mx;
    }
}

}  // namespace

extern "C" int ncw_align_transform(const double* src, int64_t n, const double* T, const double* centre, const float* box_lo,
                                   const float* box_hi, float gate, float* q32, uint8_t* inside, void* stream) {
    if (n < 0 || n > kMaxCount || !T || !centre || !box_lo || !box_hi) return NCW_E_BADARG;
    if (n > 0 && (!src || !q32 || !inside)) return NCW_E_BADARG;
    if (n == 0) return 0;
    Mat34 t;
    Vec3d c;
    Box3f b;
    for (int k = 0; k < 12; ++k) t.m[k] = T[k];
    for (int a = 0; a < 3; ++a) c.v[a] = centre[a], b.lo[a] = box_lo[a], b.hi[a] = box_hi[a];
    hipLaunchKernelGGL(align_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, n, t, c, b,
                       gate, q32, inside);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t ncw_align_sums_blocks(int64_t n) { return n <= 0 ? 0 : (n + kBlock - 1) / kBlock; }

extern "C" int ncw_align_sums(const double* src, int64_t n, const double* cp, const double* dst, int64_t m, const double* cq,
                              const int64_t* idx, const float* dist, float gate, const double* T, double* part, int64_t* ipart,
                              double* sums, int64_t* counts, void* stream) {
    if (n < 0 || n > kMaxCount || m < 0 || !cp || !cq || !T || !sums || !counts) return NCW_E_BADARG;
    if (n > 0 && (!src || !idx || !dist || !part || !ipart || (m > 0 && !dst))) return NCW_E_BADARG;
    Mat34 t;
    Vec3d a, b;
    for (int k = 0; k < 12; ++k) t.m[k] = T[k];
    for (int k = 0; k < 3; ++k) a.v[k] = cp[k], b.v[k] = cq[k];
    const int64_t nb = ncw_align_sums_blocks(n);
    if (nb > 0) {
        hipLaunchKernelGGL(align_sums_kernel, dim3((unsigned)nb), dim3(kLanes), 0, (hipStream_t)stream, src, n, a, dst, m, b, idx,
                           dist, gate, t, part, (long long*)ipart);
        NCW_CHECK_LAUNCH();
    }
    // N == 0: the fold over no rows writes the zeros
    hipLaunchKernelGGL(align_fold_kernel, dim3(1), dim3(kLanes), 0, (hipStream_t)stream, part, (const long long*)ipart, nb, sums,
                       (long long*)counts);
    NCW_CHECK_LAUNCH();
    return 0;
}
