// Per-view depth / normal scores against ground truth (include/neuconw_hip.h, "Depth and normal maps against ground truth";
// depthmetrics.compare_planes).  The reference has no such evaluation: the per-pixel rules, the row layout and the order of the
// sums are this project's, stated once in the header and restated in numpy by tests/_depthmetrics_ref.py.
//
//   depthmetrics_kernel<MODE> : workgroup b owns NCW_DM_BLOCK consecutive pixels, lane l the pixels b BLOCK + j LANES + l in
//                               ascending j.  Per pixel: class, the float32 terms, the two histogram bins (binary search over the
//                               edge tables, staged in LDS).  float64 sums: lane-sequential, then the fixed lane tree, one row of
//                               partials per workgroup.  Counts: one 64-bit ballot + popcount per wave and pixel step.
//                               Histograms: LDS integer atomics, flushed with 64-bit integer global atomics into row v (zeroed
//                               by the entry point): integer adds commute, so the bits do not depend on the order.
//   depthmetrics_fold_kernel  : ONE workgroup adds the rows of partials (lane l: rows l, l + LANES, ..) and folds by the same tree.
//
// No float atomics, no transcendental function (every cos / pow constant comes from the host), every index is range-checked.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_raymath.h"

#include <float.h>

// every product, quotient and sum is rounded on its own (no fused multiply-add): the numpy restatement is the same arithmetic
#pragma clang fp contract(off)

namespace {

constexpr int kLanes = NCW_DM_LANES;
constexpr int kBlock = NCW_DM_BLOCK;
constexpr int kPerLane = kBlock / kLanes;
constexpr int kWaves = kLanes / 64;
constexpr int kSums = NCW_DM_SUMS;
constexpr int kCounts = NCW_DM_COUNTS;
constexpr int kMaxEdges = NCW_DM_MAX_EDGES;
static_assert(kBlock % kLanes == 0 && kLanes % 64 == 0 && kWaves == 4, "the tree below is written for 4 waves of 64");
static_assert(NCW_DM_FIXED == kSums + kCounts, "row layout");

// indices into the counts (row words kSums + k)
enum { C_BOTH = 0, C_GT_ONLY, C_PRED_ONLY, C_NEITHER, C_MASKED, C_D1, C_D2, C_D3, C_NORMAL, C_A1, C_A2, C_A3 };

struct DmArgs {
    NcwViewCamera cam;
    float scale;
    float delta_thr[3];
    float cos_thr[3];
    int n_cos, n_rel;
    int width;
};

NCW_DEV bool finite32(float x) { return __builtin_fabsf(x) <= FLT_MAX; }  // false for NaN and +-inf

// v[l] = v[l] + v[l + s] for s = 32 .. 1 inside each wave, then (w0 + w1) + (w2 + w3); counts likewise (integers: any order).
// The result is valid on thread 0.
NCW_DEV void fold_lanes(double (&acc)[kSums], long long (&cnt)[kCounts], bool cnt_per_wave, double* lds, long long* ilds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = acc[k] + __shfl_down(acc[k], s, 64);
        if (!cnt_per_wave) {
#pragma unroll
            for (int k = 0; k < kCounts; ++k) cnt[k] += __shfl_down(cnt[k], s, 64);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) lds[k * kWaves + wave] = acc[k];
#pragma unroll
        for (int k = 0; k < kCounts; ++k) ilds[k * kWaves + wave] = cnt[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = (lds[k * kWaves + 0] + lds[k * kWaves + 1]) + (lds[k * kWaves + 2] + lds[k * kWaves + 3]);
#pragma unroll
        for (int k = 0; k < kCounts; ++k) cnt[k] = (ilds[k * kWaves + 0] + ilds[k * kWaves + 1]) + (ilds[k * kWaves + 2] + ilds[k * kWaves + 3]);
    }
}

template <int MODE>
__global__ __launch_bounds__(kLanes) void depthmetrics_kernel(const float* __restrict__ gt_z, const float* __restrict__ gt_n,
                                                              const float* __restrict__ pred, const float* __restrict__ pred_n,
                                                              const uint8_t* __restrict__ mask, int64_t n, DmArgs a,
                                                              const float* __restrict__ cos_edges, const float* __restrict__ rel_edges,
                                                              double* __restrict__ part, long long* __restrict__ ipart,
                                                              unsigned long long* __restrict__ hist_rel,
                                                              unsigned long long* __restrict__ hist_cos, float* __restrict__ err_rel,
                                                              float* __restrict__ err_cos, float* __restrict__ z_pred) {
    __shared__ float s_rel[kMaxEdges], s_cos[kMaxEdges];
    __shared__ unsigned int h_rel[kMaxEdges + 1], h_cos[kMaxEdges + 1];
    __shared__ double lds[kSums * kWaves];
    __shared__ long long ilds[kCounts * kWaves];
    const int nr = a.n_rel, na = a.n_cos;  // 1 .. kMaxEdges (checked by the entry point)
    const bool normals = gt_n != nullptr && pred_n != nullptr;
    const int nmax = nr > na ? nr : na;
    for (int t = threadIdx.x; t <= nmax; t += kLanes) {
        if (t < nr) s_rel[t] = rel_edges[t];
        if (t < na) s_cos[t] = cos_edges[t];
        h_rel[t] = 0u;
        h_cos[t] = 0u;
    }
    __syncthreads();

    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    int cnt[kCounts];  // the same value on every lane of a wave; at most kBlock
#pragma unroll
    for (int k = 0; k < kCounts; ++k) cnt[k] = 0;
    const float qnan = __builtin_nanf("");
    const int64_t base = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int j = 0; j < kPerLane; ++j) {  // no lane leaves early: the ballots below want whole waves
        const int64_t i = base + (int64_t)j * kLanes;
        const bool in = i < n;
        bool masked = false, vg = false, vp = false;
        float zg = 0.f, zp = 0.f;
        if (in) {
            masked = mask != nullptr && mask[i] != 0;
            zg = gt_z[i];
            vg = finite32(zg) && zg > 0.f;
            const float pv = pred[i];
            if (MODE == NCW_DM_PRED_T) {
                const int row = (int)(i / a.width), col = (int)(i - (int64_t)row * a.width);
                float d[3];
                const float nrm = view_ray_dir(a.cam, row, col, d);
                zp = (pv * a.scale) / nrm;
                vp = finite32(pv) && pv > 0.f && finite32(zp) && zp > 0.f;
            } else {
                zp = pv;
                vp = finite32(pv) && pv > 0.f;
            }
            if (z_pred != nullptr) z_pred[i] = vp ? zp : 0.f;
        }
        const bool live = in && !masked;
        const bool both = live && vg && vp;
        float r = qnan, c = qnan;
        bool d1 = false, d2 = false, d3 = false, scored = false, a1 = false, a2 = false, a3 = false;
        if (both) {
            const float e = zp - zg;
            const float ae = __builtin_fabsf(e);
            r = ae / zg;
            const float q1 = zp / zg, q2 = zg / zp;
            const float q = q1 > q2 ? q1 : q2;
            const float ee = e * e;
            const float sq = ee / zg;
            acc[0] = acc[0] + (double)ae;
            acc[1] = acc[1] + (double)e;
            acc[2] = acc[2] + (double)ee;
            acc[3] = acc[3] + (double)r;
            acc[4] = acc[4] + (double)sq;
            d1 = q < a.delta_thr[0];
            d2 = q < a.delta_thr[1];
            d3 = q < a.delta_thr[2];
            int lo = 0, hi = nr;  // bin = the number of rel_edges <= r
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_rel[mid] <= r) lo = mid + 1;
                else hi = mid;
            }
            atomicAdd(&h_rel[lo], 1u);
            if (normals) {
                float g[3], p[3];
                bool fin = true, nzg = false, nzp = false;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    g[k] = gt_n[(int64_t)k * n + i];
                    const float v = pred_n[(int64_t)k * n + i];
                    p[k] = MODE == NCW_DM_PRED_T ? 2.f * v - 1.f : v;
                    fin = fin && finite32(g[k]) && finite32(p[k]);
                    nzg = nzg || g[k] != 0.f;
                    nzp = nzp || p[k] != 0.f;
                }
                scored = fin && nzg && nzp;
                if (scored) {
                    const float dot = (g[0] * p[0] + g[1] * p[1]) + g[2] * p[2];
                    c = dot < -1.f ? -1.f : (dot > 1.f ? 1.f : dot);
                    acc[5] = acc[5] + (double)c;
                    a1 = c >= a.cos_thr[0];
                    a2 = c >= a.cos_thr[1];
                    a3 = c >= a.cos_thr[2];
                    int l2 = 0, h2 = na;  // bin = the number of cos_edges > c (the table descends)
                    while (l2 < h2) {
                        const int mid = (l2 + h2) >> 1;
                        if (s_cos[mid] > c) l2 = mid + 1;
                        else h2 = mid;
                    }
                    atomicAdd(&h_cos[l2], 1u);
                }
            }
        }
        if (in) {
            if (err_rel != nullptr) err_rel[i] = r;
            if (err_cos != nullptr) err_cos[i] = c;
        }
        cnt[C_BOTH] += __popcll(__ballot(both));
        cnt[C_GT_ONLY] += __popcll(__ballot(live && vg && !vp));
        cnt[C_PRED_ONLY] += __popcll(__ballot(live && !vg && vp));
        cnt[C_NEITHER] += __popcll(__ballot(live && !vg && !vp));
        cnt[C_MASKED] += __popcll(__ballot(in && masked));
        cnt[C_D1] += __popcll(__ballot(d1));
        cnt[C_D2] += __popcll(__ballot(d2));
        cnt[C_D3] += __popcll(__ballot(d3));
        cnt[C_NORMAL] += __popcll(__ballot(scored));
        cnt[C_A1] += __popcll(__ballot(a1));
        cnt[C_A2] += __popcll(__ballot(a2));
        cnt[C_A3] += __popcll(__ballot(a3));
    }
    long long wcnt[kCounts];
#pragma unroll
    for (int k = 0; k < kCounts; ++k) wcnt[k] = cnt[k];
    fold_lanes(acc, wcnt, true, lds, ilds);  // its barrier also orders the LDS histogram atomics before the flush
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) part[(int64_t)blockIdx.x * kSums + k] = acc[k];
#pragma unroll
        for (int k = 0; k < kCounts; ++k) ipart[(int64_t)blockIdx.x * kCounts + k] = wcnt[k];
    }
    for (int t = threadIdx.x; t <= nmax; t += kLanes) {
        if (t <= nr && h_rel[t] != 0u) atomicAdd(&hist_rel[t], (unsigned long long)h_rel[t]);
        if (t <= na && h_cos[t] != 0u) atomicAdd(&hist_cos[t], (unsigned long long)h_cos[t]);
    }
}

__global__ __launch_bounds__(kLanes) void depthmetrics_fold_kernel(const double* __restrict__ part, const long long* __restrict__ ipart,
                                                                   int64_t n_blocks, long long* __restrict__ row) {
    __shared__ double lds[kSums * kWaves];
    __shared__ long long ilds[kCounts * kWaves];
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    long long cnt[kCounts];
#pragma unroll
    for (int k = 0; k < kCounts; ++k) cnt[k] = 0;
    for (int64_t r = threadIdx.x; r < n_blocks; r += kLanes) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = acc[k] + part[r * kSums + k];
#pragma unroll
        for (int k = 0; k < kCounts; ++k) cnt[k] += ipart[r * kCounts + k];
    }
    fold_lanes(acc, cnt, false, lds, ilds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) row[k] = __double_as_longlong(acc[k]);
#pragma unroll
        for (int k = 0; k < kCounts; ++k) row[kSums + k] = cnt[k];
    }
}

inline int64_t dm_blocks(int64_t n) { return n <= 0 ? 0 : (n + kBlock - 1) / kBlock; }

}  // namespace

extern "C" int64_t ncw_depthmetrics_scratch_bytes(int64_t n_pix) { return dm_blocks(n_pix) * (int64_t)(kSums + kCounts) * 8; }

extern "C" int ncw_depthmetrics_view(const float* gt_z, const float* gt_n, const float* pred, const float* pred_n, const uint8_t* mask,
                                     int height, int width, int mode, const NcwDepthMetricsParams* prm, void* scratch, int64_t* table,
                                     int64_t row, int64_t row_words, float* err_rel, float* err_cos, float* z_pred, void* stream) {
    if (prm == nullptr || gt_z == nullptr || pred == nullptr || scratch == nullptr || table == nullptr) return NCW_E_BADARG;
    if (height < 1 || width < 1 || row < 0 || (mode != NCW_DM_PRED_Z && mode != NCW_DM_PRED_T)) return NCW_E_BADARG;
    if (prm->n_cos_edges < 1 || prm->n_cos_edges > kMaxEdges || prm->n_rel_edges < 1 || prm->n_rel_edges > kMaxEdges ||
        prm->cos_edges == nullptr || prm->rel_edges == nullptr)
        return NCW_E_BADARG;
    if (row_words != (int64_t)NCW_DM_FIXED + (prm->n_rel_edges + 1) + (prm->n_cos_edges + 1)) return NCW_E_BADARG;
    if (!(prm->scale > 0.f) || !(prm->scale <= FLT_MAX)) return NCW_E_BADARG;
    if (mode == NCW_DM_PRED_T && (prm->cam.width != width || prm->cam.height != height)) return NCW_E_BADARG;
    if (((reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(table)) & 7) != 0) return NCW_E_BADARG;
    const int64_t n = (int64_t)height * width;
    const int64_t nb = dm_blocks(n);
    if (nb > 0x7fffffffLL) return NCW_E_BADARG;
    DmArgs a;
    a.cam = prm->cam;
    a.scale = prm->scale;
    for (int k = 0; k < 3; ++k) a.delta_thr[k] = prm->delta_thr[k], a.cos_thr[k] = prm->cos_thr[k];
    a.n_cos = prm->n_cos_edges;
    a.n_rel = prm->n_rel_edges;
    a.width = width;
    long long* out = reinterpret_cast<long long*>(table) + row * row_words;
    unsigned long long* hist_rel = reinterpret_cast<unsigned long long*>(out + NCW_DM_FIXED);
    unsigned long long* hist_cos = hist_rel + (a.n_rel + 1);
    double* part = static_cast<double*>(scratch);
    long long* ipart = reinterpret_cast<long long*>(part + nb * kSums);
    hipError_t e = hipMemsetAsync(hist_rel, 0, (size_t)(a.n_rel + 1 + a.n_cos + 1) * 8, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (mode == NCW_DM_PRED_T)
        hipLaunchKernelGGL(depthmetrics_kernel<NCW_DM_PRED_T>, dim3((unsigned)nb), dim3(kLanes), 0, (hipStream_t)stream, gt_z, gt_n, pred,
                           pred_n, mask, n, a, prm->cos_edges, prm->rel_edges, part, ipart, hist_rel, hist_cos, err_rel, err_cos, z_pred);
    else
        hipLaunchKernelGGL(depthmetrics_kernel<NCW_DM_PRED_Z>, dim3((unsigned)nb), dim3(kLanes), 0, (hipStream_t)stream, gt_z, gt_n, pred,
                           pred_n, mask, n, a, prm->cos_edges, prm->rel_edges, part, ipart, hist_rel, hist_cos, err_rel, err_cos, z_pred);
    NCW_CHECK_LAUNCH();
    hipLaunchKernelGGL(depthmetrics_fold_kernel, dim3(1), dim3(kLanes), 0, (hipStream_t)stream, (const double*)part,
                       (const long long*)ipart, nb, out);
    NCW_CHECK_LAUNCH();
    return 0;
}
