// Region-of-interest shares of ALL registered views of a scene in one launch (include/neuconw_hip.h, "View selection"): the
// per-pixel test of tools/prepare_data/dataset_filter_utils.py:160-178 (view_selection), which the reference runs per image as
// get_ray_directions + get_rays + eight torch ops after decoding the image only to learn its size.  The test needs no per-pixel
// input: the camera table and the sizes are enough.
//   ncw_views_roi      dataset_filter_utils.py:168-178   (count of ROI pixels per view, optional 0 / 1 mask per pixel)
// Contract: pixel (row, col) of view v is global pixel pix_start[v] + row * width + col; its ray is view_ray_dir's
// (csrc/ncw_raymath.h: integer pixel coordinates, o = c2w[:, 3], d normalised), and in float32, in the reference's order,
//   c = origin - o;  dot = sum(c * d);  p = dot * d;  dist_ray = |c - p|;  dist_cam = |c|
//   roi = (radius > dist_cam  or  dot > 0)  and  dist_ray < radius
// One lane handles one pixel per step; a workgroup walks a contiguous RUN of tiles of TILE consecutive global pixels, so that the
// view found by ONE binary search of pix_start at the start of the run only ever moves forward.  The terms that are constant over a
// view (c, dist_cam, radius > dist_cam) are recomputed only when a lane's view changes.  The kernel reads the camera table and
// pix_start and nothing else.  Counting: 64-bit ballot + population count per wave and view, kept in a register across the
// tiles of the run while the wave stays in that view; a finished view goes to the workgroup's LDS slots with one integer add per
// wave, and at the end of the run the workgroup issues ONE integer atomicAdd per view it touched (a run that touches more than
// SLOTS views -- views of a few pixels -- adds the later ones per wave instead).  Two barriers per run, none per tile.  Integer
// sums do not depend on arrival order, so the counts are bitwise reproducible.  No float atomics.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_raymath.h"

namespace {

constexpr int RB = 256;            // threads per workgroup
constexpr int ITEMS = 4;           // pixels per lane and tile
constexpr int TILE = RB * ITEMS;   // consecutive global pixels per tile
constexpr int SLOTS = 8;           // views of a run summed in LDS (the first SLOTS the run touches); later ones add per wave
constexpr int GRID = 2048;         // workgroups of the one launch (8 per CU on 256 CUs); each walks ceil(tiles / GRID) tiles

// the view-constant part of the predicate
struct RoiView {
    float c[3];      // origin - o
    float dist_cam;  // |c|
    bool inside;     // radius > dist_cam
};

NCW_DEV RoiView roi_view(const NcwViewCamera& cam, const float (&origin)[3], float radius) {
#pragma clang fp contract(off)
    RoiView r;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.c[k] = origin[k] - cam.c2w[4 * k + 3];
    r.dist_cam = sqrtf(r.c[0] * r.c[0] + r.c[1] * r.c[1] + r.c[2] * r.c[2]);
    r.inside = radius > r.dist_cam;
    return r;
}

// dataset_filter_utils.py:171-177 for one pixel; products and sums rounded one by one, as torch does
NCW_DEV bool roi_pixel(const NcwViewCamera& cam, const RoiView& rv, int row, int col, float radius) {
#pragma clang fp contract(off)
    float d[3];
    const float nrm = view_ray_dir(cam, row, col, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = d[k] / nrm;
    const float dot = rv.c[0] * d[0] + rv.c[1] * d[1] + rv.c[2] * d[2];
    const float q0 = rv.c[0] - dot * d[0], q1 = rv.c[1] - dot * d[1], q2 = rv.c[2] - dot * d[2];
    const float dist_ray = sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
    return (rv.inside || dot > 0.f) && dist_ray < radius;
}

struct Origin3 {
    float v[3];
};

// this wave's finished count of view acc_v: into the workgroup's LDS slot of that view, or, past the slots, straight to global memory
NCW_DEV void wave_flush(int lane, int acc_v, uint32_t acc_c, int v_run, uint32_t* slots, uint32_t* __restrict__ count) {
    if (lane == 0 && acc_c != 0u) {
        const int s = acc_v - v_run;
        if (s < SLOTS) atomicAdd(&slots[s], acc_c);
        else atomicAdd(&count[acc_v], acc_c);
    }
}

__global__ __launch_bounds__(RB) void views_roi_kernel(const NcwViewCamera* __restrict__ cams, const int64_t* __restrict__ pix_start,
                                                       int n_views, Origin3 origin, float radius, uint32_t* __restrict__ count,
                                                       uint8_t* __restrict__ mask) {
    __shared__ uint32_t slots[SLOTS];
    const int64_t n_pix = pix_start[n_views];
    const int64_t n_tiles = (n_pix + TILE - 1) / TILE;
    const int64_t per_wg = (n_tiles + GRID - 1) / GRID;
    const int64_t t0 = (int64_t)blockIdx.x * per_wg;
    const int64_t t1 = t0 + per_wg < n_tiles ? t0 + per_wg : n_tiles;
    if (t0 >= t1) return;  // uniform over the workgroup
    const int lane = threadIdx.x & 63;
    // the view of the run's first pixel: the largest v with pix_start[v] <= p (p < n_pix = pix_start[n_views], so v < n_views)
    int v_run;
    {
        const int64_t p = t0 * TILE;
        int lo = 0, hi = n_views;  // pix_start[lo] <= p < pix_start[hi]
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (pix_start[mid] <= p) lo = mid; else hi = mid;
        }
        v_run = lo;
    }
    if (threadIdx.x < SLOTS) slots[threadIdx.x] = 0u;
    __syncthreads();
    const float org[3] = {origin.v[0], origin.v[1], origin.v[2]};
    int v = v_run;  // lane-local: the view of the lane's latest pixel; a lane's pixels ascend, so it only moves forward
    int v_loaded = -1;
    int64_t v_begin = 0, v_end = 0;  // pix_start[v_loaded], pix_start[v_loaded + 1]
    NcwViewCamera cam;
    RoiView rv;
    // the wave's running view and its count, the same in every lane (built from ballots); a wave's pixels ascend too, so it
    // finishes a view before it starts the next and hands every view over exactly once
    int acc_v = -1;
    uint32_t acc_c = 0u;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t base = t * TILE;
#pragma unroll 1
        for (int k = 0; k < ITEMS; ++k) {
            const int64_t p = base + (int64_t)k * RB + threadIdx.x;
            const bool active = p < n_pix;
            bool roi = false;
            if (active) {
                if (v_loaded < 0 || p >= v_end) {
                    while (p >= pix_start[v + 1]) ++v;  // p < n_pix: stops at v + 1 <= n_views
                    cam = cams[v];
                    rv = roi_view(cam, org, radius);
                    v_begin = pix_start[v];
                    v_end = pix_start[v + 1];
                    v_loaded = v;
                }
                const int64_t local = p - v_begin;
                const int w = cam.width > 0 ? cam.width : 1;
                int row, col;
                if (local <= 0x7fffffffLL) {
                    row = (int)((uint32_t)local / (uint32_t)w);
                    col = (int)((uint32_t)local - (uint32_t)row * (uint32_t)w);
                } else {
                    const int64_t r64 = local / w;
                    row = (int)r64;
                    col = (int)(local - r64 * w);
                }
                roi = roi_pixel(cam, rv, row, col, radius);
                if (mask != nullptr) mask[p] = roi ? 1 : 0;
            }
            // per wave and view: ballot + population count; the views of a wave's lanes are few and ascending
            unsigned long long pending = __ballot(active);
            while (pending != 0ull) {
                const int first = __builtin_ctzll(pending);
                const int vv = __shfl(v_loaded, first, 64);
                const bool mine = active && v_loaded == vv;
                const unsigned long long of_view = __ballot(mine);
                const uint32_t cnt = (uint32_t)__popcll(__ballot(mine && roi));
                if (vv != acc_v) {
                    wave_flush(lane, acc_v, acc_c, v_run, slots, count);
                    acc_v = vv;
                    acc_c = 0u;
                }
                acc_c += cnt;
                pending &= ~of_view;
            }
        }
    }
    wave_flush(lane, acc_v, acc_c, v_run, slots, count);
    __syncthreads();
    if (threadIdx.x < SLOTS) {
        const uint32_t c = slots[threadIdx.x];
        if (c != 0u) atomicAdd(&count[v_run + threadIdx.x], c);  // c != 0: some lane was in that view, so it is < n_views
    }
}

}  // namespace

extern "C" int ncw_views_roi(const NcwViewCamera* cams_dev, const int64_t* pix_start_dev, int n_views, const float* origin_host,
                             float radius, uint32_t* count_dev, uint8_t* mask_dev, void* stream) {
    if (cams_dev == nullptr || pix_start_dev == nullptr || origin_host == nullptr || count_dev == nullptr || n_views < 1 ||
        !(radius > 0.f))
        return NCW_E_BADARG;
    hipError_t e = hipMemsetAsync(count_dev, 0, (size_t)n_views * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    Origin3 o = {{origin_host[0], origin_host[1], origin_host[2]}};
    hipLaunchKernelGGL(views_roi_kernel, dim3(GRID), dim3(RB), 0, (hipStream_t)stream, cams_dev, pix_start_dev, n_views, o, radius,
                       count_dev, mask_dev);
    NCW_CHECK_LAUNCH();
    return 0;
}
