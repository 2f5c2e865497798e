// Training batches straight from the scene (include/neuconw_hip.h, "Ray source"): the rows ncw_cache_rows writes for an image
// (datasets/phototourism.py:557-657) and ncw_batch_assemble then gathers for a batch (datasets/phototourism.py:709-726, the
// black-list test of neuconw_system.py:345-349), rebuilt per batch row from an 8-byte record, the image's camera and the range
// octree -- no dense rows resident, none written to disk.
//   ncw_source_batch     one launch per batch, one lane per batch row
// Gather- and walk-bound, no MFMA.  Per lane: one 8-byte record (a random gather: one 64-byte sector per lane whatever the
// layout, so the record is one aligned 8-byte load and nothing else is read at a random address), a binary search over
// row_start and one 88-byte table entry (n_img is hundreds: both stay in L2 / the vector cache), and the range-octree walk, whose
// lanes diverge because a batch's rays are random: a batch is a few workgroups, each wave as slow as its longest walk, and that
// walk is the launch (profiles/source/: staging the brick mask in LDS was tried and bought 7 %, so it is not the loads).  Only
// key-point rows search the key-point table.  o, d, near, far come from ncw_rowmath.h, the functions ncw_cache_rows calls: the
// rows are the cached ones bit for bit.
// No atomics; every output element is written by exactly one lane from that lane's inputs: bitwise reproducible, and
// independent of how a set of indices is split into launches.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_rowmath.h"

namespace {

constexpr int SB = 256;    // threads per workgroup
constexpr int RAYC = 11;   // columns of a batch ray

struct SourceArgs {
    const NcwSourceRec* recs;
    int64_t n_rows;
    const NcwSourceImage* images;
    const int64_t* row_start;
    const int64_t* kp_start;
    int n_img;
    const int32_t* kp_pix;
    const float* kp_depth;
    const float* kp_weight;
    NcwCacheOctree range;
    int use_range;
    float voxel_size;
    const int64_t* idx;
    int64_t B;
    int with_semantics;
    float* rays;
    int64_t* ts;
    int64_t* label;
    float* rgbs;
    int4 ids;
    int n_ids;
    uint8_t* keep;
};

// The rows and the rgb triples go through LDS so that the workgroup writes its SB rows -- contiguous, and starting at a multiple
// of 16 bytes (SB * 44 and SB * 12 are) -- as 16-byte stores, as cache_rows_kernel does.
__global__ __launch_bounds__(SB) void source_batch_kernel(SourceArgs a) {
    __shared__ __attribute__((aligned(16))) float s_row[SB * RAYC];
    __shared__ __attribute__((aligned(16))) float s_rgb[SB * 3];
    const int64_t b0 = (int64_t)blockIdx.x * SB;
    const int64_t b = b0 + threadIdx.x;
    const int nb = (int)((a.B - b0) < (int64_t)SB ? (a.B - b0) : (int64_t)SB);  // rows of this workgroup
    if (b < a.B) {
        int64_t r = a.idx ? a.idx[b] : b;
        r = r < 0 ? 0 : (r >= a.n_rows ? a.n_rows - 1 : r);  // ncw_batch_assemble's clamp
        const uint2 w = *reinterpret_cast<const uint2*>(a.recs + r);  // the record as one 8-byte load
        // the image whose range holds r: the LAST k with row_start[k] <= r (an image without a record repeats the previous start,
        // so the first such k may be an empty one).  Invariant: row_start[lo] <= r < row_start[hi].
        int lo = 0, hi = a.n_img;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.row_start[mid] <= r) lo = mid; else hi = mid;
        }
        const NcwSourceImage im = a.images[lo];
        const int pix = (int)(w.x & 0x7fffffffu);
        const int row = pix / im.cam.width, col = pix - row * im.cam.width;
        float o[3], dn[3];
        row_ray(im.cam, row, col, o, dn);
        float near = im.cam.near, far = im.cam.far;
        if (a.use_range) row_range_near_far(o, dn, a.range, a.voxel_size, near, far);
        float depth = 0.f, weight = 0.f;
        if ((w.x >> 31) && a.kp_pix != nullptr) {
            // lower bound of pix in the image's segment of the key-point table
            int64_t klo = a.kp_start[lo], khi = a.kp_start[lo + 1];
            const int64_t kend = khi;
            while (klo < khi) {
                const int64_t mid = (klo + khi) >> 1;
                if (a.kp_pix[mid] < pix) klo = mid + 1; else khi = mid;
            }
            if (klo < kend && a.kp_pix[klo] == pix) {
                depth = a.kp_depth[klo];
                weight = a.kp_weight[klo];
            }
        }
        float* q = s_row + threadIdx.x * RAYC;
        q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
        q[3] = dn[0]; q[4] = dn[1]; q[5] = dn[2];
        q[6] = near; q[7] = far;
        q[8] = depth; q[9] = weight;
        q[10] = 0.f;  // the column the training batch carries but nothing reads
        s_rgb[3 * threadIdx.x] = row_rgb((uint8_t)(w.y & 0xffu));
        s_rgb[3 * threadIdx.x + 1] = row_rgb((uint8_t)((w.y >> 8) & 0xffu));
        s_rgb[3 * threadIdx.x + 2] = row_rgb((uint8_t)((w.y >> 16) & 0xffu));
        a.ts[b] = (int64_t)im.ts;
        const int64_t lab = a.with_semantics ? (int64_t)(w.y >> 24) : 0;
        if (a.label) a.label[b] = lab;
        if (a.keep) {
            bool k = true;
            if (a.with_semantics) {
                if (a.n_ids > 0 && lab == a.ids.x) k = false;
                if (a.n_ids > 1 && lab == a.ids.y) k = false;
                if (a.n_ids > 2 && lab == a.ids.z) k = false;
                if (a.n_ids > 3 && lab == a.ids.w) k = false;
            }
            a.keep[b] = k ? 1 : 0;
        }
    }
    __syncthreads();
    {
        const int total = nb * RAYC, vec = total >> 2;
        float* dst = a.rays + b0 * RAYC;  // b0 * 44 bytes is a multiple of 16 (b0 is a multiple of 256)
        for (int t = threadIdx.x; t < vec; t += SB) reinterpret_cast<f32x4*>(dst)[t] = reinterpret_cast<const f32x4*>(s_row)[t];
        for (int t = 4 * vec + threadIdx.x; t < total; t += SB) dst[t] = s_row[t];
    }
    if (a.rgbs) {
        const int total = nb * 3, vec = total >> 2;
        float* dst = a.rgbs + b0 * 3;
        for (int t = threadIdx.x; t < vec; t += SB) reinterpret_cast<f32x4*>(dst)[t] = reinterpret_cast<const f32x4*>(s_rgb)[t];
        for (int t = 4 * vec + threadIdx.x; t < total; t += SB) dst[t] = s_rgb[t];
    }
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline bool octree_ok(const NcwCacheOctree* t) { return t->occ != nullptr && t->brick != nullptr && t->level >= 3 && t->level <= 10 && t->scale > 0.f; }

}  // namespace

extern "C" int ncw_source_batch(const NcwSourceRec* recs, int64_t n_rows, const NcwSourceImage* images, const int64_t* row_start,
                                const int64_t* kp_start, int n_img, const int32_t* kp_pix, const float* kp_depth,
                                const float* kp_weight, const NcwCacheOctree* range, float voxel_size, const int64_t* idx, int64_t B,
                                int with_semantics, float* rays, int64_t* ts, int64_t* label, float* rgbs, const int* mask_ids,
                                int n_ids, uint8_t* keep, void* stream) {
    if (B <= 0) return 0;
    if (!recs || !images || !row_start || !kp_start || !rays || !ts || n_rows <= 0 || n_img <= 0) return NCW_E_BADARG;
    if (n_ids < 0 || n_ids > 4 || (n_ids > 0 && !mask_ids)) return NCW_E_BADARG;
    if ((B + SB - 1) / SB > 0x7fffffffLL) return NCW_E_BADARG;
    if (!aligned_to(recs, 8) || !aligned_to(images, 4) || !aligned_to(row_start, 8) || !aligned_to(kp_start, 8) ||
        !aligned_to(idx, 8) || !aligned_to(ts, 8) || !aligned_to(label, 8) || !aligned_to(rays, 16) || !aligned_to(rgbs, 16))
        return NCW_E_BADARG;  // 8-byte record loads, 16-byte row stores
    const bool kp_any = kp_pix || kp_depth || kp_weight;
    if (kp_any && (!kp_pix || !kp_depth || !kp_weight || !aligned_to(kp_pix, 4) || !aligned_to(kp_depth, 4) || !aligned_to(kp_weight, 4)))
        return NCW_E_BADARG;
    if (range != nullptr && !octree_ok(range)) return NCW_E_BADARG;
    SourceArgs a;
    a.recs = recs;
    a.n_rows = n_rows;
    a.images = images;
    a.row_start = row_start;
    a.kp_start = kp_start;
    a.n_img = n_img;
    a.kp_pix = kp_pix;
    a.kp_depth = kp_depth;
    a.kp_weight = kp_weight;
    a.use_range = range != nullptr ? 1 : 0;
    a.range = a.use_range ? *range : NcwCacheOctree{};
    a.voxel_size = voxel_size;
    a.idx = idx;
    a.B = B;
    a.with_semantics = with_semantics ? 1 : 0;
    a.rays = rays;
    a.ts = ts;
    a.label = label;
    a.rgbs = rgbs;
    a.ids = make_int4(n_ids > 0 ? mask_ids[0] : -1, n_ids > 1 ? mask_ids[1] : -1, n_ids > 2 ? mask_ids[2] : -1,
                      n_ids > 3 ? mask_ids[3] : -1);
    a.n_ids = n_ids;
    a.keep = keep;
    hipLaunchKernelGGL(source_batch_kernel, dim3((unsigned)((B + SB - 1) / SB)), dim3(SB), 0, (hipStream_t)stream, a);
    NCW_CHECK_LAUNCH();
    return 0;
}
