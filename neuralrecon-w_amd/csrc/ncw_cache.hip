// The training ray cache, one image at a time (include/neuconw_hip.h, "Ray cache"): what the reference's dataset does per image on
// its way to `all_rays` / `all_rgbs` (datasets/phototourism.py:150-209, 557-657) --
//   ncw_sfm_depth_splat   get_colmap_depth: the SfM key-points of the image as a depth plane and a weight plane
//   ncw_cache_rows        the finished cache rows of a pixel range: rays, near / far from the two SfM octrees, image id, label,
//                         key-point depth and weight, the rgb row and the keep flag of `rays[valid_mask]`
// Row width: the reference's code concatenates 12 columns with labels (11 without) while its comment says 13 and its reader slices
// [10:13] (phototourism.py:611-636, 716-724); ncw_batch_assemble and raycache.RayCache take the documented 13 / 12, so the rows
// written here are the reference's columns plus one zero column at the end, which nothing reads.
// The reference traces the octrees in 100 k-ray chunks with a .cpu() each, concatenates 13 columns on the host and indexes with a
// boolean mask there; here one launch per image writes the rows and only the kept ones leave the device.
// Per-pixel kernels: memory- and walk-bound, no MFMA.  No float atomics: bitwise reproducible run to run.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_rowmath.h"

#include <math.h>

namespace {

constexpr int CB = 256;  // threads per workgroup
constexpr int MAXC = 13; // columns of a row with labels

// ---------------------------------------------------------------------------------------------
// key-point depth planes.  Collisions: the key-point LATEST in images.bin order wins (what numpy / torch-CPU assignment with
// repeated indices does; the reference's CUDA assignment is unordered).  Pass 1 takes the largest key-point index per pixel
// with an integer atomicMax, pass 2 lets exactly that key-point write.
// ---------------------------------------------------------------------------------------------
NCW_DEV int64_t splat_pixel(const int32_t* __restrict__ px, int64_t i, int width, int height) {
    const int col = px[2 * i], row = px[2 * i + 1];
    if (col < 0 || col >= width || row < 0 || row >= height) return -1;
    return (int64_t)row * width + col;
}

__global__ __launch_bounds__(CB) void splat_winner_kernel(const int32_t* __restrict__ px, int64_t n, int width, int height,
                                                          int32_t* __restrict__ winner) {
    const int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x;
    if (i >= n) return;
    const int64_t p = splat_pixel(px, i, width, height);
    if (p >= 0) atomicMax(&winner[p], (int32_t)i);
}

struct SplatPose {
    float z[4];  // third row of the world -> camera matrix: camera-space z = z[0] x + z[1] y + z[2] z + z[3]
};

__global__ __launch_bounds__(CB) void splat_write_kernel(const float* __restrict__ xyz, const float* __restrict__ err,
                                                         const int32_t* __restrict__ px, int64_t n, double err_mean, SplatPose pose,
                                                         int width, int height, const int32_t* __restrict__ winner,
                                                         float* __restrict__ depth_z, float* __restrict__ weight) {
    const int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x;
    if (i >= n) return;
    const int64_t p = splat_pixel(px, i, width, height);
    if (p < 0 || winner[p] != (int32_t)i) return;
    // a few thousand key-points per image: f64 costs nothing here and leaves one rounding per value
    const double z = (double)pose.z[0] * xyz[3 * i] + (double)pose.z[1] * xyz[3 * i + 1] + (double)pose.z[2] * xyz[3 * i + 2] +
                     (double)pose.z[3];
    const double q = (double)err[i] / err_mean;
    depth_z[p] = (float)z;  // may be negative (a point behind the camera): written anyway, as the reference does
    weight[p] = (float)(2.0 * exp(-(q * q)));
}

// ---------------------------------------------------------------------------------------------
// cache rows
// ---------------------------------------------------------------------------------------------
struct RowArgs {
    NcwViewCamera cam;
    const uint8_t* image;   // [h, w, 3]
    const uint8_t* label;   // [hs, ws] or NULL
    int label_h, label_w;
    const float* depth_z;   // [h * w]
    const float* weight;    // [h * w]
    float ts, voxel_size;
    int use_voxel;
    NcwCacheOctree hit, range;
    int64_t p0, n;
    int ncols;
    float* rows;
    float* rgbs;
    uint8_t* keep;
};

// One thread per pixel.  The row and the rgb triple go through LDS so that the workgroup writes its CB rows -- contiguous, and
// starting at a multiple of 16 bytes whatever ncols is -- as 16-byte stores (a 13-column row alone is only 4-byte aligned).
__global__ __launch_bounds__(CB) void cache_rows_kernel(RowArgs a) {
    __shared__ __attribute__((aligned(16))) float s_row[CB * MAXC];
    __shared__ __attribute__((aligned(16))) float s_rgb[CB * 3];
    const int64_t i0 = (int64_t)blockIdx.x * CB;
    const int64_t i = i0 + threadIdx.x;
    const int nb = (int)((a.n - i0) < (int64_t)CB ? (a.n - i0) : (int64_t)CB);  // rows of this workgroup
    const int nc = a.ncols;
    if (i < a.n) {
        const int64_t p = a.p0 + i;
        const int row = (int)(p / a.cam.width), col = (int)(p - (int64_t)row * a.cam.width);
        float o[3], dn[3];
        row_ray(a.cam, row, col, o, dn);  // ncw_rowmath.h: shared with ncw_source.hip
        float near = a.cam.near, far = a.cam.far;
        bool kept = true;
        if (a.use_voxel) {
            // phototourism.py:638-657: the hit octree decides which rays stay, the range octree gives their near / far
            float hn, hf;
            ray_voxel_near_far(o, dn, a.hit, hn, hf);
            kept = hn > 0.f;
            if (kept) row_range_near_far(o, dn, a.range, a.voxel_size, near, far);
        }
        // key-point depth along the ray: z * |((col - cx) / fx, (row - cy) / fy, 1)| -- the reference's dir_norm (a rotation keeps
        // the norm).  Only the few key-point pixels take the f64 branch.
        const float dz = a.depth_z[p];
        float depth = 0.f;
        if (dz != 0.f) {
            const double dx = ((double)col - (double)a.cam.cx) / (double)a.cam.fx;
            const double dy = ((double)row - (double)a.cam.cy) / (double)a.cam.fy;
            depth = (float)((double)dz * sqrt(dx * dx + dy * dy + 1.0));
        }
        float* r = s_row + threadIdx.x * nc;
        r[0] = o[0]; r[1] = o[1]; r[2] = o[2];
        r[3] = dn[0]; r[4] = dn[1]; r[5] = dn[2];
        r[6] = near; r[7] = far;
        r[8] = a.ts;
        int c = 9;
        if (a.label != nullptr) {
            // nearest sample of the label map at its own size: stands in for cv2.resize(..., INTER_NEAREST) (phototourism.py:601-608).
            // Parity with cv2's own rounding is unpinned (cv2 is not a dependency), like the JET table of views.py.
            int lr = (int)(((int64_t)row * a.label_h) / a.cam.height), lc = (int)(((int64_t)col * a.label_w) / a.cam.width);
            lr = lr < a.label_h - 1 ? lr : a.label_h - 1;
            lc = lc < a.label_w - 1 ? lc : a.label_w - 1;
            r[c++] = (float)a.label[(int64_t)lr * a.label_w + lc];
        }
        r[c] = depth;
        r[c + 1] = a.weight[p];
        r[c + 2] = 0.f;  // the column the training batch carries but nothing reads (ncw_batch_assemble: rays[:, 10])
        const uint8_t* px = a.image + 3 * p;
        s_rgb[3 * threadIdx.x] = row_rgb(px[0]);
        s_rgb[3 * threadIdx.x + 1] = row_rgb(px[1]);
        s_rgb[3 * threadIdx.x + 2] = row_rgb(px[2]);
        a.keep[i] = kept ? 1 : 0;
    }
    __syncthreads();
    {
        const int total = nb * nc, vec = total >> 2;
        float* dst = a.rows + i0 * nc;  // i0 * nc * 4 bytes is a multiple of 16 (i0 is a multiple of 256)
        for (int t = threadIdx.x; t < vec; t += CB) reinterpret_cast<f32x4*>(dst)[t] = reinterpret_cast<const f32x4*>(s_row)[t];
        for (int t = 4 * vec + threadIdx.x; t < total; t += CB) dst[t] = s_row[t];
    }
    {
        const int total = nb * 3, vec = total >> 2;
        float* dst = a.rgbs + i0 * 3;
        for (int t = threadIdx.x; t < vec; t += CB) reinterpret_cast<f32x4*>(dst)[t] = reinterpret_cast<const f32x4*>(s_rgb)[t];
        for (int t = 4 * vec + threadIdx.x; t < total; t += CB) dst[t] = s_rgb[t];
    }
}

inline bool grid_fits(int64_t n) { return (n + CB - 1) / CB <= 0x7fffffffLL; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool octree_ok(const NcwCacheOctree* t) { return t->occ != nullptr && t->brick != nullptr && t->level >= 3 && t->level <= 10 && t->scale > 0.f; }

}  // namespace

extern "C" int ncw_sfm_depth_splat(const float* xyz, const float* err, const int32_t* px, int64_t n, double err_mean,
                                   const float* w2c_host, int width, int height, int32_t* winner, float* depth_z, float* weight,
                                   void* stream) {
    if (width < 1 || height < 1 || n < 0 || n > 0x7fffffffLL || !winner || !depth_z || !weight) return NCW_E_BADARG;
    if (!aligned4(winner) || !aligned4(depth_z) || !aligned4(weight)) return NCW_E_BADARG;
    if (n > 0 && (!xyz || !err || !px || !w2c_host || !aligned4(xyz) || !aligned4(err) || !aligned4(px) || !(err_mean > 0.0)))
        return NCW_E_BADARG;
    const size_t hw = (size_t)width * height;
    hipStream_t s = (hipStream_t)stream;
    // fills, not kernels: the planes are zero where no key-point lands, also for n == 0
    if (hipMemsetAsync(winner, 0xff, hw * sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(depth_z, 0, hw * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(weight, 0, hw * sizeof(float), s) != hipSuccess)
        return NCW_E_BADARG;
    if (n == 0) return 0;
    SplatPose pose;
    for (int k = 0; k < 4; ++k) pose.z[k] = w2c_host[8 + k];
    const dim3 grid((unsigned)((n + CB - 1) / CB));
    hipLaunchKernelGGL(splat_winner_kernel, grid, dim3(CB), 0, s, px, n, width, height, winner);
    hipLaunchKernelGGL(splat_write_kernel, grid, dim3(CB), 0, s, xyz, err, px, n, err_mean, pose, width, height,
                       (const int32_t*)winner, depth_z, weight);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_cache_rows(const NcwViewCamera* cam, const uint8_t* image, const uint8_t* label, int label_h, int label_w,
                              const float* depth_z, const float* weight, int image_id, float voxel_size, const NcwCacheOctree* hit,
                              const NcwCacheOctree* range, int64_t p0, int64_t n, int ncols, float* rows, float* rgbs,
                              uint8_t* keep, void* stream) {
    if (cam == nullptr || cam->width < 1 || cam->height < 1 || p0 < 0 || n < 0 || p0 + n > (int64_t)cam->width * cam->height ||
        !grid_fits(n))
        return NCW_E_BADARG;
    if (ncols != (label != nullptr ? 13 : 12)) return NCW_E_BADARG;
    if (label != nullptr && (label_h < 1 || label_w < 1)) return NCW_E_BADARG;
    if ((hit != nullptr && !octree_ok(hit)) || (range != nullptr && !octree_ok(range))) return NCW_E_BADARG;
    if (n == 0) return 0;
    if (!image || !depth_z || !weight || !rows || !rgbs || !keep) return NCW_E_BADARG;
    if (!aligned16(rows) || !aligned16(rgbs) || !aligned4(depth_z) || !aligned4(weight)) return NCW_E_BADARG;  // 16-byte row stores
    RowArgs a;
    a.cam = *cam;
    a.image = image;
    a.label = label;
    a.label_h = label_h;
    a.label_w = label_w;
    a.depth_z = depth_z;
    a.weight = weight;
    a.ts = (float)image_id;  // id_ * torch.ones(...) (phototourism.py:562)
    a.voxel_size = voxel_size;
    a.use_voxel = (hit != nullptr && range != nullptr) ? 1 : 0;  // either octree missing: use_voxel = False
    a.hit = a.use_voxel ? *hit : NcwCacheOctree{};
    a.range = a.use_voxel ? *range : NcwCacheOctree{};
    a.p0 = p0;
    a.n = n;
    a.ncols = ncols;
    a.rows = rows;
    a.rgbs = rgbs;
    a.keep = keep;
    hipLaunchKernelGGL(cache_rows_kernel, dim3((unsigned)((n + CB - 1) / CB)), dim3(CB), 0, (hipStream_t)stream, a);
    NCW_CHECK_LAUNCH();
    return 0;
}
