// Whole-view rendering glue and image metrics (include/neuconw_hip.h, "Camera views"): everything around the forward-only
// render of one camera view that the reference does with torch.cat / .cpu() / numpy / cv2 --
//   ncw_view_rays      datasets/ray_utils.py:18-52 + datasets/phototourism.py:769-782   (rays of a pixel range)
//   ncw_view_store     lightning_modules/neuconw_system.py:440-460                      (chunk outputs -> planar images)
//   ncw_image_minmax / ncw_depth_colormap   utils/visualization.py:13-25               (depth colour map)
//   ncw_image_sqerr    metrics.py:5-14                                                  (MSE / PSNR)
//   ncw_image_ssim     metrics.py:16-21 over kornia's ssim                              (SSIM)
// Per-pixel / per-ray kernels: memory-bound, no MFMA.  Every reduction is two-stage and fixed-order (per-thread strided
// partial -> wave shuffle tree -> LDS across the waves -> one partial per workgroup -> ONE workgroup sums the partials in f64):
// no float atomics, bitwise reproducible run to run.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_raymath.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int VB = 256;            // threads per workgroup of every kernel in this file
constexpr int RED_BLOCKS = 1024;   // most first-stage workgroups of minmax / sqerr (the scratch holds that many partials)

// ---------------------------------------------------------------------------------------------
// fixed-order workgroup reductions (VB = 256 threads = 4 waves); the result is valid on thread 0
// ---------------------------------------------------------------------------------------------
template <class T, class Op>
NCW_DEV T wave_reduce(T v, Op op) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = op(v, __shfl_xor(v, m, 64));
    return v;
}
template <class T, class Op>
NCW_DEV T block_reduce(T v, T* lds, Op op) {
    v = wave_reduce(v, op);
    __syncthreads();  // lds may still be read by a previous reduction
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = lds[0];
#pragma unroll
    for (int w = 1; w < VB / 64; ++w) r = op(r, lds[w]);
    return r;
}
struct OpAdd {
    template <class T> NCW_DEV T operator()(T a, T b) const { return a + b; }
};
struct OpMin {
    NCW_DEV float operator()(float a, float b) const { return a < b ? a : b; }
};
struct OpMax {
    NCW_DEV float operator()(float a, float b) const { return a > b ? a : b; }
};

// np.nan_to_num (utils/visualization.py:18): NaN -> 0, +-inf -> +-FLT_MAX
NCW_DEV float nan_to_num(float x) {
    if (x != x) return 0.f;
    if (x > FLT_MAX) return FLT_MAX;
    if (x < -FLT_MAX) return -FLT_MAX;
    return x;
}

// ---------------------------------------------------------------------------------------------
// rays
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VB) void view_rays_kernel(NcwViewCamera cam, int64_t p0, int64_t n, float* __restrict__ rays) {
    const int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x;
    if (i >= n) return;
    const int64_t p = p0 + i;
    const int row = (int)(p / cam.width), col = (int)(p - (int64_t)row * cam.width);
    float d[3];
    const float nrm = view_ray_dir(cam, row, col, d);
    f32x4 a = {cam.c2w[3], cam.c2w[7], cam.c2w[11], d[0] / nrm};
    f32x4 b = {d[1] / nrm, d[2] / nrm, cam.near, cam.far};
    f32x4* o = reinterpret_cast<f32x4*>(rays + 8 * i);  // rays is 16-byte aligned (checked by the entry point); rows are 32 bytes
    o[0] = a;
    o[1] = b;
}

// ---------------------------------------------------------------------------------------------
// chunk outputs -> planar images
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VB) void view_store_kernel(const float* __restrict__ color, const float* __restrict__ depth,
                                                        const float* __restrict__ normals, int64_t p0, int64_t n, int64_t hw,
                                                        float* __restrict__ color_img, float* __restrict__ depth_img,
                                                        float* __restrict__ normal_img) {
    const int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x;
    if (i >= n) return;
    const int64_t p = p0 + i;
    if (color != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) color_img[c * hw + p] = color[3 * i + c];
    }
    if (depth != nullptr) depth_img[p] = depth[i];
    if (normals != nullptr) {
        const float x = normals[3 * i], y = normals[3 * i + 1], z = normals[3 * i + 2];
        const float nrm = sqrtf(x * x + y * y + z * z);  // torch.linalg.norm; 0 / 0 stays NaN (neuconw_system.py:459)
        normal_img[p] = x / nrm / 2.f + 0.5f;
        normal_img[hw + p] = y / nrm / 2.f + 0.5f;
        normal_img[2 * hw + p] = z / nrm / 2.f + 0.5f;
    }
}

// ---------------------------------------------------------------------------------------------
// min / max after nan_to_num
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VB) void minmax_stage1(const float* __restrict__ x, int64_t n, float* __restrict__ part) {
    __shared__ float lds[VB / 64];
    float mi = FLT_MAX, ma = -FLT_MAX;
    for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) {
        const float v = nan_to_num(x[i]);
        mi = v < mi ? v : mi;
        ma = v > ma ? v : ma;
    }
    mi = block_reduce(mi, lds, OpMin());
    ma = block_reduce(ma, lds, OpMax());
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = mi;
        part[2 * blockIdx.x + 1] = ma;
    }
}
__global__ __launch_bounds__(VB) void minmax_stage2(const float* __restrict__ part, int nb, float* __restrict__ out) {
    __shared__ float lds[VB / 64];
    float mi = FLT_MAX, ma = -FLT_MAX;
    for (int i = threadIdx.x; i < nb; i += VB) {
        mi = part[2 * i] < mi ? part[2 * i] : mi;
        ma = part[2 * i + 1] > ma ? part[2 * i + 1] : ma;
    }
    mi = block_reduce(mi, lds, OpMin());
    ma = block_reduce(ma, lds, OpMax());
    if (threadIdx.x == 0) {
        out[0] = mi;
        out[1] = ma;
    }
}

// utils/visualization.py:18-23 per pixel: index = uint8(255 * (x - mi) / (ma - mi + 1e-8)), all in f32 with IEEE division
__global__ __launch_bounds__(VB) void colormap_kernel(const float* __restrict__ depth, int64_t n, const float* __restrict__ minmax,
                                                      const uint8_t* __restrict__ lut, float* __restrict__ out_f32,
                                                      uint8_t* __restrict__ out_u8, uint8_t* __restrict__ out_index) {
    const int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x;
    if (i >= n) return;
    const float mi = minmax[0], ma = minmax[1];
    const float den = (ma - mi) + 1e-8f;
    const float x = (nan_to_num(depth[i]) - mi) / den;
    const float s = 255.f * x;
    int k = (s == s) ? (int)s : 0;  // inf / inf (an image holding +inf AND -inf): NaN -> 0
    k = k < 0 ? 0 : (k > 255 ? 255 : k);
    if (out_index != nullptr) out_index[i] = (uint8_t)k;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t v = lut[3 * k + c];
        if (out_f32 != nullptr) out_f32[c * n + i] = (float)v / 255.f;  // torchvision ToTensor: value / 255
        if (out_u8 != nullptr) out_u8[c * n + i] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// squared error
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VB) void sqerr_stage1(const float* __restrict__ pred, const float* __restrict__ gt,
                                                   const uint8_t* __restrict__ mask, int64_t n, int64_t pix_stride,
                                                   int64_t ch_stride, float* __restrict__ part_sum, int64_t* __restrict__ part_cnt) {
    __shared__ float lds_f[VB / 64];
    __shared__ int lds_i[VB / 64];
    float s = 0.f;
    int cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) {
        if (mask != nullptr && mask[i] == 0) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = pred[i * pix_stride + c * ch_stride] - gt[i * pix_stride + c * ch_stride];
            s += d * d;
        }
        cnt += 3;
    }
    s = block_reduce(s, lds_f, OpAdd());
    cnt = block_reduce(cnt, lds_i, OpAdd());
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = s;
        part_cnt[blockIdx.x] = cnt;
    }
}
__global__ __launch_bounds__(VB) void sqerr_stage2(const float* __restrict__ part_sum, const int64_t* __restrict__ part_cnt, int nb,
                                                   float* __restrict__ sum_out, int64_t* __restrict__ count_out) {
    __shared__ double lds_d[VB / 64];
    __shared__ long long lds_l[VB / 64];
    double s = 0.0;
    long long cnt = 0;
    for (int i = threadIdx.x; i < nb; i += VB) {
        s += (double)part_sum[i];
        cnt += (long long)part_cnt[i];
    }
    s = block_reduce(s, lds_d, OpAdd());
    cnt = block_reduce(cnt, lds_l, OpAdd());
    if (threadIdx.x == 0) {
        sum_out[0] = (float)s;
        count_out[0] = (int64_t)cnt;
    }
}

// ---------------------------------------------------------------------------------------------
// SSIM: one 32 x 32 output tile per workgroup, its inputs with a halo of (w - 1) / 2 <= 5 in LDS, both passes of the
// separable Gaussian in LDS
// ---------------------------------------------------------------------------------------------
constexpr int ST = 32;                 // output tile side
constexpr int SPAD = 5;                // largest halo (window 11)
constexpr int SIN = ST + 2 * SPAD;     // 42
struct SsimWin {
    float g[2 * SPAD + 1];
    int pad;
};

NCW_DEV int reflect(int i, int n) {  // F.pad(mode="reflect"): -k -> k, n - 1 + k -> n - 1 - k (k < n, checked by the host)
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);  // tiles past a ragged edge load (and never use) in-bounds values
}

// the reference's ssim_map (kornia) from the five filtered moments, clamped to [-1, 1]: 1 - 2 clamp((1 - map) / 2, 0, 1) of
// metrics.py:20-21 is clamp(map, -1, 1) (NOT [0, 1]: noisy images do produce negative map values).  No FMA contraction here: with
// identical images numerator and denominator must be the SAME float, so that the map is exactly 1.
NCW_DEV float ssim_value(float mx, float my, float exx, float eyy, float exy) {
#pragma clang fp contract(off)
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float mxx = mx * mx, myy = my * my, mxy = mx * my;
    const float sx = exx - mxx, sy = eyy - myy, sxy = exy - mxy;
    const float num = (2.f * mxy + C1) * (2.f * sxy + C2);
    const float den = (mxx + myy + C1) * (sx + sy + C2);
    const float v = num / den;
    return v < -1.f ? -1.f : (v > 1.f ? 1.f : v);  // a NaN stays a NaN, as torch.clamp keeps it
}

__global__ __launch_bounds__(VB) void ssim_stage1(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W,
                                                  int tiles_x, int tiles_y, SsimWin win, float* __restrict__ part) {
    __shared__ float xt[SIN * SIN], yt[SIN * SIN];
    __shared__ float hp[5][SIN * ST];
    __shared__ float lds[VB / 64];
    const int pad = win.pad, in = ST + 2 * pad;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, ch = b / tiles_y;
    const float* xp = pred + (size_t)ch * H * W;
    const float* yp = gt + (size_t)ch * H * W;
    const int r0 = ty * ST - pad, c0 = tx * ST - pad;
    for (int t = threadIdx.x; t < in * in; t += VB) {
        const int r = t / in, c = t - r * in;
        const size_t src = (size_t)reflect(r0 + r, H) * W + reflect(c0 + c, W);
        xt[r * SIN + c] = xp[src];
        yt[r * SIN + c] = yp[src];
    }
    __syncthreads();
    // horizontal pass: five moments for every input row of the tile
    for (int t = threadIdx.x; t < in * ST; t += VB) {
        const int r = t / ST, c = t - r * ST;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
        for (int k = 0; k <= 2 * pad; ++k) {
            const float g = win.g[k], x = xt[r * SIN + c + k], y = yt[r * SIN + c + k];
            const float xx = x * x, yy = y * y, xy = x * y;
            a0 += g * x;
            a1 += g * y;
            a2 += g * xx;
            a3 += g * yy;
            a4 += g * xy;
        }
        hp[0][t] = a0;
        hp[1][t] = a1;
        hp[2][t] = a2;
        hp[3][t] = a3;
        hp[4][t] = a4;
    }
    __syncthreads();
    // vertical pass + the map; a thread's pixels are summed in a fixed order
    float s = 0.f;
    for (int t = threadIdx.x; t < ST * ST; t += VB) {
        const int r = t / ST, c = t - r * ST;
        if (ty * ST + r >= H || tx * ST + c >= W) continue;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
        for (int k = 0; k <= 2 * pad; ++k) {
            const float g = win.g[k];
            const int q = (r + k) * ST + c;
            a0 += g * hp[0][q];
            a1 += g * hp[1][q];
            a2 += g * hp[2][q];
            a3 += g * hp[3][q];
            a4 += g * hp[4][q];
        }
        s += ssim_value(a0, a1, a2, a3, a4);
    }
    s = block_reduce(s, lds, OpAdd());
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(VB) void ssim_stage2(const float* __restrict__ part, int nb, double count, float* __restrict__ out) {
    __shared__ double lds_d[VB / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += VB) s += (double)part[i];
    s = block_reduce(s, lds_d, OpAdd());
    if (threadIdx.x == 0) out[0] = (float)(s / count);
}

inline int red_blocks(int64_t n) {
    const int64_t nb = (n + VB - 1) / VB;
    return nb < 1 ? 1 : (nb > RED_BLOCKS ? RED_BLOCKS : (int)nb);
}
inline bool grid_fits(int64_t n) { return (n + VB - 1) / VB <= 0x7fffffffLL; }

}  // namespace

extern "C" int ncw_view_rays(const NcwViewCamera* cam, int64_t p0, int64_t n, float* rays, void* stream) {
    if (cam == nullptr || cam->width < 1 || cam->height < 1 || p0 < 0 || n < 0 || p0 + n > (int64_t)cam->width * cam->height ||
        !grid_fits(n))
        return -1;
    if (n == 0) return 0;
    if (rays == nullptr || (reinterpret_cast<uintptr_t>(rays) & 15) != 0) return -1;  // rows are written as two 16-byte stores
    hipLaunchKernelGGL(view_rays_kernel, dim3((unsigned)((n + VB - 1) / VB)), dim3(VB), 0, (hipStream_t)stream, *cam, p0, n, rays);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_view_store(const float* color, const float* depth, const float* normals, int64_t p0, int64_t n, int64_t n_pix,
                              float* color_img, float* depth_img, float* normal_img, void* stream) {
    if (p0 < 0 || n < 0 || p0 + n > n_pix || !grid_fits(n)) return -1;
    if ((color != nullptr && color_img == nullptr) || (depth != nullptr && depth_img == nullptr) ||
        (normals != nullptr && normal_img == nullptr))
        return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(view_store_kernel, dim3((unsigned)((n + VB - 1) / VB)), dim3(VB), 0, (hipStream_t)stream, color, depth, normals,
                       p0, n, n_pix, color_img, depth_img, normal_img);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t ncw_image_reduce_scratch_bytes(void) { return (int64_t)RED_BLOCKS * 16; }

extern "C" int ncw_image_minmax(const float* x, int64_t n, void* scratch, float* minmax, void* stream) {
    if (n < 1 || x == nullptr || scratch == nullptr || minmax == nullptr) return -1;
    const int nb = red_blocks(n);
    float* part = static_cast<float*>(scratch);
    hipLaunchKernelGGL(minmax_stage1, dim3(nb), dim3(VB), 0, (hipStream_t)stream, x, n, part);
    hipLaunchKernelGGL(minmax_stage2, dim3(1), dim3(VB), 0, (hipStream_t)stream, (const float*)part, nb, minmax);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_depth_colormap(const float* depth, int64_t n, const float* minmax, const uint8_t* lut, float* out_f32,
                                  uint8_t* out_u8, uint8_t* out_index, void* stream) {
    if (n < 0 || !grid_fits(n)) return -1;
    if (n == 0) return 0;
    if (depth == nullptr || minmax == nullptr || lut == nullptr) return -1;
    hipLaunchKernelGGL(colormap_kernel, dim3((unsigned)((n + VB - 1) / VB)), dim3(VB), 0, (hipStream_t)stream, depth, n, minmax, lut,
                       out_f32, out_u8, out_index);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_image_sqerr(const float* pred, const float* gt, const uint8_t* mask, int64_t n, int planar, void* scratch,
                               float* sum_out, int64_t* count_out, void* stream) {
    if (n < 0 || scratch == nullptr || sum_out == nullptr || count_out == nullptr) return -1;
    if (n > 0 && (pred == nullptr || gt == nullptr)) return -1;
    const int nb = red_blocks(n);
    float* part_sum = static_cast<float*>(scratch);
    int64_t* part_cnt = reinterpret_cast<int64_t*>(static_cast<char*>(scratch) + (size_t)RED_BLOCKS * 8);
    hipLaunchKernelGGL(sqerr_stage1, dim3(nb), dim3(VB), 0, (hipStream_t)stream, pred, gt, mask, n, planar ? (int64_t)1 : (int64_t)3,
                       planar ? n : (int64_t)1, part_sum, part_cnt);
    hipLaunchKernelGGL(sqerr_stage2, dim3(1), dim3(VB), 0, (hipStream_t)stream, (const float*)part_sum, (const int64_t*)part_cnt, nb,
                       sum_out, count_out);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t ncw_image_ssim_scratch_floats(int channels, int height, int width) {
    if (channels < 1 || height < 1 || width < 1) return 0;
    return (int64_t)channels * ((height + ST - 1) / ST) * ((width + ST - 1) / ST);
}

extern "C" int ncw_image_ssim(const float* pred, const float* gt, int channels, int height, int width, int window, float* scratch,
                              float* ssim_out, void* stream) {
    if (window < 3 || window > 2 * SPAD + 1 || (window & 1) == 0) return -1;
    const int pad = (window - 1) / 2;
    if (channels < 1 || height <= pad || width <= pad) return -2;  // reflect padding is undefined
    if (pred == nullptr || gt == nullptr || scratch == nullptr || ssim_out == nullptr) return -1;
    const int tiles_x = (width + ST - 1) / ST, tiles_y = (height + ST - 1) / ST;
    const int64_t nb = (int64_t)channels * tiles_x * tiles_y;
    if (nb > 0x7fffffffLL) return -1;
    // kornia get_gaussian_kernel1d(window, 1.5): exp(-(i - window // 2)^2 / (2 sigma^2)), normalised
    SsimWin win;
    double g[2 * SPAD + 1], sum = 0.0;
    for (int i = 0; i < window; ++i) {
        const double d = (double)(i - pad);
        g[i] = exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i < 2 * SPAD + 1; ++i) win.g[i] = i < window ? (float)(g[i] / sum) : 0.f;
    win.pad = pad;
    hipLaunchKernelGGL(ssim_stage1, dim3((unsigned)nb), dim3(VB), 0, (hipStream_t)stream, pred, gt, height, width, tiles_x, tiles_y, win,
                       scratch);
    hipLaunchKernelGGL(ssim_stage2, dim3(1), dim3(VB), 0, (hipStream_t)stream, (const float*)scratch, (int)nb,
                       (double)channels * height * width, ssim_out);
    NCW_CHECK_LAUNCH();
    return 0;
}
