// Synthetic scenes with known ground truth (neuralrecon-w_amd/synth.py): the two per-image passes that turn a triangle mesh into
// what a photo collection and its SfM model give the pipeline.  The reference has nothing of the kind (its scenes are
// downloaded), so nothing here is pinned by it: the contract is the numpy restatement in tests/_synth_ref.py, bit for bit.
//
//   ncw_synth_shade   : one lane per PIXEL of the height x width image: for each of its ss x ss sub-samples of the depth / face
//                       planes of ncw_raster_resolve, camera point -> world (c2w) -> GT frame (sfm2gt), albedo = material colour
//                       times three octaves of hashed value noise (Philox4x32-10 on the integer lattice, trilinear), flat
//                       Lambert with the face's unit normal from the host, per-image gain / bias, clamp; sky where there is no
//                       face; mean over the sub-samples in fixed (j, i) order -> uint8; label and depth of the centre sub-sample.
//   ncw_synth_observe : one lane per POINT: float64 projection, facing test, uniform-sum pixel noise (Philox of the point's index
//                       and the view's serial), visibility against the shaded depth plane.
//
// Pixel convention (pinned by tests/test_gpu_synth.py): the project's rays go through INTEGER pixel coordinates (ncw_view_rays),
// the rasterizer samples at (c + 0.5, r + 0.5).  The caller rasterizes (height ss) x (width ss) samples with fx ss, fy ss,
// cx ss + 0.5 ss, cy ss + 0.5 ss; sub-sample (i, j) of pixel (r, c) then sits at image point (c + (i + 0.5) / ss - 0.5,
// r + (j + 0.5) / ss - 0.5) of the image's own fx, fy, cx, cy, and with ss = 1 exactly on the ray of ncw_view_rays.
//
// No atomics, no LDS, no transcendental function, no square root: every output is a function of its own index, and every
// product, sum and quotient is rounded once (the file is built with -ffp-contract=off, division is IEEE).  What needs a root
// comes from the host: unit normals, sigma sqrt(3); the squared pixel error goes back to it.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_philox.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;

// lattice value at (ix, iy, iz): 24 bits of the first Philox word, in [0, 1)
__device__ __forceinline__ float lattice(int32_t ix, int32_t iy, int32_t iz, uint32_t seed, uint32_t octave) {
    uint32_t w[4] = {(uint32_t)ix, (uint32_t)iy, (uint32_t)iz, seed};
    philox4x32_10(w, octave, 0u);
    return (float)(w[0] >> 8) * 0x1p-24f;
}

__device__ __forceinline__ float lerp1(float a, float b, float t) { return a + t * (b - a); }

// trilinear value noise at q (x first, then y, then z); lattice coordinates clamped to +-2^30 (NaN -> -2^30)
__device__ __forceinline__ float value_noise(float qx, float qy, float qz, uint32_t seed, uint32_t octave) {
    const float lim = 0x1p30f;
    const float fx = fminf(fmaxf(floorf(qx), -lim), lim), fy = fminf(fmaxf(floorf(qy), -lim), lim),
                fz = fminf(fmaxf(floorf(qz), -lim), lim);
    const float tx = qx - fx, ty = qy - fy, tz = qz - fz;
    const int32_t ix = (int32_t)fx, iy = (int32_t)fy, iz = (int32_t)fz;
    const float c00 = lerp1(lattice(ix, iy, iz, seed, octave), lattice(ix + 1, iy, iz, seed, octave), tx);
    const float c10 = lerp1(lattice(ix, iy + 1, iz, seed, octave), lattice(ix + 1, iy + 1, iz, seed, octave), tx);
    const float c01 = lerp1(lattice(ix, iy, iz + 1, seed, octave), lattice(ix + 1, iy, iz + 1, seed, octave), tx);
    const float c11 = lerp1(lattice(ix, iy + 1, iz + 1, seed, octave), lattice(ix + 1, iy + 1, iz + 1, seed, octave), tx);
    return lerp1(lerp1(c00, c10, ty), lerp1(c01, c11, ty), tz);
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__global__ __launch_bounds__(kBlock) void synth_shade_kernel(const float* __restrict__ depth_ss, const int32_t* __restrict__ face_ss,
                                                             NcwSynthImage im, const float* __restrict__ face_normal,
                                                             const uint8_t* __restrict__ face_material, int64_t n_faces,
                                                             const NcwSynthMaterial* __restrict__ materials, int n_materials,
                                                             uint8_t* __restrict__ rgb, uint8_t* __restrict__ label,
                                                             float* __restrict__ depth) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (int64_t)im.height * im.width) return;
    const int r = (int)(p / im.width), c = (int)(p - (int64_t)r * im.width);
    const int ss = im.ss;
    const float fss = (float)ss;
    const int64_t wss = (int64_t)im.width * ss;
    const float trow = (float)r / (float)im.height;
    float sky[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) sky[ch] = clamp01(lerp1(im.sky_top[ch], im.sky_bottom[ch], trow));
    float acc[3] = {0.f, 0.f, 0.f};
    int lab = im.sky_label;
    float dep = 0.f;
    for (int j = 0; j < ss; ++j)
        for (int i = 0; i < ss; ++i) {
            const int64_t s = ((int64_t)r * ss + j) * wss + (int64_t)c * ss + i;
            const float d = depth_ss[s];
            const int32_t f = face_ss[s];
            const bool hit = f >= 0 && (int64_t)f < n_faces && d > 0.f;
            float v[3] = {sky[0], sky[1], sky[2]};
            int l = im.sky_label;
            if (hit) {
                const float px = (float)c + ((float)i + 0.5f) / fss - 0.5f, py = (float)r + ((float)j + 0.5f) / fss - 0.5f;
                const float X = ((px - im.cx) / im.fx) * d, Y = ((py - im.cy) / im.fy) * d;
                float w[3], g[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) w[a] = im.c2w[4 * a] * X + im.c2w[4 * a + 1] * Y + im.c2w[4 * a + 2] * d + im.c2w[4 * a + 3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    g[a] = im.sfm2gt[4 * a] * w[0] + im.sfm2gt[4 * a + 1] * w[1] + im.sfm2gt[4 * a + 2] * w[2] + im.sfm2gt[4 * a + 3];
                const int m = min((int)face_material[f], n_materials - 1);
                const NcwSynthMaterial mat = materials[m];
                float f0 = mat.freq;
                float n = 0.f, wgt = 0.5f;
                for (uint32_t o = 0; o < 3; ++o) {
                    n = n + wgt * value_noise(g[0] * f0, g[1] * f0, g[2] * f0, im.tex_seed, o);
                    f0 = f0 * 2.f;
                    wgt = wgt * 0.5f;
                }
                const float tex = 1.f + mat.amp * (n - 0.4375f);
                const float* nf = face_normal + (int64_t)f * 3;
                const float ndl = nf[0] * im.light[0] + nf[1] * im.light[1] + nf[2] * im.light[2];
                const float lam = im.ambient + im.diffuse * fmaxf(0.f, ndl);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch] = clamp01(im.gain[ch] * ((mat.base[ch] * tex) * lam) + im.bias[ch]);
                l = mat.label;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + v[ch];
            if (j == ss / 2 && i == ss / 2) {
                lab = l;
                dep = hit ? d : 0.f;
            }
        }
    const float cnt = (float)(ss * ss);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[p * 3 + ch] = (uint8_t)(int)((acc[ch] / cnt) * 255.f + 0.5f);
    label[p] = (uint8_t)lab;
    depth[p] = dep;
}

// four 24-bit uniforms of one Philox call, summed left to right, minus 2: in [-2, 2), variance 1 / 3
__device__ __forceinline__ double usum4(uint64_t index, uint32_t serial, uint32_t call, uint32_t k0, uint32_t k1) {
    uint32_t w[4] = {(uint32_t)index, (uint32_t)(index >> 32), serial, call};
    philox4x32_10(w, k0, k1);
    const double u0 = (double)(w[0] >> 8) * 0x1p-24, u1 = (double)(w[1] >> 8) * 0x1p-24, u2 = (double)(w[2] >> 8) * 0x1p-24,
                 u3 = (double)(w[3] >> 8) * 0x1p-24;
    return (((u0 + u1) + u2) + u3) - 2.0;
}

__global__ __launch_bounds__(kBlock) void synth_observe_kernel(const double* __restrict__ pts, const double* __restrict__ nrm,
                                                               const int64_t* __restrict__ index, int64_t n, NcwSynthView v,
                                                               const float* __restrict__ depth, double* __restrict__ xy,
                                                               double* __restrict__ err2, uint8_t* __restrict__ vis) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const double px = pts[t * 3 + 0], py = pts[t * 3 + 1], pz = pts[t * 3 + 2];
    const double x = v.w2c[0] * px + v.w2c[1] * py + v.w2c[2] * pz + v.w2c[3];
    const double y = v.w2c[4] * px + v.w2c[5] * py + v.w2c[6] * pz + v.w2c[7];
    const double z = v.w2c[8] * px + v.w2c[9] * py + v.w2c[10] * pz + v.w2c[11];
    if (!(z > v.znear)) {
        xy[t * 2 + 0] = 0.0;
        xy[t * 2 + 1] = 0.0;
        err2[t] = 0.0;
        vis[t] = 0;
        return;
    }
    const double u = v.fx * (x / z) + v.cx, w = v.fy * (y / z) + v.cy;
    const double facing = nrm[t * 3 + 0] * (v.centre[0] - px) + nrm[t * 3 + 1] * (v.centre[1] - py) + nrm[t * 3 + 2] * (v.centre[2] - pz);
    const uint64_t id = (uint64_t)index[t];
    const double nx = v.sigma_r3 * usum4(id, v.serial, 0u, (uint32_t)v.seed, (uint32_t)(v.seed >> 32));
    const double ny = v.sigma_r3 * usum4(id, v.serial, 1u, (uint32_t)v.seed, (uint32_t)(v.seed >> 32));
    xy[t * 2 + 0] = u + nx;
    xy[t * 2 + 1] = w + ny;
    err2[t] = nx * nx + ny * ny;
    const double cu = floor(u + 0.5), cv = floor(w + 0.5);
    bool seen = facing > 0.0 && cu >= 0.0 && cu < (double)v.width && cv >= 0.0 && cv < (double)v.height;  // NaN: outside
    if (seen) {
        const double d = (double)depth[(int64_t)cv * v.width + (int64_t)cu];
        seen = d > 0.0 && fabs(z - d) <= v.depth_tol * z;
    }
    vis[t] = seen ? 1 : 0;
}

constexpr int64_t kMaxLaunch = (int64_t)0x7fffffffll * kBlock;

}  // namespace

extern "C" int ncw_synth_shade(const float* depth_ss, const int32_t* face_ss, const NcwSynthImage* img, const float* face_normal,
                               const uint8_t* face_material, int64_t n_faces, const NcwSynthMaterial* materials, int32_t n_materials,
                               uint8_t* rgb, uint8_t* label, float* depth, void* stream) {
    if (!depth_ss || !face_ss || !img || !materials || !rgb || !label || !depth || n_faces < 0 ||
        (n_faces > 0 && (!face_normal || !face_material)) || n_materials < 1 || n_materials > 256)
        return NCW_E_BADARG;
    if (img->ss < 1 || img->ss > NCW_SYNTH_MAX_SS || img->height < 1 || img->width < 1 || !(img->fx > 0.f) || !(img->fy > 0.f) ||
        (int64_t)img->height * img->width * img->ss * img->ss >= ((int64_t)1 << 31))
        return NCW_E_BADARG;
    const int64_t n = (int64_t)img->height * img->width;
    hipLaunchKernelGGL(synth_shade_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, depth_ss,
                       face_ss, *img, face_normal, face_material, n_faces, materials, (int)n_materials, rgb, label, depth);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_synth_observe(const double* pts, const double* nrm, const int64_t* index, int64_t n, const NcwSynthView* view,
                                 const float* depth, double* xy, double* err2, uint8_t* vis, void* stream) {
    if (n <= 0) return 0;
    if (!pts || !nrm || !index || !view || !depth || !xy || !err2 || !vis || n > kMaxLaunch) return NCW_E_BADARG;
    if (view->height < 1 || view->width < 1 || (int64_t)view->height * view->width >= ((int64_t)1 << 31) || !(view->fx > 0.0) ||
        !(view->fy > 0.0) || !(view->znear > 0.0) || !(view->sigma_r3 >= 0.0) || !(view->depth_tol >= 0.0))
        return NCW_E_BADARG;
    hipLaunchKernelGGL(synth_observe_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, pts, nrm,
                       index, n, *view, depth, xy, err2, vis);
    NCW_CHECK_LAUNCH();
    return 0;
}
