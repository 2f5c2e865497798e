// Appearance-code fit on frozen geometry (appfit.py): the two small launches of one fit iteration.
//
// With every network weight frozen and perturb = 0 the sample depths, the SDF values / gradients / features, the NeuS weights and
// the background densities are constants of a ray; only the colour network and the background NeRF's colour head see the
// appearance code, and the rendered colour is LINEAR in their outputs with coefficients the compositor has already written
// (NcwCompositeOut.weights / inside / weights_sum, composite_fwd_kernel).  An iteration is then: colour forward, background forward,
//   ncw_appfit_loss   compose + L1 loss + the adjoints of both colour inputs (one wave per ray, four rays per workgroup)
// the two data-path backwards storing per-point code adjoints (d_a_rows), and
//   ncw_appfit_step   order-fixed sum of those rows into one [n_a] gradient; on the final call the non-finite guard, one Adam
//                     step on the code and its broadcast into the [R, n_a] buffer the forward launches read.
// No atomics anywhere; every result is bitwise run-to-run reproducible.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"
#include "ncw_raymath.h"

namespace {

// the compositor's wave reduction (csrc/ncw_rays.hip wave_sum): same butterfly, same order
NCW_DEV float appfit_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

NCW_DEV float sign0(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }  // torch.sign: sign(0) = 0 (NaN -> 0 as well)

// color = sum_j w_j (inside_j ? rgb_j : bg_rgb_j or 0) + background_rgb (1 - weights_sum): the Q.color expression of
// composite_fwd_kernel, lane-strided over the M merged samples, then wave_sum -- the same order, so the same bits.
__global__ __launch_bounds__(256) void appfit_loss_kernel(const float* __restrict__ weights, const float* __restrict__ inside,
                                                          const float* __restrict__ weights_sum, const float* __restrict__ rgb,
                                                          const float* __restrict__ bg_rgb, const float* __restrict__ background_rgb,
                                                          const float* __restrict__ target, int R, int S, int M, float inv_denom,
                                                          const float* __restrict__ loss_scale, float* __restrict__ color,
                                                          float* __restrict__ ray_loss, float* __restrict__ d_rgb,
                                                          float* __restrict__ d_bg_rgb) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wv;
    if (r >= R) return;
    float cr = 0.f, cg = 0.f, cb = 0.f;
    for (int j = lane; j < M; j += 64) {
        const float w = weights[(size_t)r * M + j];
        float rr, gg, bb;
        bool ins = false;
        if (j < S) ins = inside[(size_t)r * S + j] > 0.f;
        if (ins) {
            const size_t q = ((size_t)r * S + j) * 3;
            rr = rgb[q]; gg = rgb[q + 1]; bb = rgb[q + 2];
        } else if (bg_rgb) {
            const size_t q = ((size_t)r * M + j) * 3;
            rr = bg_rgb[q]; gg = bg_rgb[q + 1]; bb = bg_rgb[q + 2];
        } else rr = gg = bb = 0.f;
        cr += rr * w; cg += gg * w; cb += bb * w;
    }
    cr = appfit_wave_sum(cr); cg = appfit_wave_sum(cg); cb = appfit_wave_sum(cb);
    if (background_rgb) {
        const float wsum = weights_sum[r];
        cr += background_rgb[0] * (1.0f - wsum);
        cg += background_rgb[1] * (1.0f - wsum);
        cb += background_rgb[2] * (1.0f - wsum);
    }
    const float er = cr - target[(size_t)r * 3], eg = cg - target[(size_t)r * 3 + 1], eb = cb - target[(size_t)r * 3 + 2];
    if (lane == 0) {
        color[(size_t)r * 3] = cr; color[(size_t)r * 3 + 1] = cg; color[(size_t)r * 3 + 2] = cb;
        ray_loss[r] = (fabsf(er) + fabsf(eg)) + fabsf(eb);
    }
    // d color_c = scale sign(color_c - target_c) / (R_total + 1e-5); the scale is a power of two (exact)
    const float k = loss_scale ? inv_denom * loss_scale[0] : inv_denom;
    const float gr = sign0(er) * k, gg_ = sign0(eg) * k, gb = sign0(eb) * k;
    for (int j = lane; j < M; j += 64) {
        const float w = weights[(size_t)r * M + j];
        bool ins = false;
        if (j < S) ins = inside[(size_t)r * S + j] > 0.f;
        if (j < S) {
            const size_t q = ((size_t)r * S + j) * 3;
            d_rgb[q] = ins ? w * gr : 0.f; d_rgb[q + 1] = ins ? w * gg_ : 0.f; d_rgb[q + 2] = ins ? w * gb : 0.f;
        }
        if (d_bg_rgb) {
            const size_t q = ((size_t)r * M + j) * 3;
            d_bg_rgb[q] = ins ? 0.f : w * gr; d_bg_rgb[q + 1] = ins ? 0.f : w * gg_; d_bg_rgb[q + 2] = ins ? 0.f : w * gb;
        }
    }
}

// ---- reduction of the per-point code adjoints ----------------------------------------------------------------------------
// Block k owns rows [APPFIT_BLOCK_ROWS k, APPFIT_BLOCK_ROWS (k + 1)) of the buffer: wave w adds its 64 rows in sequence (lane =
// column, so a row is one coalesced read), the four wave sums combine as (w0 + w1) + (w2 + w3).  Absent rows (past n) add nothing.
constexpr int APPFIT_BLOCK_ROWS = NCW_APPFIT_BLOCK_ROWS;
constexpr int APPFIT_MAX_NA = NCW_APPFIT_MAX_NA;

__global__ __launch_bounds__(256) void appfit_partial_kernel(const float* __restrict__ rows, int64_t n, int n_a,
                                                             float* __restrict__ partials) {
    __shared__ float sm[4][APPFIT_MAX_NA];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)blockIdx.x * APPFIT_BLOCK_ROWS + wv * 64;
    const int64_t r1 = r0 + 64 < n ? r0 + 64 : n;
    for (int c = lane; c < n_a; c += 64) {
        float acc = 0.f;
        for (int64_t r = r0; r < r1; ++r) acc += rows[r * n_a + c];
        sm[wv][c] = acc;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n_a; c += 256)
        partials[(size_t)blockIdx.x * n_a + c] = (sm[0][c] + sm[1][c]) + (sm[2][c] + sm[3][c]);
}

// One workgroup: grad_acc[c] = (accumulate ? grad_acc[c] : 0) + partials[0][c] + partials[1][c] + ...  in block order; with `fin`
// the guard, the Adam step (the arithmetic of adam_dev_kernel, csrc/ncw_optim.hip, clip coefficient 1) and the broadcast.
__global__ __launch_bounds__(256) void appfit_final_kernel(const float* __restrict__ partials, int n_blocks, int n_a,
                                                           float* __restrict__ grad_acc, int accumulate, int fin,
                                                           float* __restrict__ code, float* __restrict__ exp_avg,
                                                           float* __restrict__ exp_avg_sq, NcwAdamState* __restrict__ st, float lr,
                                                           float beta1, float beta2, float eps, float* __restrict__ loss_scale,
                                                           float scale_min, float* __restrict__ a_rows, int64_t a_count) {
    __shared__ float s_code[APPFIT_MAX_NA];
    __shared__ float s_step[2];
    const int c = threadIdx.x;
    float g = 0.f;
    if (c < n_a) {
        g = accumulate ? grad_acc[c] : 0.f;
        for (int k = 0; k < n_blocks; ++k) g += partials[(size_t)k * n_a + c];
        grad_acc[c] = g;
    }
    if (!fin) return;
    float gc = 0.f;
    if (c < n_a) gc = loss_scale ? g * loss_scale[1] : g;  // the loss scale divided back out
    const bool finite = gc < __builtin_inff() && gc > -__builtin_inff();  // false for NaN as well
    const int bad = __syncthreads_or((c < n_a && !finite) ? 1 : 0);
    if (bad) {  // nothing is written to the code or its moments; the scale backs off (convention of ncw_adam_step_dev)
        if (c == 0) {
            st->skip_now = 1;
            st->skipped += 1;
            st->good = 0;
            if (loss_scale) {
                const float s = fmaxf(loss_scale[0] * 0.5f, scale_min);
                loss_scale[0] = s;
                loss_scale[1] = 1.f / s;
            }
        }
        return;
    }
    if (c == 0) {
        const int t = st->step + 1;
        st->step = t;
        st->good += 1;
        st->skip_now = 0;
        // torch's _single_tensor_adam computes both corrections in double
        const double bc1 = 1.0 - pow((double)beta1, (double)t);
        const double bc2 = 1.0 - pow((double)beta2, (double)t);
        const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
        st->coef = 1.f;
        st->step_size = step_size;
        st->bc2_sqrt = bc2_sqrt;
        s_step[0] = step_size;
        s_step[1] = bc2_sqrt;
    }
    __syncthreads();
    if (c < n_a) {
        const float step_size = s_step[0], bc2_sqrt = s_step[1];
        const float w1 = 1.f - beta1, w2 = 1.f - beta2;
        const float mi = exp_avg[c] + w1 * (gc - exp_avg[c]);
        const float vi = exp_avg_sq[c] * beta2 + w2 * gc * gc;
        exp_avg[c] = mi;
        exp_avg_sq[c] = vi;
        const float p = code[c] - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
        code[c] = p;
        s_code[c] = p;
    }
    __syncthreads();
    for (int64_t i = threadIdx.x; i < a_count; i += 256) a_rows[i] = s_code[(int)(i % n_a)];
}

}  // namespace

extern "C" int ncw_appfit_loss(const float* weights, const float* inside, const float* weights_sum, const float* rgb,
                               const float* bg_rgb, const float* background_rgb, const float* target, int R, int S, int O,
                               float inv_denom, const float* loss_scale, float* color, float* ray_loss, float* d_rgb,
                               float* d_bg_rgb, void* stream) {
    if (R == 0) return 0;
    if (!weights || !inside || !weights_sum || !rgb || !target || !color || !ray_loss || !d_rgb) return NCW_E_BADARG;
    if (R < 0 || S < 1 || O < 0 || (bg_rgb == nullptr) != (d_bg_rgb == nullptr)) return NCW_E_BADARG;
    const int M = bg_rgb ? S + O : S;  // weights [R, M]: S + O columns with a background, S without
    if ((int64_t)R * M > 0x7fffffffLL / 3) return NCW_E_BADARG;
    hipLaunchKernelGGL(appfit_loss_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, weights, inside,
                       weights_sum, rgb, bg_rgb, background_rgb, target, R, S, M, inv_denom, loss_scale, color, ray_loss, d_rgb,
                       d_bg_rgb);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t ncw_appfit_step_scratch_floats(int64_t n, int n_a) {
    if (n < 0 || n_a < 1) return 0;
    return ((n + APPFIT_BLOCK_ROWS - 1) / APPFIT_BLOCK_ROWS) * (int64_t)n_a;
}

extern "C" int ncw_appfit_step(const float* d_a_rows, int64_t n, int n_a, float* scratch, float* grad_acc, int accumulate,
                               int final_call, float* code, float* exp_avg, float* exp_avg_sq, NcwAdamState* state, float lr,
                               float beta1, float beta2, float eps, float* loss_scale, float scale_min, float* a_rows,
                               int64_t R_rows, void* stream) {
    if (n_a < 1 || n_a > APPFIT_MAX_NA || n < 0 || !grad_acc) return NCW_E_BADARG;
    if (n > 0 && (!d_a_rows || !scratch)) return NCW_E_BADARG;
    if (final_call && (!code || !exp_avg || !exp_avg_sq || !state || R_rows < 0 || (R_rows > 0 && !a_rows))) return NCW_E_BADARG;
    const int64_t n_blocks = (n + APPFIT_BLOCK_ROWS - 1) / APPFIT_BLOCK_ROWS;
    if (n_blocks > 0x7fffffffLL) return NCW_E_BADARG;
    if (n_blocks > 0) {
        hipLaunchKernelGGL(appfit_partial_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, d_a_rows, n, n_a,
                           scratch);
        NCW_CHECK_LAUNCH();
    }
    if (n_blocks == 0 && accumulate && !final_call) return 0;  // nothing to add, nothing to finish
    hipLaunchKernelGGL(appfit_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, (int)n_blocks, n_a, grad_acc,
                       accumulate, final_call, code, exp_avg, exp_avg_sq, state, lr, beta1, beta2, eps, loss_scale, scale_min,
                       a_rows, final_call ? R_rows * (int64_t)n_a : 0);
    NCW_CHECK_LAUNCH();
    return 0;
}
