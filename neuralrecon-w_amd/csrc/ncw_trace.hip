// Sphere tracing of the SDF's zero level set (include/neuconw_hip.h, "Surface views by sphere tracing"; not in the reference):
//   ncw_trace_begin   per-ray record + the first active list and its points
//   ncw_trace_step    one evaluation of the per-ray recurrence + the next active list and its points
//   ncw_trace_finish  record -> t / state / iters / points
//   ncw_trace_store   a chunk's results -> planar images
// The SDF is evaluated between the launches by the value path (ncw_sdf_infer).  Per-ray kernels: memory-bound, no MFMA.
// The recurrence is float32 with every operation rounded once: this file is compiled with -ffp-contract=off (build.py
// FILE_FLAGS), and hipcc's float division is IEEE; tests/_trace_ref.py restates it in numpy float32 bit for bit.
// Active lists are compacted ORDER-PRESERVING with a fixed-order scan in two launches -- (1) update + one count per workgroup,
// (2) every workgroup sums the counts in front of it, ranks its survivors by ballot and writes them -- no atomics, no spinning
// on another workgroup: bitwise reproducible and independent of how workgroups are scheduled.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

#include <math.h>

namespace {

constexpr int TB = 256;  // threads per workgroup of every kernel in this file (4 waves)
constexpr int REC = NCW_TRACE_REC_WORDS;
constexpr unsigned ST_MASK = 15u, BR_SHIFT = 4, BR_MASK = 0x3fffu, IT_SHIFT = 18;

NCW_DEV unsigned pack_word(unsigned state, unsigned bracket, unsigned iters) {
    return state | (bracket << BR_SHIFT) | (iters << IT_SHIFT);
}

// number of set flags in the workgroup (valid on every thread); lds: TB / 64 ints
NCW_DEV int block_count(bool flag, int* lds) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < TB / 64; ++w) s += lds[w];
    return s;
}

__global__ __launch_bounds__(TB) void trace_init_kernel(const float* __restrict__ near, const float* __restrict__ far, int n,
                                                        float* __restrict__ rec, int* __restrict__ block_counts) {
    __shared__ int lds[TB / 64];
    const int i = blockIdx.x * TB + threadIdx.x;
    bool alive = false;
    if (i < n) {
        const float t0 = near[i];
        alive = far[i] > t0;
        float* r = rec + (size_t)REC * i;
        r[0] = t0;
        r[1] = t0;
        r[2] = 0.f;
        r[3] = t0;
        r[4] = 0.f;
        reinterpret_cast<unsigned*>(r)[5] = pack_word(alive ? 0u : (unsigned)NCW_TRACE_MISS, 0u, 0u);
    }
    const int c = block_count(alive, lds);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = c;
}

__global__ __launch_bounds__(TB) void trace_update_kernel(const float* __restrict__ sdf, const int* __restrict__ active,
                                                          const int* __restrict__ count, int m_bound,
                                                          const float* __restrict__ far, float eps, float step, int max_iter,
                                                          float* __restrict__ rec,
                                                          int* __restrict__ block_counts) {
    __shared__ int lds[TB / 64];
    const int m = min(count[0], m_bound);  // the grid and the sdf buffer cover m_bound entries
    const int i = blockIdx.x * TB + threadIdx.x;
    bool alive = false;
    if (i < m) {
        const int ray = active[i];
        float* r = rec + (size_t)REC * ray;
        float t = r[0], t_lo = r[1], s_lo = r[2], t_hi = r[3], s_hi = r[4];
        const unsigned w0 = reinterpret_cast<unsigned*>(r)[5];
        unsigned state = w0 & ST_MASK, br = (w0 >> BR_SHIFT) & BR_MASK, it = w0 >> IT_SHIFT;
        const float s = sdf[i];
        it += 1;
        if (!(fabsf(s) <= 3.402823466e38f)) {  // NaN, +-inf
            state = NCW_TRACE_STALLED;
        } else if (fabsf(s) <= eps) {
            state = NCW_TRACE_HIT;
        } else if (s > 0.f) {
            t_lo = t;
            s_lo = s;
        } else if (it == 1) {
            state = NCW_TRACE_INSIDE;
        } else {
            t_hi = t;
            s_hi = s;
            br = br < 1 ? 1 : br;
        }
        if (state == 0) {
            if (br == 0) {
                const float tn = t + step * s;
                if (tn > far[ray])
                    state = NCW_TRACE_MISS;
                else
                    t = tn;
            } else {
                const float w = t_hi - t_lo;
                t = (br & 1) ? t_lo + (s_lo * w) / (s_lo - s_hi) : t_lo + 0.5f * w;
                br += 1;
            }
            if (state == 0 && it == (unsigned)max_iter) state = NCW_TRACE_STALLED;
        }
        r[0] = t;
        r[1] = t_lo;
        r[2] = s_lo;
        r[3] = t_hi;
        r[4] = s_hi;
        reinterpret_cast<unsigned*>(r)[5] = pack_word(state, br, it);
        alive = state == 0;
    }
    const int c = block_count(alive, lds);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = c;
}

// the rays of the list (active_in == NULL: the identity list 0 .. m - 1) that are still ACTIVE, in list order, and their points
__global__ __launch_bounds__(TB) void trace_compact_kernel(const int* __restrict__ active_in, const int* __restrict__ count_in,
                                                           int m_host, const float* __restrict__ rec,
                                                           const int* __restrict__ block_counts, const float* __restrict__ rays_o,
                                                           const float* __restrict__ rays_d, int* __restrict__ active_out,
                                                           int* __restrict__ count_out, float* __restrict__ points) {
    __shared__ int lds_pre[TB / 64];
    __shared__ int lds_cnt[TB / 64];
    const int m = count_in != nullptr ? min(count_in[0], m_host) : m_host;
    // counts of the workgroups in front of this one, summed in a fixed order
    int pre = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += TB) pre += block_counts[b];
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) pre += __shfl_xor(pre, k, 64);
    const int i = blockIdx.x * TB + threadIdx.x;
    int ray = -1;
    bool alive = false;
    if (i < m) {
        ray = active_in != nullptr ? active_in[i] : i;
        alive = (reinterpret_cast<const unsigned*>(rec)[(size_t)REC * ray + 5] & ST_MASK) == 0;
    }
    const unsigned long long bal = __ballot(alive);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        lds_pre[wave] = pre;
        lds_cnt[wave] = __popcll(bal);
    }
    __syncthreads();
    int base = 0, in_front = 0, total = 0;
#pragma unroll
    for (int w = 0; w < TB / 64; ++w) {
        base += lds_pre[w];
        in_front += w < wave ? lds_cnt[w] : 0;
        total += lds_cnt[w];
    }
    if (alive) {
        const int dst = base + in_front + __popcll(bal & ((1ull << lane) - 1ull));
        active_out[dst] = ray;
        const float t = rec[(size_t)REC * ray];
#pragma unroll
        for (int c = 0; c < 3; ++c) points[3 * (size_t)dst + c] = rays_o[3 * (size_t)ray + c] + t * rays_d[3 * (size_t)ray + c];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) count_out[0] = base + total;
}

__global__ __launch_bounds__(TB) void trace_finish_kernel(const float* __restrict__ rec, const float* __restrict__ rays_o,
                                                          const float* __restrict__ rays_d, int n, float* __restrict__ t_out,
                                                          uint8_t* __restrict__ state, int* __restrict__ iters,
                                                          float* __restrict__ points) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const float t = rec[(size_t)REC * i];
    const unsigned w0 = reinterpret_cast<const unsigned*>(rec)[(size_t)REC * i + 5];
    if (t_out != nullptr) t_out[i] = t;
    if (state != nullptr) state[i] = (uint8_t)(w0 & ST_MASK);
    if (iters != nullptr) iters[i] = (int)(w0 >> IT_SHIFT);
    if (points != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) points[3 * (size_t)i + c] = rays_o[3 * (size_t)i + c] + t * rays_d[3 * (size_t)i + c];
    }
}

struct Rgb3 {
    float v[3];
};

__global__ __launch_bounds__(TB) void trace_store_fill_kernel(const float* __restrict__ t, const uint8_t* __restrict__ state,
                                                              const int* __restrict__ iters, Rgb3 bg, int64_t p0, int n, int64_t hw,
                                                              float* __restrict__ color_img, float* __restrict__ depth_img,
                                                              float* __restrict__ normal_img, uint8_t* __restrict__ state_img,
                                                              int* __restrict__ iters_img) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int64_t p = p0 + i;
    const uint8_t st = state[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (color_img != nullptr) color_img[c * hw + p] = bg.v[c];
        if (normal_img != nullptr) normal_img[c * hw + p] = 0.f;
    }
    if (depth_img != nullptr) depth_img[p] = st == NCW_TRACE_HIT ? t[i] : 0.f;
    if (state_img != nullptr) state_img[p] = st;
    if (iters_img != nullptr) iters_img[p] = iters[i];
}

__global__ __launch_bounds__(TB) void trace_store_hits_kernel(const int64_t* __restrict__ hit_idx, const float* __restrict__ rgb,
                                                              const float* __restrict__ grad, int n_hit, int64_t p0, int n,
                                                              int64_t hw, float* __restrict__ color_img,
                                                              float* __restrict__ normal_img) {
    const int j = blockIdx.x * TB + threadIdx.x;
    if (j >= n_hit) return;
    const int64_t k = hit_idx[j];
    if (k < 0 || k >= n) return;  // not a pixel of this chunk: never written
    const int64_t p = p0 + k;
    if (color_img != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) color_img[c * hw + p] = rgb[3 * (size_t)j + c];
    }
    if (normal_img != nullptr) {
        const float x = grad[3 * (size_t)j], y = grad[3 * (size_t)j + 1], z = grad[3 * (size_t)j + 2];
        const float nrm = sqrtf(x * x + y * y + z * z);  // as ncw_view_store: 0 / 0 stays NaN
        normal_img[p] = x / nrm / 2.f + 0.5f;
        normal_img[hw + p] = y / nrm / 2.f + 0.5f;
        normal_img[2 * hw + p] = z / nrm / 2.f + 0.5f;
    }
}

inline bool bad_ptr(const void* p, uintptr_t mask = 3) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
inline bool bad_opt(const void* p, uintptr_t mask = 3) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
inline bool count_ok(int64_t n) { return n >= 0 && n <= 0x7fffffffLL; }
inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TB - 1) / TB); }

}  // namespace

extern "C" int64_t ncw_trace_scratch_bytes(int64_t R) {
    if (!count_ok(R)) return 0;
    const int64_t nb = (R + TB - 1) / TB;
    return 4 * (nb < 1 ? 1 : nb);
}

extern "C" int ncw_trace_begin(const float* rays_o, const float* rays_d, const float* near, const float* far, int64_t R, float* rec,
                               int32_t* active, int32_t* count, float* points, void* scratch, void* stream) {
    if (!count_ok(R)) return NCW_E_BADARG;
    if (R == 0) return 0;
    if (bad_ptr(rays_o) || bad_ptr(rays_d) || bad_ptr(near) || bad_ptr(far) || bad_ptr(rec) || bad_ptr(active) || bad_ptr(count) ||
        bad_ptr(points) || bad_ptr(scratch))
        return NCW_E_BADARG;
    const unsigned nb = blocks_of(R);
    int* bc = static_cast<int*>(scratch);
    hipLaunchKernelGGL(trace_init_kernel, dim3(nb), dim3(TB), 0, (hipStream_t)stream, near, far, (int)R, rec, bc);
    hipLaunchKernelGGL(trace_compact_kernel, dim3(nb), dim3(TB), 0, (hipStream_t)stream, (const int*)nullptr, (const int*)nullptr,
                       (int)R, (const float*)rec, (const int*)bc, rays_o, rays_d, active, count, points);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_trace_step(const float* sdf, const int32_t* active_in, const int32_t* count_in, int64_t m_bound,
                              const float* rays_o, const float* rays_d, const float* far, int64_t R, float eps, float step,
                              int max_iter, float* rec, int32_t* active_out, int32_t* count_out, float* points, void* scratch,
                              void* stream) {
    if (!count_ok(R) || !count_ok(m_bound) || m_bound > R) return NCW_E_BADARG;
    if (!(eps > 0.f) || !(step > 0.f && step <= 1.f) || max_iter < 1 || max_iter > NCW_TRACE_MAX_ITER) return NCW_E_BADARG;
    if (m_bound == 0) return 0;
    if (bad_ptr(sdf) || bad_ptr(active_in) || bad_ptr(count_in) || bad_ptr(rays_o) || bad_ptr(rays_d) || bad_ptr(far) ||
        bad_ptr(rec) || bad_ptr(active_out) || bad_ptr(count_out) || bad_ptr(points) || bad_ptr(scratch))
        return NCW_E_BADARG;
    if (active_out == active_in || count_out == count_in) return NCW_E_BADARG;
    const unsigned nb = blocks_of(m_bound);
    int* bc = static_cast<int*>(scratch);
    hipLaunchKernelGGL(trace_update_kernel, dim3(nb), dim3(TB), 0, (hipStream_t)stream, sdf, active_in, count_in, (int)m_bound, far,
                       eps, step, max_iter, rec, bc);
    hipLaunchKernelGGL(trace_compact_kernel, dim3(nb), dim3(TB), 0, (hipStream_t)stream, active_in, count_in, (int)m_bound,
                       (const float*)rec, (const int*)bc, rays_o, rays_d, active_out, count_out, points);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_trace_finish(const float* rec, const float* rays_o, const float* rays_d, int64_t R, float* t, uint8_t* state,
                                int32_t* iters, float* points, void* stream) {
    if (!count_ok(R)) return NCW_E_BADARG;
    if (R == 0) return 0;
    if (bad_ptr(rec) || bad_opt(t) || bad_opt(iters) || bad_opt(points)) return NCW_E_BADARG;
    if (points != nullptr && (bad_ptr(rays_o) || bad_ptr(rays_d))) return NCW_E_BADARG;
    hipLaunchKernelGGL(trace_finish_kernel, dim3(blocks_of(R)), dim3(TB), 0, (hipStream_t)stream, rec, rays_o, rays_d, (int)R, t,
                       state, iters, points);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_trace_store(const float* t, const uint8_t* state, const int32_t* iters, const int64_t* hit_idx, const float* rgb,
                               const float* grad, int64_t n_hit, const float* background_host, int64_t p0, int64_t n, int64_t n_pix,
                               float* color_img, float* depth_img, float* normal_img, uint8_t* state_img, int32_t* iters_img,
                               void* stream) {
    if (!count_ok(n) || p0 < 0 || n_pix < 0 || p0 + n > n_pix || n_hit < 0 || n_hit > n) return NCW_E_BADARG;
    if (n == 0) return 0;
    if (bad_ptr(t) || state == nullptr || bad_ptr(iters) || bad_opt(color_img) || bad_opt(depth_img) || bad_opt(normal_img) ||
        bad_opt(iters_img))
        return NCW_E_BADARG;
    if (n_hit > 0 && (bad_ptr(hit_idx, 7) || (color_img != nullptr && bad_ptr(rgb)) || (normal_img != nullptr && bad_ptr(grad))))
        return NCW_E_BADARG;
    Rgb3 bg = {{0.f, 0.f, 0.f}};
    if (background_host != nullptr)
        for (int c = 0; c < 3; ++c) bg.v[c] = background_host[c];
    hipLaunchKernelGGL(trace_store_fill_kernel, dim3(blocks_of(n)), dim3(TB), 0, (hipStream_t)stream, t, state, iters, bg, p0, (int)n,
                       n_pix, color_img, depth_img, normal_img, state_img, iters_img);
    if (n_hit > 0)
        hipLaunchKernelGGL(trace_store_hits_kernel, dim3(blocks_of(n_hit)), dim3(TB), 0, (hipStream_t)stream, hit_idx, rgb, grad,
                           (int)n_hit, p0, (int)n, n_pix, color_img, normal_img);
    NCW_CHECK_LAUNCH();
    return 0;
}
