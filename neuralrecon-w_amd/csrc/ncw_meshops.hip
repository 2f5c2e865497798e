// Mesh operations on the GPU: connected components of a triangle mesh and the compaction of a face subset (meshops.py).  The
// reference has no such mode: its evaluation filter (utils/reproj_filter.py) writes a point cloud and nothing in it labels
// components.  Two users: the reprojection filter keeps the faces of the vertices it marks (reproj.reproj_filter keep_faces),
// and the extraction drops floaters before the colour pass (mesh.extract_mesh).  Both choose a subset of faces and compact.
//
// CONNECTIVITY is by SHARED VERTEX INDEX: two faces that only share coordinates are not connected, two pieces that touch in
// one welded vertex are one component.  A face PARTICIPATES iff keep[f] != 0 (keep == NULL: every face), its three corners
// lie in [0, V) and are distinct.
//
//   ncw_mesh_cc_hook    : one lane per face, lock-free union-find over parent[V] (= arange(V) on entry).  union(u, v): walk
//                         both to their roots; equal -> done; else old = atomicMin(&parent[hi], lo) with hi the larger root.
//                         old == hi: hi was a root and now hangs under lo, done.  Otherwise hi had been hooked meanwhile
//                         (its parent was old < hi, and is min(old, lo) now): whichever of old / lo lost the word still has
//                         to be joined to the other, so the lane goes on with (old, lo).
//                         INVARIANT parent[x] <= x at all times (the word only ever takes a minimum with a smaller index):
//                         no cycles, every walk ends, and every retry continues from max(old, lo) < hi, a strictly smaller
//                         index.  NO LANE EVER WAITS ON ANOTHER: there is no spin loop and no lock, every loop is bounded by
//                         a decreasing index whatever the other lanes do.  Reads of parent are device-scope relaxed loads
//                         (served by L2, never a stale L1 line); the walks shorten the path they follow by path halving,
//                         itself an atomicMin(&parent[x], grandparent) -- an ancestor, so the invariant and the partition
//                         hold.  A value that has once been x's parent stays in x's component: whoever lowers the word
//                         re-joins the old parent (the retry above), or the old parent keeps its own link to the new one
//                         (halving).
//   ncw_mesh_cc_flatten : parent[v] = root of v.  The root of a tree is its smallest index (invariant), and hook leaves one
//                         tree per component: the label of a component is THE SMALLEST VERTEX INDEX IN IT, a property of
//                         the mesh and not of the schedule.  A vertex of no participating face is its own label.
//   ncw_mesh_cc_sizes   : sizes[label] += participating faces of the component (label of corner 0), integer adds, aggregated
//                         per wave (one add per distinct label of the wave) and per workgroup (an LDS table) before they
//                         reach global memory: one add per face measured 40 ms on a 34 M-face mesh, 8x the hook.
//   ncw_mesh_face_select: the face rule (see the header).
//   ncw_mesh_compact_*  : mark the used vertices (plain stores of the same value), write the kept faces remapped.
//
// Integer atomics only (min, add): every result is a function of the mesh, bitwise reproducible and independent of launch
// order or split.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxCount = 0x7fffffffll;

__device__ __forceinline__ bool face_valid(int a, int b, int c, int n_verts) {
    const unsigned v = (unsigned)n_verts;  // negative indices wrap above 2^31 > V
    return (unsigned)a < v && (unsigned)b < v && (unsigned)c < v && a != b && b != c && a != c;
}

__device__ __forceinline__ int parent_of(const int32_t* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x.  Path halving: x's word takes the minimum with its grandparent, then the walk continues from the grandparent.
// Bounded by the invariant: every step moves to a strictly smaller index or stops.
__device__ __forceinline__ int find_halving(int32_t* parent, int x) {
    int p = parent_of(parent, x);
    while (p != x) {
        const int g = parent_of(parent, p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
        p = parent_of(parent, x);
    }
    return x;
}

__device__ __forceinline__ int find_readonly(const int32_t* parent, int x) {
    int p = parent_of(parent, x);
    while (p != x) {
        x = p;
        p = parent_of(parent, x);
    }
    return x;
}

__device__ __forceinline__ void unite(int32_t* parent, int u, int v) {
    for (;;) {
        u = find_halving(parent, u);
        v = find_halving(parent, v);
        if (u == v) return;
        const int hi = u > v ? u : v, lo = u > v ? v : u;
        const int old = atomicMin(parent + hi, lo);
        if (old == hi) return;
        u = old;  // < hi
        v = lo;   // < hi
    }
}

__global__ __launch_bounds__(kBlock) void cc_hook_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep,
                                                          int n_faces, int n_verts, int32_t* parent) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    if (keep && !keep[f]) return;
    const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (!face_valid(a, b, c, n_verts)) return;
    unite(parent, a, b);
    unite(parent, a, c);
}

__global__ __launch_bounds__(kBlock) void cc_flatten_kernel(int32_t* parent, int n_verts) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n_verts) return;
    // the other lanes only replace words by roots of the same (now fixed) trees: whatever this walk reads is an ancestor
    const int r = find_readonly(parent, (int)v);
    __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup of kSizesBlock faces.  Per wave: for every distinct label among its lanes (a wave-uniform loop over the ballot of
// the lanes still to be counted, at most 64 rounds) the first such lane adds the population count of the lanes that share it.
// Per workgroup: those adds go to a small LDS table (key = label, claimed by ONE compare-and-swap attempt per probed slot, four
// probes, never retried: a lane that finds no slot adds to global memory itself), and the table is flushed with one global
// atomicAdd per occupied slot.  Integer adds only: the sums do not depend on who claimed which slot.
constexpr int kSizesBlock = 1024;
constexpr int kSizesSlots = 128;

__global__ __launch_bounds__(kSizesBlock) void cc_sizes_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep,
                                                                int n_faces, int n_verts, const int32_t* __restrict__ labels,
                                                                int32_t* sizes) {
    __shared__ int s_key[kSizesSlots];
    __shared__ int s_cnt[kSizesSlots];
    for (int i = threadIdx.x; i < kSizesSlots; i += kSizesBlock) {
        s_key[i] = -1;
        s_cnt[i] = 0;
    }
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * kSizesBlock + threadIdx.x;
    int label = -1;  // every lane reaches the ballots and the barrier below: no early return
    if (f < n_faces && (!keep || keep[f])) {
        const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
        if (face_valid(a, b, c, n_verts)) {
            const int l = labels[a];
            if ((unsigned)l < (unsigned)n_verts) label = l;  // labels come from flatten; never index sizes outside [0, V)
        }
    }
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long todo = __ballot(label >= 0);  // the same value in every lane: the loop is wave-uniform
    while (todo != 0ull) {
        const int first = __ffsll((long long)todo) - 1;
        const int lead = __shfl(label, first);
        const unsigned long long same = __ballot(label == lead);
        if (lane == first) {
            const int n = (int)__popcll(same);
            const unsigned h = ((unsigned)lead * 2654435761u) >> 25;  // 7 bits
            bool placed = false;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (!placed) {
                    const int slot = (int)((h + (unsigned)p) & (unsigned)(kSizesSlots - 1));
                    const int old = atomicCAS(&s_key[slot], -1, lead);
                    if (old == -1 || old == lead) {
                        atomicAdd(&s_cnt[slot], n);
                        placed = true;
                    }
                }
            }
            if (!placed) atomicAdd(sizes + lead, n);
        }
        todo &= ~same;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSizesSlots; i += kSizesBlock) {
        if (s_key[i] >= 0) atomicAdd(sizes + s_key[i], s_cnt[i]);
    }
}

__global__ __launch_bounds__(kBlock) void face_select_kernel(const int32_t* __restrict__ faces, int n_faces, int n_verts,
                                                              const uint8_t* __restrict__ vflags, int min_corners,
                                                              const int32_t* __restrict__ labels,
                                                              const uint8_t* __restrict__ comp_ok, uint8_t* __restrict__ keep_out) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    bool k = face_valid(a, b, c, n_verts);
    if (k && vflags) k = (int)(vflags[a] != 0) + (int)(vflags[b] != 0) + (int)(vflags[c] != 0) >= min_corners;
    if (k && labels) {
        const int l = labels[a];
        k = (unsigned)l < (unsigned)n_verts && comp_ok[l] != 0;
    }
    keep_out[f] = k ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void compact_mark_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep,
                                                               int n_faces, int n_verts, uint8_t* used) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces || !keep[f]) return;
    const unsigned v = (unsigned)n_verts;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = faces[f * 3 + k];
        if ((unsigned)i < v) used[i] = 1;  // every writer stores the same value
    }
}

__global__ __launch_bounds__(kBlock) void compact_faces_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep,
                                                                const int32_t* __restrict__ face_offset,
                                                                const int32_t* __restrict__ vmap, int n_faces, int n_verts,
                                                                int n_out, int32_t* __restrict__ faces_out) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces || !keep[f]) return;
    const int o = face_offset[f];
    if ((unsigned)o >= (unsigned)n_out) return;  // an offset that is not the prefix sum of keep: write nothing
    const unsigned v = (unsigned)n_verts;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = faces[f * 3 + k];
        faces_out[(int64_t)o * 3 + k] = (unsigned)i < v ? vmap[i] : -1;
    }
}

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

}  // namespace

extern "C" int ncw_mesh_cc_hook(const int32_t* faces, const uint8_t* keep, int64_t n_faces, int64_t n_verts, int32_t* parent,
                                void* stream) {
    if (n_faces < 0 || n_faces > kMaxCount || n_verts < 0 || n_verts > kMaxCount) return NCW_E_BADARG;
    if (n_faces == 0 || n_verts == 0) return 0;
    if (!faces || !parent) return NCW_E_BADARG;
    hipLaunchKernelGGL(cc_hook_kernel, grid_for(n_faces), dim3(kBlock), 0, (hipStream_t)stream, faces, keep, (int)n_faces,
                       (int)n_verts, parent);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mesh_cc_flatten(int32_t* parent, int64_t n_verts, void* stream) {
    if (n_verts < 0 || n_verts > kMaxCount) return NCW_E_BADARG;
    if (n_verts == 0) return 0;
    if (!parent) return NCW_E_BADARG;
    hipLaunchKernelGGL(cc_flatten_kernel, grid_for(n_verts), dim3(kBlock), 0, (hipStream_t)stream, parent, (int)n_verts);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mesh_cc_sizes(const int32_t* faces, const uint8_t* keep, int64_t n_faces, int64_t n_verts,
                                 const int32_t* labels, int32_t* sizes, void* stream) {
    if (n_faces < 0 || n_faces > kMaxCount || n_verts < 0 || n_verts > kMaxCount) return NCW_E_BADARG;
    if (n_faces == 0 || n_verts == 0) return 0;
    if (!faces || !labels || !sizes) return NCW_E_BADARG;
    hipLaunchKernelGGL(cc_sizes_kernel, dim3((unsigned)((n_faces + kSizesBlock - 1) / kSizesBlock)), dim3(kSizesBlock), 0,
                       (hipStream_t)stream, faces, keep, (int)n_faces, (int)n_verts, labels, sizes);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mesh_face_select(const int32_t* faces, int64_t n_faces, int64_t n_verts, const uint8_t* vflags, int min_corners,
                                    const int32_t* labels, const uint8_t* comp_ok, uint8_t* keep_out, void* stream) {
    if (n_faces < 0 || n_faces > kMaxCount || n_verts < 0 || n_verts > kMaxCount) return NCW_E_BADARG;
    if (min_corners < 1 || min_corners > 3 || (labels != nullptr) != (comp_ok != nullptr)) return NCW_E_BADARG;
    if (n_faces == 0) return 0;
    if (!faces || !keep_out) return NCW_E_BADARG;
    hipLaunchKernelGGL(face_select_kernel, grid_for(n_faces), dim3(kBlock), 0, (hipStream_t)stream, faces, (int)n_faces,
                       (int)n_verts, vflags, min_corners, labels, comp_ok, keep_out);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mesh_compact_mark(const int32_t* faces, const uint8_t* keep, int64_t n_faces, int64_t n_verts, uint8_t* used,
                                     void* stream) {
    if (n_faces < 0 || n_faces > kMaxCount || n_verts < 0 || n_verts > kMaxCount) return NCW_E_BADARG;
    if (n_faces == 0 || n_verts == 0) return 0;
    if (!faces || !keep || !used) return NCW_E_BADARG;
    hipLaunchKernelGGL(compact_mark_kernel, grid_for(n_faces), dim3(kBlock), 0, (hipStream_t)stream, faces, keep, (int)n_faces,
                       (int)n_verts, used);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_mesh_compact_faces(const int32_t* faces, const uint8_t* keep, const int32_t* face_offset, const int32_t* vmap,
                                      int64_t n_faces, int64_t n_verts, int64_t n_out, int32_t* faces_out, void* stream) {
    if (n_faces < 0 || n_faces > kMaxCount || n_verts < 0 || n_verts > kMaxCount || n_out < 0 || n_out > n_faces)
        return NCW_E_BADARG;
    if (n_faces == 0 || n_out == 0) return 0;
    if (!faces || !keep || !face_offset || !vmap || !faces_out) return NCW_E_BADARG;
    hipLaunchKernelGGL(compact_faces_kernel, grid_for(n_faces), dim3(kBlock), 0, (hipStream_t)stream, faces, keep, face_offset,
                       vmap, (int)n_faces, (int)n_verts, (int)n_out, faces_out);
    NCW_CHECK_LAUNCH();
    return 0;
}
