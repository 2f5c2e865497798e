// Fusion of traced surface samples into ONE oriented, coloured surface cloud (surfcloud.SurfaceCloud; not in the reference).
// The contract -- QUANTISE, ACCUMULATE, RESOLVE -- is stated once in include/neuconw_hip.h and restated in numpy by
// tests/_fuse_ref.py.
//
//   ncw_fuse_insert  : one lane per sample: quantise it (float64, every operation rounded on its own) to a cell key and an
//                      all-integer payload, find or claim the key's slot in an open-addressed table and add the payload;
//   ncw_fuse_move    : one lane per row of a smaller table: the same find-or-claim and adds into a larger one (growth);
//   (caller)         : the occupied rows, compacted and sorted by key (torch.nonzero / torch.sort) -- plumbing;
//   ncw_fuse_resolve : one lane per occupied row, in the caller's order: mean position inside the cell, unit normal, colour.
//
// TABLE RULES (insert and move).  The probe loop is bounded by the capacity; a sample that finds no slot adds 1 to the
// overflow counter and is dropped.  No lane waits for another: no spin, no lock, no flag hand-off -- a lane that loses the
// compare-and-swap on an EMPTY word looks at what the winner wrote and walks on.  While workgroups insert, every word of the
// destination table is touched ONLY by agent-scope atomics (compare-and-swap, integer add, integer max) or relaxed agent-scope
// atomic loads: the L2s of the XCDs are not coherent for plain accesses.  Only integers are added, so the table's content is a
// function of the multiset of (sample, serial) pairs; no float atomics.  The payload words are zero before a key can be
// claimed (the caller zeroes the table), so an add may land before or after the claim becomes visible elsewhere: no ordering
// between the claim and the adds is needed.  The occupied / valid / overflow counters are summed per wave (ballot + popcount)
// before their one atomic.
#include "../../include/neuconw_hip.h"
#include "ncw_common.h"

// every product, sum and quotient is rounded on its own (no fused multiply-add): the numpy restatement is the same arithmetic
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxCount = 0x7fffffffll;
constexpr int64_t kMaxDim = 1ll << NCW_FUSE_MAX_DIM_LOG2;
constexpr int64_t kMaxCapacity = 1ll << NCW_FUSE_MAX_CAPACITY_LOG2;
constexpr int64_t kEmpty = NCW_FUSE_EMPTY;

struct FuseGrid {
    double lo[3];
    double h;
    int64_t dims[3];
    double scale;
    double off[3];
    double cos_min;
    int facing;
};

struct FuseTable {
    int64_t* keys;      // [capacity]
    int64_t* acc;       // [capacity, NCW_FUSE_ACC]
    int32_t* stamp;     // [capacity]
    int32_t* views;     // [capacity]
    int64_t* counters;  // [NCW_FUSE_COUNTERS]
    int64_t capacity;
};

#define FUSE_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// splitmix64's finaliser: the 64-bit mix the probe sequence starts from
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// The slot of `key` (>= 0) in the table, claiming an EMPTY word if the key is not there yet; -1 if `capacity` probes found
// neither.  claimed = this lane's compare-and-swap put the key there.
__device__ __forceinline__ int64_t find_or_claim(int64_t* keys, int64_t capacity, int64_t key, bool& claimed) {
    const uint64_t mask = (uint64_t)capacity - 1;
    uint64_t slot = mix64((uint64_t)key) & mask;
    claimed = false;
    for (int64_t probe = 0; probe < capacity; ++probe) {
        int64_t seen = __hip_atomic_load(&keys[slot], FUSE_RLX);
        if (seen == kEmpty) {
            int64_t expected = kEmpty;
            if (__hip_atomic_compare_exchange_strong(&keys[slot], &expected, key, __ATOMIC_RELAXED, FUSE_RLX)) {
                claimed = true;
                return (int64_t)slot;
            }
            seen = expected;  // the word another lane won the claim with
        }
        if (seen == key) return (int64_t)slot;
        slot = (slot + 1) & mask;
    }
    return -1;
}

// one atomic per wave for a counter every lane may add 0 / 1 to; every lane of the wave that is still running calls it
__device__ __forceinline__ void wave_count(int64_t* counter, bool one) {
    const unsigned long long m = __ballot(one);
    if (m != 0 && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1)
        __hip_atomic_fetch_add(counter, (int64_t)__popcll(m), FUSE_RLX);
}

__device__ __forceinline__ bool finite3(const float* v) {
    return __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]);
}

__global__ __launch_bounds__(kBlock) void fuse_insert_kernel(const float* __restrict__ points, const float* __restrict__ grads,
                                                             const float* __restrict__ dirs, const float* __restrict__ colours,
                                                             int n, int serial, FuseGrid g, FuseTable t) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    int64_t key = -1;
    int64_t pay[NCW_FUSE_ACC];
    if (live) {
        const float p[3] = {points[i * 3 + 0], points[i * 3 + 1], points[i * 3 + 2]};
        const float gr[3] = {grads[i * 3 + 0], grads[i * 3 + 1], grads[i * 3 + 2]};
        const float d[3] = {dirs[i * 3 + 0], dirs[i * 3 + 1], dirs[i * 3 + 2]};
        bool ok = finite3(p) && finite3(gr) && finite3(d);
        double frac[3];
        int64_t cell[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = (double)p[a] * g.scale + g.off[a];
            const double ga = (x - g.lo[a]) / g.h;
            const double cf = floor(ga);
            ok = ok && cf >= 0.0 && cf < (double)g.dims[a];  // false for NaN
            frac[a] = ga - cf;
            cell[a] = ok ? (int64_t)cf : 0;
        }
        const double nx = (double)gr[0], ny = (double)gr[1], nz = (double)gr[2];
        const double nn = (nx * nx + ny * ny) + nz * nz;
        ok = ok && __builtin_isfinite(nn) && nn > 0.0;
        const double len = sqrt(nn);
        if (g.facing) {
            const double facing = -((nx * (double)d[0] + ny * (double)d[1]) + nz * (double)d[2]);
            ok = ok && facing >= g.cos_min * len;
        }
        if (ok) {
            key = (cell[2] * g.dims[1] + cell[1]) * g.dims[0] + cell[0];
            pay[0] = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double q = floor(frac[a] * 65536.0);
                pay[1 + a] = q < 65535.0 ? (int64_t)q : 65535;
                pay[4 + a] = (int64_t)rint((double)gr[a] / len * 32767.0);  // ties to even
                double c = (double)colours[i * 3 + a];
                c = c > 0.0 ? c : 0.0;  // NaN -> 0
                c = c < 1.0 ? c : 1.0;
                pay[7 + a] = (int64_t)rint(c * 255.0);
            }
        }
    }
    bool claimed = false;
    int64_t slot = -1;
    if (key >= 0) {
        slot = find_or_claim(t.keys, t.capacity, key, claimed);
        if (slot >= 0) {
            int64_t* row = t.acc + slot * NCW_FUSE_ACC;
#pragma unroll
            for (int j = 0; j < NCW_FUSE_ACC; ++j) __hip_atomic_fetch_add(&row[j], pay[j], FUSE_RLX);
            // distinct serials: the caller's serials never decrease, so exactly one sample of a serial raises the stamp
            const int old = __hip_atomic_fetch_max(&t.stamp[slot], serial + 1, FUSE_RLX);
            if (old < serial + 1) __hip_atomic_fetch_add(&t.views[slot], 1, FUSE_RLX);
        }
    }
    wave_count(&t.counters[NCW_FUSE_CNT_OCCUPIED], claimed);
    wave_count(&t.counters[NCW_FUSE_CNT_OVERFLOW], key >= 0 && slot < 0);
    wave_count(&t.counters[NCW_FUSE_CNT_VALID], key >= 0);
}

__global__ __launch_bounds__(kBlock) void fuse_move_kernel(FuseTable s, FuseTable t) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    // the source table is not written by this launch: plain loads
    const int64_t key = r < s.capacity ? s.keys[r] : -1;
    bool claimed = false;
    int64_t slot = -1;
    if (key >= 0) {
        slot = find_or_claim(t.keys, t.capacity, key, claimed);
        if (slot >= 0) {
            const int64_t* from = s.acc + r * NCW_FUSE_ACC;
            int64_t* row = t.acc + slot * NCW_FUSE_ACC;
#pragma unroll
            for (int j = 0; j < NCW_FUSE_ACC; ++j) __hip_atomic_fetch_add(&row[j], from[j], FUSE_RLX);
            __hip_atomic_fetch_max(&t.stamp[slot], s.stamp[r], FUSE_RLX);
            __hip_atomic_fetch_add(&t.views[slot], s.views[r], FUSE_RLX);
        }
    }
    wave_count(&t.counters[NCW_FUSE_CNT_OCCUPIED], claimed);
    wave_count(&t.counters[NCW_FUSE_CNT_OVERFLOW], key >= 0 && slot < 0);
}

__global__ __launch_bounds__(kBlock) void fuse_resolve_kernel(FuseTable t, const int64_t* __restrict__ rows, int n_rows, FuseGrid g,
                                                              double* __restrict__ pos, float* __restrict__ normal,
                                                              uint8_t* __restrict__ colour, int64_t* __restrict__ count,
                                                              int32_t* __restrict__ views, uint8_t* __restrict__ degenerate,
                                                              int64_t* __restrict__ keys) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_rows) return;
    const int64_t r = rows[k];
    int64_t key = -1;
    if (r >= 0 && r < t.capacity) key = t.keys[r];
    const int64_t cells = g.dims[0] * g.dims[1] * g.dims[2];
    if (key < 0 || key >= cells) {  // not a row of this table: nothing is used as an index
        for (int a = 0; a < 3; ++a) {
            pos[k * 3 + a] = 0.0;
            normal[k * 3 + a] = 0.f;
            colour[k * 3 + a] = 0;
        }
        count[k] = 0;
        views[k] = 0;
        degenerate[k] = 1;
        keys[k] = -1;
        return;
    }
    const int64_t* row = t.acc + r * NCW_FUSE_ACC;
    const int64_t cnt = row[0];
    const int64_t den = cnt > 0 ? cnt : 1;
    const int64_t cell[3] = {key % g.dims[0], (key / g.dims[0]) % g.dims[1], key / g.dims[0] / g.dims[1]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double m = ((double)row[1 + a] / (double)den + 0.5) / 65536.0;
        pos[k * 3 + a] = g.lo[a] + ((double)cell[a] + m) * g.h;
        colour[k * 3 + a] = (uint8_t)((2 * row[7 + a] + den) / (2 * den));
    }
    const double nx = (double)row[4], ny = (double)row[5], nz = (double)row[6];
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    const bool deg = !(len > 0.0);
    normal[k * 3 + 0] = deg ? 0.f : (float)(nx / len);
    normal[k * 3 + 1] = deg ? 0.f : (float)(ny / len);
    normal[k * 3 + 2] = deg ? 0.f : (float)(nz / len);
    count[k] = cnt;
    views[k] = t.views[r];
    degenerate[k] = deg ? 1 : 0;
    keys[k] = key;
}

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

inline bool aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

inline bool grid_ok(const NcwFuseGrid* in, FuseGrid* g) {
    if (!in || !(in->h > 0.0) || !__builtin_isfinite(in->h) || !__builtin_isfinite(in->scale)) return false;
    for (int a = 0; a < 3; ++a) {
        if (!__builtin_isfinite(in->lo[a]) || !__builtin_isfinite(in->off[a]) || in->dims[a] < 1 || in->dims[a] > kMaxDim)
            return false;
        g->lo[a] = in->lo[a];
        g->off[a] = in->off[a];
        g->dims[a] = in->dims[a];
    }
    if (in->facing != 0 && !__builtin_isfinite(in->cos_min)) return false;
    g->h = in->h;
    g->scale = in->scale;
    g->cos_min = in->cos_min;
    g->facing = in->facing != 0;
    return true;
}

inline bool table_ok(const NcwFuseTable* in, FuseTable* t) {
    if (!in || in->capacity < 1 || in->capacity > kMaxCapacity || (in->capacity & (in->capacity - 1)) != 0) return false;
    if (!aligned(in->keys, 8) || !aligned(in->acc, 8) || !aligned(in->stamp, 4) || !aligned(in->views, 4) ||
        !aligned(in->counters, 8))
        return false;
    t->keys = in->keys;
    t->acc = in->acc;
    t->stamp = in->stamp;
    t->views = in->views;
    t->counters = in->counters;
    t->capacity = in->capacity;
    return true;
}

}  // namespace

extern "C" int ncw_fuse_insert(const float* points, const float* grads, const float* dirs, const float* colours, int64_t n,
                               int32_t serial, const NcwFuseGrid* grid, const NcwFuseTable* table, void* stream) {
    FuseGrid g;
    FuseTable t;
    if (n < 0 || n > kMaxCount || serial < 0 || serial > NCW_FUSE_MAX_SERIAL || !grid_ok(grid, &g) || !table_ok(table, &t))
        return NCW_E_BADARG;
    if (n == 0) return 0;
    if (!aligned(points, 4) || !aligned(grads, 4) || !aligned(dirs, 4) || !aligned(colours, 4)) return NCW_E_BADARG;
    hipLaunchKernelGGL(fuse_insert_kernel, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, points, grads, dirs, colours, (int)n,
                       (int)serial, g, t);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_fuse_move(const NcwFuseTable* src, const NcwFuseTable* dst, void* stream) {
    FuseTable s, t;
    if (!table_ok(src, &s) || !table_ok(dst, &t) || t.capacity < s.capacity || s.keys == t.keys || s.acc == t.acc ||
        s.stamp == t.stamp || s.views == t.views)
        return NCW_E_BADARG;
    hipLaunchKernelGGL(fuse_move_kernel, grid_for(s.capacity), dim3(kBlock), 0, (hipStream_t)stream, s, t);
    NCW_CHECK_LAUNCH();
    return 0;
}

extern "C" int ncw_fuse_resolve(const NcwFuseTable* table, const int64_t* rows, int64_t n_rows, const NcwFuseGrid* grid,
                                double* pos, float* normal, uint8_t* colour, int64_t* count, int32_t* views, uint8_t* degenerate,
                                int64_t* keys, void* stream) {
    FuseGrid g;
    FuseTable t;
    if (n_rows < 0 || n_rows > kMaxCount || !grid_ok(grid, &g) || !table_ok(table, &t) || n_rows > t.capacity) return NCW_E_BADARG;
    if (n_rows == 0) return 0;
    if (!aligned(rows, 8) || !aligned(pos, 8) || !aligned(normal, 4) || !colour || !aligned(count, 8) || !aligned(views, 4) ||
        !degenerate || !aligned(keys, 8))
        return NCW_E_BADARG;
    hipLaunchKernelGGL(fuse_resolve_kernel, grid_for(n_rows), dim3(kBlock), 0, (hipStream_t)stream, t, rows, (int)n_rows, g, pos,
                       normal, colour, count, views, degenerate, keys);
    NCW_CHECK_LAUNCH();
    return 0;
}
