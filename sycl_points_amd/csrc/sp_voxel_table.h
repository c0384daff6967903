// What the two hashed voxel maps share (voxel_hash_map.hip, occupancy_grid_map.hip). The reference keeps a copy of each piece in both
// classes (mapping/voxel_hash_map.hpp, mapping/occupancy_grid_map.hpp); here there is one.
//   * the arithmetic: the 63-bit voxel key, the double-hashed slot sequence, the capacity ladder, the log-Euclidean covariance
//     encoding and the no-return float atomic;
//   * the table: six parallel arrays in HBM (key u64 | core, the map's own {sums, counts, ...} | log-covariance sums 24 B | colour
//     sums 16 B | intensity sum | stamp of the last update), open addressing; its allocation, the read-only probe, the attribute
//     atomics, the averaged output row and the overlap kernel;
//   * the host state around it (VoxelMapState): settings and has_* flags, the 4-word device counter, growing into a larger table,
//     the flags -> exclusive scan compaction scratch (and the list of flagged slots), create / clear / destroy.
// What stays in the two .hip files differs on purpose: how a slot is claimed, how a table is rehashed, which slots an export keeps.
// The kernels here are compiled into both translation units (unnamed namespace, voxel_table_* names).
#pragma once
#include "radix_sort.h"
#include "sp_common.h"
#include "sp_math.h"
#include "sp_spatial.h"

void sp_set_error(const char* msg);

namespace sp {

constexpr uint64_t kInvalidKey = ~0ull;  // VoxelConstants::invalid_coord
constexpr size_t kCapacityCandidates[11] = {30029,  60013,   120011,  240007,   480013,  960017,
                                            1920001, 3840007, 7680017, 15360013, 30720007};  // voxel_hash_map.hpp:486-487

// get_next_capacity_value: the first rung above `capacity`, or `capacity` on the last one
inline size_t next_capacity(size_t capacity) {
    for (const size_t c : kCapacityCandidates)
        if (c > capacity) return c;
    return capacity;
}

struct CovSum { float xx, xy, xz, yy, yz, zz; };

// filter::kernel::compute_voxel_bit (voxel_constants.hpp:36-62) — the same arithmetic as voxel.hip's K9
__device__ __forceinline__ uint64_t voxel_key3(float x, float y, float z, float inv) {
    constexpr int64_t mask = (1 << 21) - 1;
    constexpr int64_t offset = 1 << 20;
    if (!isfinite(x) || !isfinite(y) || !isfinite(z)) return kInvalidKey;
    const int64_t c0 = (int64_t)floorf(x * inv) + offset;
    const int64_t c1 = (int64_t)floorf(y * inv) + offset;
    const int64_t c2 = (int64_t)floorf(z * inv) + offset;
    if (c0 < 0 || mask < c0 || c1 < 0 || mask < c1 || c2 < 0 || mask < c2) return kInvalidKey;
    return ((uint64_t)(c0 & mask)) | ((uint64_t)(c1 & mask) << 21) | ((uint64_t)(c2 & mask) << 42);
}

// compute_slot_id (voxel_hash_map.hpp:587-592)
__device__ __forceinline__ unsigned long long slot_id(uint64_t h, unsigned long long probe, unsigned long long cap) {
    const unsigned long long h2 = (cap - 2) - (h % (cap - 2));
    return (h + probe * h2) % cap;
}

// V diag(f(ev)) V^T, symmetrised (eigen_utils.hpp:646-677): LOG = log(max(ev, 1e-6)), else exp(ev)
template <bool LOG>
__device__ __forceinline__ Mat3 spd_map(const Mat3& A) {
    float ev[3];
    Mat3 V;
    symmetric_eigen3(A, ev, V);
    float f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = LOG ? logf(sycl_max(ev[i], 1e-6f)) : expf(ev[i]);
    Mat3 VD;  // multiply<3,3,3>(V, diag): per element an fma chain over k with two zero terms
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) s = fmaf(V.m[i][k], (k == j) ? f[k] : 0.0f, s);
            VD.m[i][j] = s;
        }
    const Mat3 P = matmul_bt(VD, V);  // (V D) V^T
    Mat3 S;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S.m[i][j] = (i == j) ? P.m[i][j] : (P.m[i][j] + P.m[j][i]) * 0.5f;
    return S;
}

// rotate_covariance_upper_triangle (voxel_hash_map.hpp:420-458), the reference's fma order
__device__ __forceinline__ CovSum rotate_cov(const float4* __restrict__ c, const Rigid& T) {
    const float4 c0 = c[0], c1 = c[1], c2 = c[2];  // columns of the 4x4
    const float cxx = c0.x, cxy = c1.x, cxz = c2.x, cyy = c1.y, cyz = c2.y, czz = c2.z;
    const float(&R)[3][3] = T.R;
    auto f3 = [](float a, float b, float c_, float d, float e, float f) { return fmaf(a, b, fmaf(c_, d, e * f)); };
    const float a00 = f3(R[0][2], cxz, R[0][1], cxy, R[0][0], cxx), a01 = f3(R[0][2], cyz, R[0][1], cyy, R[0][0], cxy),
                a02 = f3(R[0][2], czz, R[0][1], cyz, R[0][0], cxz);
    const float a10 = f3(R[1][2], cxz, R[1][1], cxy, R[1][0], cxx), a11 = f3(R[1][2], cyz, R[1][1], cyy, R[1][0], cxy),
                a12 = f3(R[1][2], czz, R[1][1], cyz, R[1][0], cxz);
    const float a20 = f3(R[2][2], cxz, R[2][1], cxy, R[2][0], cxx), a21 = f3(R[2][2], cyz, R[2][1], cyy, R[2][0], cxy),
                a22 = f3(R[2][2], czz, R[2][1], cyz, R[2][0], cxz);
    CovSum o;
    o.xx = f3(a02, R[0][2], a01, R[0][1], a00, R[0][0]);
    o.xy = f3(a02, R[1][2], a01, R[1][1], a00, R[1][0]);
    o.xz = f3(a02, R[2][2], a01, R[2][1], a00, R[2][0]);
    o.yy = f3(a12, R[1][2], a11, R[1][1], a10, R[1][0]);
    o.yz = f3(a12, R[2][2], a11, R[2][1], a10, R[2][0]);
    o.zz = f3(a22, R[2][2], a21, R[2][1], a20, R[2][0]);
    return o;
}

// rotate into the map frame, then the log-Euclidean encoding (encode_covariance_for_aggregation, voxel_hash_map.hpp:460-480)
__device__ __forceinline__ CovSum encode_cov(const float4* __restrict__ c, const Rigid& T) {
    const CovSum r = rotate_cov(c, T);
    Mat3 m;
    m.m[0][0] = r.xx; m.m[0][1] = m.m[1][0] = r.xy; m.m[0][2] = m.m[2][0] = r.xz;
    m.m[1][1] = r.yy; m.m[1][2] = m.m[2][1] = r.yz; m.m[2][2] = r.zz;
    const Mat3 l = spd_map<true>(m);
    return CovSum{l.m[0][0], l.m[0][1], l.m[0][2], l.m[1][1], l.m[1][2], l.m[2][2]};
}

// exp of the mean log-covariance into a column-major 4x4 row (decode_covariance_average / compute_averaged_attributes)
__device__ __forceinline__ void decode_cov(const CovSum& s, float inv, float4* __restrict__ o4) {
    Mat3 m;
    m.m[0][0] = s.xx * inv; m.m[0][1] = m.m[1][0] = s.xy * inv; m.m[0][2] = m.m[2][0] = s.xz * inv;
    m.m[1][1] = s.yy * inv; m.m[1][2] = m.m[2][1] = s.yz * inv; m.m[2][2] = s.zz * inv;
    const Mat3 e = spd_map<false>(m);
    o4[0] = make_float4(e.m[0][0], e.m[1][0], e.m[2][0], 0.0f);
    o4[1] = make_float4(e.m[0][1], e.m[1][1], e.m[2][1], 0.0f);
    o4[2] = make_float4(e.m[0][2], e.m[1][2], e.m[2][2], 0.0f);
    o4[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// atomic_ref<float, relaxed, device>::fetch_add with the result unused: the hardware's no-return global_atomic_add_f32 (plain
// atomicAdd(float*) compiles to a compare-and-swap loop without -munsafe-fp-atomics; the tables are hipMalloc memory, where the
// hardware form is valid)
__device__ __forceinline__ void fadd(float* p, float v) { unsafeAtomicAdd(p, v); }

inline Mat4Arg pose_arg(const float* pose16) { return query_pose(pose16, 0); }  // a host pose by value, the identity for none

constexpr unsigned long long kNoSlot = ~0ull;

// Passed to kernels by value. Core is the map's own 16- or 32-byte record; the other five arrays mean the same in both maps.
template <class Core>
struct VoxelTable {
    uint64_t* key;
    Core* core;
    CovSum* cov;  // sums of log(C) (upper triangle)
    float4* color;
    float* intensity;
    uint32_t* last_update;
    unsigned long long capacity;
};

// the arrays of an averaged export; cov / rgb / inten / keys may be null
struct MeanRows {
    float4 *pts, *cov, *rgb;
    float* inten;
    uint64_t* keys;
};

// The read-only probe (find_voxel, compute_overlap_ratio): the key's slot, or kNoSlot at the first never-used slot or after kProbes.
template <unsigned kProbes>
__device__ __forceinline__ unsigned long long find_slot(const uint64_t* keys, unsigned long long cap, uint64_t h) {
    for (unsigned p = 0; p < kProbes; ++p) {
        const unsigned long long s = slot_id(h, p, cap);
        const uint64_t k = keys[s];
        if (k == h) return s;
        if (k == kInvalidKey) return kNoSlot;
    }
    return kNoSlot;
}

// What a hit adds to slot s besides the core: 6 + 4 + 1 relaxed float atomics, each group only where the map keeps it. A caller
// that must not even load or encode an attribute it does not add (ogm_hit_kernel) calls the groups under its own conditions.
template <class Core>
__device__ __forceinline__ void add_cov_sums(const VoxelTable<Core>& t, unsigned long long s, const CovSum& cv) {
    float* c = reinterpret_cast<float*>(t.cov + s);
    fadd(c + 0, cv.xx); fadd(c + 1, cv.xy); fadd(c + 2, cv.xz);
    fadd(c + 3, cv.yy); fadd(c + 4, cv.yz); fadd(c + 5, cv.zz);
}
template <class Core>
__device__ __forceinline__ void add_color_sums(const VoxelTable<Core>& t, unsigned long long s, const float4 col) {
    float* c = reinterpret_cast<float*>(t.color + s);
    fadd(c + 0, col.x); fadd(c + 1, col.y); fadd(c + 2, col.z); fadd(c + 3, col.w);
}
template <class Core>
__device__ __forceinline__ void add_attributes(const VoxelTable<Core>& t, unsigned long long s, const CovSum& cv, bool has_cov,
                                               const float4 col, bool has_rgb, float inten, bool has_intensity) {
    if (has_cov) add_cov_sums(t, s, cv);
    if (has_rgb) add_color_sums(t, s, col);
    if (has_intensity) fadd(t.intensity + s, inten);
}

template <class Core>
__device__ __forceinline__ void stamp(const VoxelTable<Core>& t, unsigned long long s, uint32_t when) {
    __hip_atomic_store(t.last_update + s, when, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// compute_averaged_attributes into row o of a compacted output: slot i's sums over its count
template <class Core>
__device__ __forceinline__ void write_mean_row(const VoxelTable<Core>& t, unsigned long long i, unsigned o, unsigned count, float sx,
                                               float sy, float sz, const MeanRows& out) {
    const float inv = 1.0f / (float)count;
    out.pts[o] = make_float4(sx * inv, sy * inv, sz * inv, 1.0f);
    if (out.cov) decode_cov(t.cov[i], inv, out.cov + 4 * (size_t)o);  // column-major 4x4, 3x3 block used
    if (out.rgb) {
        const float4 k = t.color[i];
        out.rgb[o] = make_float4(k.x * inv, k.y * inv, k.z * inv, k.w * inv);
    }
    if (out.inten) out.inten[o] = t.intensity[i] * inv;
    if (out.keys) out.keys[o] = t.key[i];
}

namespace {

__global__ void voxel_table_fill_keys_kernel(uint64_t* keys, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) keys[i] = kInvalidKey;
}
__global__ void voxel_table_seed_kernel(unsigned* counter, unsigned v0, unsigned v1, unsigned v2) {
    counter[0] = v0; counter[1] = v1; counter[2] = v2;
}

// compute_overlap_ratio of either map: one lane per point, transform -> key -> probe -> `counts(core)` -> wave sum -> one atomic
template <unsigned kProbes, class Core, class Pred>
__global__ __launch_bounds__(kBlock) void voxel_table_overlap_kernel(VoxelTable<Core> t, const float4* __restrict__ pts, unsigned n,
                                                                     Mat4Arg pose, float inv, Pred counts,
                                                                     unsigned* __restrict__ hits) {
    const Rigid T = load_rigid_colmajor(pose.m);
    unsigned mine = 0;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float4 p = pts[i];
        float wx, wy, wz;
        transform_point(T, p.x, p.y, p.z, wx, wy, wz);
        const uint64_t h = voxel_key3(wx, wy, wz, inv);
        if (h == kInvalidKey) continue;
        const unsigned long long s = find_slot<kProbes>(t.key, t.capacity, h);
        if (s != kNoSlot && counts(t.core[s])) ++mine;
    }
    mine = wave_sum_u32(mine);
    if ((threadIdx.x & (kWave - 1)) == 0 && mine) atomicAdd(hits, mine);  // integer: exact, order-independent
}

template <class Core>
void free_table(VoxelTable<Core>& t) {
    (void)hipFree(t.key); (void)hipFree(t.core); (void)hipFree(t.cov); (void)hipFree(t.color); (void)hipFree(t.intensity);
    (void)hipFree(t.last_update);
    t = VoxelTable<Core>{};
}

// allocate_storage: keys invalid, everything else zero
template <class Core>
int alloc_table(VoxelTable<Core>& t, size_t cap, hipStream_t st) {
    hipError_t e = hipMalloc(&t.key, cap * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&t.core, cap * sizeof(Core));
    if (e == hipSuccess) e = hipMalloc(&t.cov, cap * sizeof(CovSum));
    if (e == hipSuccess) e = hipMalloc(&t.color, cap * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc(&t.intensity, cap * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&t.last_update, cap * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(t.core, 0, cap * sizeof(Core), st);
    if (e == hipSuccess) e = hipMemsetAsync(t.cov, 0, cap * sizeof(CovSum), st);
    if (e == hipSuccess) e = hipMemsetAsync(t.color, 0, cap * sizeof(float4), st);
    if (e == hipSuccess) e = hipMemsetAsync(t.intensity, 0, cap * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(t.last_update, 0, cap * sizeof(uint32_t), st);
    if (e != hipSuccess) { sp_set_error(hipGetErrorString(e)); free_table(t); return SP_ERR_HIP; }
    t.capacity = cap;
    voxel_table_fill_keys_kernel<<<div_up(cap, kBlock), kBlock, 0, st>>>(t.key, cap);
    return launch_status();
}

// The host side both maps are built on; sp_voxel_hash_map and sp_occupancy_grid_map inherit it and add their own settings.
template <class Core>
struct VoxelMapState {
    float voxel_size = 0.0f, voxel_size_inv = 0.0f;
    float rehash_threshold = 0.7f;
    size_t voxel_num = 0;
    bool has_cov = false, has_rgb = false, has_intensity = false;
    VoxelTable<Core> t{};
    unsigned* counter = nullptr;  // device, 4 words: the voxel count / hit count / result of the running call in the first
    unsigned *flags = nullptr, *pos = nullptr;  // compaction scratch, sized to the capacity + 1
    unsigned* list = nullptr;                   // the flagged slots as a dense list (OccupancyGridMap's candidates), sized with them
    size_t scratch_cap = 0;
    void* scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;

    int read_counter(hipStream_t st, unsigned* out, int words = 1) const {
        if (hipMemcpyAsync(out, counter, words * sizeof(unsigned), hipMemcpyDeviceToHost, st) != hipSuccess) return SP_ERR_HIP;
        return hip_status(hipStreamSynchronize(st));  // the reference waits here too (wait_and_throw + shared read)
    }
    int write_counter(hipStream_t st, unsigned v0, unsigned v1 = 0, unsigned v2 = 0) const {
        // the values travel in the kernarg segment: nothing is read from a host variable after this returns
        voxel_table_seed_kernel<<<1, 1, 0, st>>>(counter, v0, v1, v2);
        return launch_status();
    }
    // launch_status of the kernel just launched, then its count from the counter's first word into voxel_num
    int read_voxel_num(hipStream_t st) {
        unsigned cnt = 0;
        int rc = launch_status();
        if (rc == SP_OK) rc = read_counter(st, &cnt);
        if (rc == SP_OK) voxel_num = cnt;
        return rc;
    }
    void note_attributes(const float* covs, const float* rgb, const float* intensities) {
        has_cov |= covs != nullptr;
        has_rgb |= rgb != nullptr;
        has_intensity |= intensities != nullptr;
    }

    // rehash: a table of new_cap slots, the counter at zero, launch_rehash(old, new) moves the live slots and counts them there
    template <class Launch>
    int grow(size_t new_cap, hipStream_t st, Launch launch_rehash) {
        if (t.capacity >= new_cap) return SP_OK;
        VoxelTable<Core> old_t = t, new_t{};
        int rc = alloc_table(new_t, new_cap, st);
        if (rc != SP_OK) return rc;
        if ((rc = write_counter(st, 0)) == SP_OK) {
            launch_rehash(old_t, new_t);
            rc = read_voxel_num(st);
        }
        if (rc != SP_OK) { free_table(new_t); return rc; }
        t = new_t;
        free_table(old_t);
        return SP_OK;
    }
    // ensure_rehash: one rung up the ladder when the table is fuller than rehash_threshold
    template <class Launch>
    int ensure_rehash(hipStream_t st, Launch launch_rehash) {
        if (!(rehash_threshold < (float)voxel_num / (float)t.capacity)) return SP_OK;
        return grow(next_capacity((size_t)t.capacity), st, launch_rehash);
    }

    // The slot-order compaction of every export: ensure_scratch, the map's own flag kernel into `flags`, scan_flags, the map's
    // writer kernel over flags / pos, read_total.
    int ensure_scratch() {
        const size_t cap = (size_t)t.capacity;
        if (scratch_cap >= cap) return SP_OK;
        (void)hipFree(flags); (void)hipFree(pos); (void)hipFree(list); (void)hipFree(scan_tmp);
        flags = pos = list = nullptr; scan_tmp = nullptr; scratch_cap = 0;
        const size_t tmp = exclusive_scan_u32_workspace_bytes(cap + 1);
        hipError_t e = hipMalloc(&flags, (cap + 1) * sizeof(unsigned));
        if (e == hipSuccess) e = hipMalloc(&pos, (cap + 1) * sizeof(unsigned));
        if (e == hipSuccess) e = hipMalloc(&list, (cap + 1) * sizeof(unsigned));
        if (e == hipSuccess) e = hipMalloc(&scan_tmp, tmp ? tmp : 16);
        if (e != hipSuccess) { sp_set_error(hipGetErrorString(e)); return SP_ERR_HIP; }
        scan_tmp_bytes = tmp;
        scratch_cap = cap;
        return SP_OK;
    }
    int scan_flags(hipStream_t st) {  // pos[i] = the output row of slot i, pos[capacity] = the number of rows
        const size_t cap = (size_t)t.capacity;
        if (hipMemsetAsync(flags + cap, 0, sizeof(unsigned), st) != hipSuccess) return SP_ERR_HIP;
        if (exclusive_scan_u32(flags, pos, cap + 1, nullptr, scan_tmp, scan_tmp_bytes, st) != SP_OK) {
            sp_set_error("[voxel table] scan failed");
            return SP_ERR_HIP;
        }
        return SP_OK;
    }
    int read_total(hipStream_t st, size_t* n_out) {  // after the writer kernel: its launch status, then the wait
        unsigned total = 0;
        int rc = launch_status();
        if (rc == SP_OK && hipMemcpyAsync(&total, pos + t.capacity, sizeof(unsigned), hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = SP_ERR_HIP;
        if (rc == SP_OK) rc = hip_status(hipStreamSynchronize(st));
        if (rc == SP_OK) *n_out = total;
        return rc;
    }
    // the arrays an averaged export writes: an attribute the map holds no sums of is left out
    MeanRows mean_rows(float* points, float* covs, float* rgb, float* intensities, uint64_t* keys) const {
        return MeanRows{reinterpret_cast<float4*>(points), has_cov ? reinterpret_cast<float4*>(covs) : nullptr,
                        has_rgb ? reinterpret_cast<float4*>(rgb) : nullptr, has_intensity ? intensities : nullptr, keys};
    }

    // compute_overlap_ratio: the share of the n points whose voxel the map holds and `counts` accepts
    template <unsigned kProbes, class Pred>
    int overlap_ratio(Pred counts, const float* points, size_t n, const float* pose16, float* ratio_out, hipStream_t st) const {
        if (!ratio_out) return SP_ERR_INVALID_ARGUMENT;
        *ratio_out = 0.0f;
        if (n == 0 || !points || voxel_num == 0) return SP_OK;
        if (n >= (1ull << 32)) { sp_set_error("[voxel map] more than 2^32 points"); return SP_ERR_INVALID_ARGUMENT; }
        int rc = write_counter(st, 0);
        if (rc != SP_OK) return rc;
        voxel_table_overlap_kernel<kProbes><<<stream_grid(n), kBlock, 0, st>>>(t, reinterpret_cast<const float4*>(points), (unsigned)n,
                                                                               pose_arg(pose16), voxel_size_inv, counts, counter);
        unsigned hits = 0;
        rc = launch_status();
        if (rc == SP_OK) rc = read_counter(st, &hits);
        if (rc == SP_OK) *ratio_out = (float)hits / (float)n;
        return rc;
    }

    // create and clear: a fresh table on the first rung, no voxels, no attributes; the old table goes only once the new one stands
    int reset_to_first_capacity(hipStream_t st) {
        int rc = counter ? SP_OK : hip_status(hipMalloc(&counter, 4 * sizeof(unsigned)));
        VoxelTable<Core> fresh{};
        if (rc == SP_OK) rc = alloc_table(fresh, kCapacityCandidates[0], st);
        if (rc == SP_OK) rc = hip_status(hipStreamSynchronize(st));
        if (rc != SP_OK) { free_table(fresh); return rc; }
        free_table(t);
        t = fresh;
        voxel_num = 0;
        has_cov = has_rgb = has_intensity = false;
        return SP_OK;
    }
    void release() {
        free_table(t);
        (void)hipFree(counter); (void)hipFree(flags); (void)hipFree(pos); (void)hipFree(list); (void)hipFree(scan_tmp);
        counter = flags = pos = list = nullptr; scan_tmp = nullptr; scratch_cap = 0;
    }
};

// sp_*_create / sp_*_destroy of a map type that inherits VoxelMapState
template <class Map>
int create_map(float voxel_size, void* stream, Map** out) {
    if (!out) return SP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!(voxel_size > 0.0f)) {
        sp_set_error("voxel_size must be positive.");  // voxel_hash_map.hpp:41-43, occupancy_grid_map.hpp:74-76
        return SP_ERR_INVALID_ARGUMENT;
    }
    Map* m = new Map();
    m->voxel_size = voxel_size;
    m->voxel_size_inv = 1.0f / voxel_size;
    const int rc = m->reset_to_first_capacity(as_stream(stream));
    if (rc != SP_OK) { m->release(); delete m; return rc; }
    *out = m;
    return SP_OK;
}
template <class Map>
void destroy_map(Map* m) {
    if (!m) return;
    m->release();
    delete m;
}

}  // namespace
}  // namespace sp
