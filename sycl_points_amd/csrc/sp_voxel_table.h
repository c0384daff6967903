// What the two hashed voxel maps share (voxel_hash_map.hip, occupancy_grid_map.hip): the 63-bit voxel key, the double-hashed slot
// sequence, the capacity ladder, the log-Euclidean covariance encoding and the no-return float atomic. The reference keeps a copy
// of each in both classes (mapping/voxel_hash_map.hpp, mapping/occupancy_grid_map.hpp); here there is one.
#pragma once
#include "sp_common.h"
#include "sp_math.h"

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

inline Mat4Arg pose_arg(const float* pose16) {
    Mat4Arg a;
    for (int i = 0; i < 16; ++i) a.m[i] = pose16 ? pose16[i] : ((i % 5 == 0) ? 1.0f : 0.0f);
    return a;
}

}  // namespace sp
