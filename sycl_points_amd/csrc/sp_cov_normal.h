// A covariance from the sums over a neighbourhood as K5 forms it, and the normal of a covariance as K7 forms it, shared by every
// kernel that needs one (covariance.hip's K5 - K8, grid.hip's fused self-kNN epilogues, scan_refine.hip's angle-of-incidence
// kernels): one definition each, so that a covariance or a normal made inside another kernel carries the bits sp_cov_estimate /
// sp_normals_from_cov would have stored for the same row.
#pragma once
#include "sp_math.h"

namespace sp {

// the 3x3 block of a stored covariance's first three columns (column-major storage: C(i, k) is component i of column k)
__device__ __forceinline__ Mat3 cov_of_columns(const float4 c0, const float4 c1, const float4 c2) {
    Mat3 C;
    C.m[0][0] = c0.x; C.m[1][0] = c0.y; C.m[2][0] = c0.z;
    C.m[0][1] = c1.x; C.m[1][1] = c1.y; C.m[2][1] = c1.z;
    C.m[0][2] = c2.x; C.m[1][2] = c2.y; C.m[2][2] = c2.z;
    return C;
}
__device__ __forceinline__ Mat3 load_cov(const float4* __restrict__ in) { return cov_of_columns(in[0], in[1], in[2]); }

__device__ __forceinline__ void store_cov(float4* __restrict__ out, const Mat3& C) {
    out[0] = make_float4(C.m[0][0], C.m[1][0], C.m[2][0], 0.0f);  // column 0
    out[1] = make_float4(C.m[0][1], C.m[1][1], C.m[2][1], 0.0f);
    out[2] = make_float4(C.m[0][2], C.m[1][2], C.m[2][2], 0.0f);
    out[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__device__ __forceinline__ Mat3 identity3() {
    Mat3 C;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C.m[i][j] = (i == j) ? 1.0f : 0.0f;
    return C;
}

// The tail of covariance::kernel::estimate (covariance.hpp:41-46): mean = sums * inv, (sum_outer * inv) - outer(mean, mean), then
// ensure_symmetric (eigen_utils.hpp:208-219): (a + a) * 0.5. outer(p, p) is bitwise symmetric (p_i * p_j == p_j * p_i), so six
// sums carry all nine entries. `inv`: 1 / the number of neighbours, or 1 / their total weight.
__device__ __forceinline__ Mat3 cov_from_scaled_sums(float sx, float sy, float sz, float oxx, float oxy, float oxz, float oyy,
                                                     float oyz, float ozz, float inv, float& mx, float& my, float& mz) {
    mx = sx * inv; my = sy * inv; mz = sz * inv;
    const float cxx = oxx * inv - mx * mx, cxy = oxy * inv - mx * my, cxz = oxz * inv - mx * mz;
    const float cyy = oyy * inv - my * my, cyz = oyz * inv - my * mz, czz = ozz * inv - mz * mz;
    const float sxy = (cxy + cxy) * 0.5f, sxz = (cxz + cxz) * 0.5f, syz = (cyz + cyz) * 0.5f;
    Mat3 C;
    C.m[0][0] = cxx; C.m[0][1] = sxy; C.m[0][2] = sxz;
    C.m[1][0] = sxy; C.m[1][1] = cyy; C.m[1][2] = syz;
    C.m[2][0] = sxz; C.m[2][1] = syz; C.m[2][2] = czz;
    return C;
}
// ... of `cnt` neighbours; the identity when fewer than 4 (covariance.hpp:34-39). 1.0f / correspondences (size_t -> float).
__device__ __forceinline__ Mat3 cov_from_sums(float sx, float sy, float sz, float oxx, float oxy, float oxz, float oyy, float oyz,
                                              float ozz, unsigned cnt) {
    if (cnt < 4) return identity3();
    float mx, my, mz;
    return cov_from_scaled_sums(sx, sy, sz, oxx, oxy, oxz, oyy, oyz, ozz, 1.0f / (float)cnt, mx, my, mz);
}

// covariance::kernel::extract_normal (covariance.hpp:49-65): smallest-eigenvalue eigenvector, flipped when n.p > 1.
__device__ __forceinline__ float4 normal_of(const Mat3& C, const float4 p) {
    float ev[3];
    Mat3 V;
    symmetric_eigen3(C, ev, V);
    const float nx = V.m[0][0], ny = V.m[1][0], nz = V.m[2][0];
    const float d = chain3(nx, p.x, ny, p.y, nz, p.z);
    if (d <= 1.0f) return make_float4(nx, ny, nz, 0.0f);
    return make_float4(-nx, -ny, -nz, 0.0f);
}

}  // namespace sp
