// The normal of a covariance as K7 forms it, shared by every kernel that needs one (covariance.hip's K6 / K7, scan_refine.hip's
// angle-of-incidence kernels): one definition, so that a normal taken from a covariance inside another kernel carries the bits
// sp_normals_from_cov would have stored for the same row.
#pragma once
#include "sp_math.h"

namespace sp {

__device__ __forceinline__ Mat3 load_cov(const float4* __restrict__ in) {
    const float4 c0 = in[0], c1 = in[1], c2 = in[2];
    Mat3 C;
    C.m[0][0] = c0.x; C.m[1][0] = c0.y; C.m[2][0] = c0.z;
    C.m[0][1] = c1.x; C.m[1][1] = c1.y; C.m[2][1] = c1.z;
    C.m[0][2] = c2.x; C.m[1][2] = c2.y; C.m[2][2] = c2.z;
    return C;
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
