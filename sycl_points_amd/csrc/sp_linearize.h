// The per-point algebra of the prepared GICP / point-to-distribution linearisation as one host + device function, so that a host
// program can hold it, bit for bit, against a plain restatement of the formulas (tests/cpp/test_linearize_pairs.cpp).
//
// It is written on single floats and the two translation units that run it (registration.hip, registration_opt.hip) are compiled
// with -fno-slp-vectorize. On gfx950 a packed v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 occupies the vector unit as long as the
// two single operations it replaces, so packing buys nothing here — neither the compiler's own (SLP: pairs that are adjacent
// nowhere, glued with 46 register moves per point, and permuted pairs of R that overflow the scalar registers into 28
// v_readlane_b32 reloads) nor pairs chosen by hand so that nothing has to be moved (scratch/experiments/
// r07_hand_paired_linearisation.patch: 199 vector instructions per certified point against 238, the same time). What costs is
// every instruction that is not arithmetic.
// DESIGN.md §A, profiles/r07_a_*.
#pragma once
#include "sp_math.h"

namespace sp {

struct Sym3 {
    float xx, xy, xz, yy, yz, zz;
};

constexpr int kLinTerms = 28;  // 21 H (upper triangle, row-major) + 6 b + error: the order of a partial row

// Linearisation of one correspondence: source point s with q = T s, winner t, prepared covariances Cs' (source) and Ct'
// (target); out = what the point adds to the 28 sums, already weighted.
// Source-frame form of factor.hpp:239-278. With S = skew(s), J = [R S | -R] and M = (Ct' + R Cs' R^T)^-1:
//   N := R^T M R = (Cs' + R^T Ct' R)^-1,  v := R^T r,  u := N v,  G := S N
//   H = [[-G S, G], [G^T, N]],   b = [u x s, -u],   e = v . u
// (same mathematics as J^T M J / J^T M r, about half the multiply-adds).
// P2D (linearize_point_to_distribution, factor.hpp:311-354): Ct' is the target's information matrix M = inverse(Ct_raw)
// (prepared once per target) and there is no source covariance: N = R^T M R, nothing to invert per point.
// ERR_ONLY (calculate_gicp_error / calculate_point_to_distribution_error, factor.hpp:280-306, 356-373): only the robust
// error, into out[0].
template <int LOSS, bool P2D, bool ERR_ONLY, int NOUT>
SP_HD void linearize_terms(const Rigid& T, float px, float py, float pz, float qx, float qy, float qz, float tx, float ty,
                           float tz, const Sym3& Cs, const Sym3& Ct, float scale, float (&out)[NOUT]) {
    static_assert(NOUT == (ERR_ONLY ? 1 : kLinTerms), "28 terms, or the error alone");
    const float r0 = tx - qx, r1 = ty - qy, r2 = tz - qz;
    const float (&R)[3][3] = T.R;
    float W[3][3];  // W = Ct' R
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        W[0][j] = chain3(Ct.xx, R[0][j], Ct.xy, R[1][j], Ct.xz, R[2][j]);
        W[1][j] = chain3(Ct.xy, R[0][j], Ct.yy, R[1][j], Ct.yz, R[2][j]);
        W[2][j] = chain3(Ct.xz, R[0][j], Ct.yz, R[1][j], Ct.zz, R[2][j]);
    }
    // A = Cs' + R^T Ct' R (symmetric); P2D: R^T M R with no source term, and A is N itself
    const float g00 = chain3(R[0][0], W[0][0], R[1][0], W[1][0], R[2][0], W[2][0]);
    const float g01 = chain3(R[0][0], W[0][1], R[1][0], W[1][1], R[2][0], W[2][1]);
    const float g02 = chain3(R[0][0], W[0][2], R[1][0], W[1][2], R[2][0], W[2][2]);
    const float g11 = chain3(R[0][1], W[0][1], R[1][1], W[1][1], R[2][1], W[2][1]);
    const float g12 = chain3(R[0][1], W[0][2], R[1][1], W[1][2], R[2][1], W[2][2]);
    const float g22 = chain3(R[0][2], W[0][2], R[1][2], W[1][2], R[2][2], W[2][2]);
    float n00, n01, n02, n11, n12, n22;
    if constexpr (P2D) {
        n00 = g00; n01 = g01; n02 = g02; n11 = g11; n12 = g12; n22 = g22;
    } else {
        const float a00 = g00 + Cs.xx, a01 = g01 + Cs.xy, a02 = g02 + Cs.xz, a11 = g11 + Cs.yy, a12 = g12 + Cs.yz,
                    a22 = g22 + Cs.zz;
        // symmetric inverse by the adjugate; Zero when |det| < 1e-6 (eigen_utils::inverse, eigen_utils.hpp:403-423;
        // det is invariant under the rotation)
        const float c00 = fmaf(a11, a22, -a12 * a12);
        const float c01 = fmaf(a02, a12, -a01 * a22);
        const float c02 = fmaf(a01, a12, -a02 * a11);
        const float det = fmaf(a00, c00, fmaf(a01, c01, a02 * c02));
        const float inv_det = fabsf(det) < 1e-6f ? 0.0f : 1.0f / det;
        n00 = c00 * inv_det; n01 = c01 * inv_det; n02 = c02 * inv_det;
        n11 = fmaf(a00, a22, -a02 * a02) * inv_det;
        n12 = fmaf(a01, a02, -a00 * a12) * inv_det;
        n22 = fmaf(a00, a11, -a01 * a01) * inv_det;
    }
    const float v0 = chain3(R[0][0], r0, R[1][0], r1, R[2][0], r2);
    const float v1 = chain3(R[0][1], r0, R[1][1], r1, R[2][1], r2);
    const float v2 = chain3(R[0][2], r0, R[1][2], r1, R[2][2], r2);
    const float u0 = chain3(n00, v0, n01, v1, n02, v2);
    const float u1 = chain3(n01, v0, n11, v1, n12, v2);
    const float u2 = chain3(n02, v0, n12, v1, n22, v2);
    const float sq = chain3(v0, u0, v1, u1, v2, u2);
    const float rn = sqrtf(sq);
    if constexpr (ERR_ONLY) {
        out[0] = robust_error<LOSS>(rn, scale);
    } else {
        const float w = robust_weight<LOSS>(rn, scale);
        // G = S N, rows: s x (columns of N)
        const float G00 = fmaf(py, n02, -pz * n01), G01 = fmaf(py, n12, -pz * n11), G02 = fmaf(py, n22, -pz * n12);
        const float G10 = fmaf(pz, n00, -px * n02), G11 = fmaf(pz, n01, -px * n12), G12 = fmaf(pz, n02, -px * n22);
        const float G20 = fmaf(px, n01, -py * n00), G21 = fmaf(px, n11, -py * n01), G22 = fmaf(px, n12, -py * n02);
        // H_rr = -G S (symmetric)
        const float h00 = fmaf(G02, py, -G01 * pz), h01 = fmaf(G00, pz, -G02 * px), h02 = fmaf(G01, px, -G00 * py);
        const float h11 = fmaf(G10, pz, -G12 * px), h12 = fmaf(G11, px, -G10 * py), h22 = fmaf(G21, px, -G20 * py);
        out[0] = w * h00; out[1] = w * h01; out[2] = w * h02; out[3] = w * G00; out[4] = w * G01; out[5] = w * G02;
        out[6] = w * h11; out[7] = w * h12; out[8] = w * G10; out[9] = w * G11; out[10] = w * G12;
        out[11] = w * h22; out[12] = w * G20; out[13] = w * G21; out[14] = w * G22;
        out[15] = w * n00; out[16] = w * n01; out[17] = w * n02; out[18] = w * n11; out[19] = w * n12; out[20] = w * n22;
        // b = [u x s, -u]
        out[21] = w * fmaf(u1, pz, -u2 * py); out[22] = w * fmaf(u2, px, -u0 * pz); out[23] = w * fmaf(u0, py, -u1 * px);
        out[24] = w * -u0; out[25] = w * -u1; out[26] = w * -u2;
        out[27] = robust_error<LOSS>(rn, scale);
    }
}

}  // namespace sp
