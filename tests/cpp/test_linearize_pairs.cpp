// Host check of the per-point algebra of the prepared GICP / point-to-distribution linearisation (csrc/sp_linearize.h,
// linearize_terms — the function the kernels' fused_math calls): its 28 weighted terms and the error, bit for bit against a plain
// scalar statement of the same formulas kept HERE — fmaf chains written out, nothing shared with the header but the robust kernels
// of sp_math.h. However the header's body is arranged (single floats today; pairs of floats for packed arithmetic were tried), a
// swapped pair, a term in another slot of the row, or an operation whose rounding differs shows as a different bit pattern.
//
// 100 000 random correspondences, each through GICP and point-to-distribution, the five losses, the terms and the error-only form.
// Among them: a fixed rotation whose nine entries are all distinct and non-zero; covariances so small that |det| < 1e-6 (the
// inverse is Zero); a zero source covariance; negative coordinates throughout.
//
// Built by tests/test_linearize_pairs_cpu.py with hipcc's HOST compiler only (the header is HIP source), once more under
// -fsanitize=address,undefined. No device, no library.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../sycl_points_amd/csrc/sp_linearize.h"

namespace {

float ch3(float a0, float b0, float a1, float b1, float a2, float b2) {
    return std::fmaf(a2, b2, std::fmaf(a1, b1, std::fmaf(a0, b0, 0.0f)));
}

struct Sym {
    float xx, xy, xz, yy, yz, zz;
};

// The formulas, one float per value (the order of a partial row: 21 H upper triangle, 6 b, error).
template <int LOSS, bool P2D>
void scalar_terms(const float R[3][3], float px, float py, float pz, float qx, float qy, float qz, float tx, float ty, float tz,
                  const Sym& Cs, const Sym& Ct, float scale, float out[28]) {
    const float r0 = tx - qx, r1 = ty - qy, r2 = tz - qz;
    float W[3][3];
    for (int j = 0; j < 3; ++j) {
        W[0][j] = ch3(Ct.xx, R[0][j], Ct.xy, R[1][j], Ct.xz, R[2][j]);
        W[1][j] = ch3(Ct.xy, R[0][j], Ct.yy, R[1][j], Ct.yz, R[2][j]);
        W[2][j] = ch3(Ct.xz, R[0][j], Ct.yz, R[1][j], Ct.zz, R[2][j]);
    }
    const float g00 = ch3(R[0][0], W[0][0], R[1][0], W[1][0], R[2][0], W[2][0]);
    const float g01 = ch3(R[0][0], W[0][1], R[1][0], W[1][1], R[2][0], W[2][1]);
    const float g02 = ch3(R[0][0], W[0][2], R[1][0], W[1][2], R[2][0], W[2][2]);
    const float g11 = ch3(R[0][1], W[0][1], R[1][1], W[1][1], R[2][1], W[2][1]);
    const float g12 = ch3(R[0][1], W[0][2], R[1][1], W[1][2], R[2][1], W[2][2]);
    const float g22 = ch3(R[0][2], W[0][2], R[1][2], W[1][2], R[2][2], W[2][2]);
    float n00, n01, n02, n11, n12, n22;
    if (P2D) {
        n00 = g00; n01 = g01; n02 = g02; n11 = g11; n12 = g12; n22 = g22;
    } else {
        const float a00 = g00 + Cs.xx, a01 = g01 + Cs.xy, a02 = g02 + Cs.xz, a11 = g11 + Cs.yy, a12 = g12 + Cs.yz,
                    a22 = g22 + Cs.zz;
        const float c00 = std::fmaf(a11, a22, -a12 * a12);
        const float c01 = std::fmaf(a02, a12, -a01 * a22);
        const float c02 = std::fmaf(a01, a12, -a02 * a11);
        const float det = std::fmaf(a00, c00, std::fmaf(a01, c01, a02 * c02));
        const float inv_det = std::fabs(det) < 1e-6f ? 0.0f : 1.0f / det;
        n00 = c00 * inv_det; n01 = c01 * inv_det; n02 = c02 * inv_det;
        n11 = std::fmaf(a00, a22, -a02 * a02) * inv_det;
        n12 = std::fmaf(a01, a02, -a00 * a12) * inv_det;
        n22 = std::fmaf(a00, a11, -a01 * a01) * inv_det;
    }
    const float v0 = ch3(R[0][0], r0, R[1][0], r1, R[2][0], r2);
    const float v1 = ch3(R[0][1], r0, R[1][1], r1, R[2][1], r2);
    const float v2 = ch3(R[0][2], r0, R[1][2], r1, R[2][2], r2);
    const float u0 = ch3(n00, v0, n01, v1, n02, v2);
    const float u1 = ch3(n01, v0, n11, v1, n12, v2);
    const float u2 = ch3(n02, v0, n12, v1, n22, v2);
    const float sq = ch3(v0, u0, v1, u1, v2, u2);
    const float rn = std::sqrt(sq);
    const float w = sp::robust_weight<LOSS>(rn, scale);
    const float G00 = std::fmaf(py, n02, -pz * n01), G01 = std::fmaf(py, n12, -pz * n11), G02 = std::fmaf(py, n22, -pz * n12);
    const float G10 = std::fmaf(pz, n00, -px * n02), G11 = std::fmaf(pz, n01, -px * n12), G12 = std::fmaf(pz, n02, -px * n22);
    const float G20 = std::fmaf(px, n01, -py * n00), G21 = std::fmaf(px, n11, -py * n01), G22 = std::fmaf(px, n12, -py * n02);
    const float h00 = std::fmaf(G02, py, -G01 * pz), h01 = std::fmaf(G00, pz, -G02 * px), h02 = std::fmaf(G01, px, -G00 * py);
    const float h11 = std::fmaf(G10, pz, -G12 * px), h12 = std::fmaf(G11, px, -G10 * py), h22 = std::fmaf(G21, px, -G20 * py);
    out[0] = w * h00; out[1] = w * h01; out[2] = w * h02; out[3] = w * G00; out[4] = w * G01; out[5] = w * G02;
    out[6] = w * h11; out[7] = w * h12; out[8] = w * G10; out[9] = w * G11; out[10] = w * G12;
    out[11] = w * h22; out[12] = w * G20; out[13] = w * G21; out[14] = w * G22;
    out[15] = w * n00; out[16] = w * n01; out[17] = w * n02; out[18] = w * n11; out[19] = w * n12; out[20] = w * n22;
    out[21] = w * std::fmaf(u1, pz, -u2 * py); out[22] = w * std::fmaf(u2, px, -u0 * pz); out[23] = w * std::fmaf(u0, py, -u1 * px);
    out[24] = w * -u0; out[25] = w * -u1; out[26] = w * -u2;
    out[27] = sp::robust_error<LOSS>(rn, scale);
}

struct Case {
    sp::Rigid T;
    float p[3], q[3], t[3];
    Sym Cs, Ct;
    float scale;
};

unsigned long long g_bad = 0, g_checked = 0;

void report(const char* what, int loss, bool p2d, size_t i, int slot, float got, float want) {
    if (g_bad < 20) {
        uint32_t a, b;
        std::memcpy(&a, &got, 4);
        std::memcpy(&b, &want, 4);
        std::printf("MISMATCH %s loss %d %s case %zu slot %d: header %.9g (%08x) restatement %.9g (%08x)\n", what, loss,
                    p2d ? "P2D" : "GICP", i, slot, got, a, want, b);
    }
    ++g_bad;
}

template <int LOSS, bool P2D>
void check(const Case& c, size_t i) {
    float want[28], got[28];
    scalar_terms<LOSS, P2D>(c.T.R, c.p[0], c.p[1], c.p[2], c.q[0], c.q[1], c.q[2], c.t[0], c.t[1], c.t[2], c.Cs, c.Ct, c.scale, want);
    const sp::Sym3 Cs{c.Cs.xx, c.Cs.xy, c.Cs.xz, c.Cs.yy, c.Cs.yz, c.Cs.zz}, Ct{c.Ct.xx, c.Ct.xy, c.Ct.xz, c.Ct.yy, c.Ct.yz, c.Ct.zz};
    sp::linearize_terms<LOSS, P2D, false>(c.T, c.p[0], c.p[1], c.p[2], c.q[0], c.q[1], c.q[2], c.t[0], c.t[1], c.t[2], Cs, Ct, c.scale, got);
    for (int k = 0; k < 28; ++k)
        if (std::memcmp(&got[k], &want[k], 4) != 0) report("terms", LOSS, P2D, i, k, got[k], want[k]);
    float e[1];
    sp::linearize_terms<LOSS, P2D, true>(c.T, c.p[0], c.p[1], c.p[2], c.q[0], c.q[1], c.q[2], c.t[0], c.t[1], c.t[2], Cs, Ct, c.scale, e);
    if (std::memcmp(&e[0], &want[27], 4) != 0) report("error only", LOSS, P2D, i, 27, e[0], want[27]);
    g_checked += 28 + 1;
}

template <bool P2D>
void check_losses(const Case& c, size_t i) {
    check<sp::LOSS_NONE, P2D>(c, i);
    check<sp::LOSS_HUBER, P2D>(c, i);
    check<sp::LOSS_TUKEY, P2D>(c, i);
    check<sp::LOSS_CAUCHY, P2D>(c, i);
    check<sp::LOSS_GEMAN_MCCLURE, P2D>(c, i);
}

void rotation_from_quaternion(float x, float y, float z, float w, float R[3][3]) {
    const float n = std::sqrt(x * x + y * y + z * z + w * w);
    const float q[4] = {x / n, y / n, z / n, w / n};
    sp::quat_to_rot(q, R);
}

Sym random_cov(std::mt19937& rng, float size) {
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    float A[3][3];
    for (auto& row : A)
        for (float& v : row) v = U(rng) * size;
    Sym s;  // A A^T + a small diagonal: symmetric, positive
    s.xx = A[0][0] * A[0][0] + A[0][1] * A[0][1] + A[0][2] * A[0][2] + 1e-3f * size * size;
    s.xy = A[0][0] * A[1][0] + A[0][1] * A[1][1] + A[0][2] * A[1][2];
    s.xz = A[0][0] * A[2][0] + A[0][1] * A[2][1] + A[0][2] * A[2][2];
    s.yy = A[1][0] * A[1][0] + A[1][1] * A[1][1] + A[1][2] * A[1][2] + 1e-3f * size * size;
    s.yz = A[1][0] * A[2][0] + A[1][1] * A[2][1] + A[1][2] * A[2][2];
    s.zz = A[2][0] * A[2][0] + A[2][1] * A[2][1] + A[2][2] * A[2][2] + 1e-3f * size * size;
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 100000;
    std::mt19937 rng(20260719u);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    size_t zero_inverse = 0, zero_cs = 0, negative = 0, distinct = 0;
    for (size_t i = 0; i < n; ++i) {
        Case c;
        if (i % 4 == 0) rotation_from_quaternion(0.3f, -0.5f, 0.2f, 0.7f, c.T.R);  // nine distinct non-zero entries
        else rotation_from_quaternion(U(rng), U(rng), U(rng), U(rng) + 1.5f, c.T.R);
        bool all_distinct = true;
        for (int a = 0; a < 9; ++a) {
            if (c.T.R[a / 3][a % 3] == 0.0f) all_distinct = false;
            for (int b = 0; b < a; ++b)
                if (c.T.R[a / 3][a % 3] == c.T.R[b / 3][b % 3]) all_distinct = false;
        }
        distinct += all_distinct;
        for (int k = 0; k < 3; ++k) {
            c.T.t[k] = 5.0f * U(rng);
            c.p[k] = 50.0f * U(rng);
            if (c.p[k] < 0.0f) ++negative;
        }
        sp::transform_point(c.T, c.p[0], c.p[1], c.p[2], c.q[0], c.q[1], c.q[2]);
        const float reach = (i % 3 == 0) ? 2.0f : 0.05f;  // far and near winners: both sides of the robust scales
        for (int k = 0; k < 3; ++k) c.t[k] = c.q[k] + reach * U(rng);
        float size = 0.3f;
        if (i % 11 == 0) size = 0.02f;  // |det(Cs' + R^T Ct' R)| of the order 1e-9: the inverse is Zero
        c.Cs = random_cov(rng, size);
        c.Ct = random_cov(rng, size);
        if (i % 7 == 0) {
            c.Cs = Sym{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            ++zero_cs;
        }
        c.scale = 0.05f + 1.5f * std::fabs(U(rng));
        {  // count the Zero-inverse inputs with the scalar statement's own determinant
            float o[28];
            scalar_terms<sp::LOSS_NONE, false>(c.T.R, c.p[0], c.p[1], c.p[2], c.q[0], c.q[1], c.q[2], c.t[0], c.t[1], c.t[2], c.Cs, c.Ct,
                                               c.scale, o);
            if (o[15] == 0.0f && o[18] == 0.0f && o[20] == 0.0f) ++zero_inverse;
        }
        check_losses<false>(c, i);
        check_losses<true>(c, i);
    }
    std::printf("%zu cases: %llu values compared, %llu differ; Zero inverse %zu, zero source covariance %zu, negative coordinates %zu, "
                "rotations with nine distinct non-zero entries %zu\n",
                n, g_checked, g_bad, zero_inverse, zero_cs, negative, distinct);
    if (n >= 1000 && (zero_inverse == 0 || zero_cs == 0 || negative == 0 || distinct == 0)) {
        std::printf("an edge case the test is about did not occur\n");
        return 2;
    }
    return g_bad == 0 ? 0 : 1;
}
