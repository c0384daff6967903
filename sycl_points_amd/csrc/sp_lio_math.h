// Host-only dense algebra of the 15-DoF LiDAR-inertial alignment (lio_host.hip): Eigen's pivoted LDL^T and the Powell dog-leg
// step for any size up to 15. No kernel includes this header. The LDL^T is the algorithm of ldlt6_solve (sp_math.h) with run-time
// loops; Eigen's reductions are restated as plain ascending sums, as everywhere in this library.
// Matrices are column-major with leading dimension n: A(i, j) = A[j * n + i].
#pragma once
#include <cfloat>
#include <cmath>

namespace sp {

constexpr int kLioMaxN = 15;

// Eigen::LDLT<Matrix<float, N, N>>: compute() once, solve() any number of right-hand sides.
struct LdltN {
    int n = 0;
    float m[kLioMaxN][kLioMaxN];
    int perm[kLioMaxN];
    bool ok = false;    // info() == Success
    float dmin = 0.0f;  // vectorD().minCoeff()

    void compute(const float* A, int size) {
        n = size;
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < n; ++j) m[i][j] = A[j * n + i];
            perm[i] = i;
        }
        ok = true;
        for (int k = 0; k < n; ++k) {
            int piv = k;
            float best = fabsf(m[k][k]);
            for (int i = k + 1; i < n; ++i)
                if (fabsf(m[i][i]) > best) { best = fabsf(m[i][i]); piv = i; }
            if (piv != k) {
                for (int j = 0; j < n; ++j) { const float t = m[k][j]; m[k][j] = m[piv][j]; m[piv][j] = t; }
                for (int i = 0; i < n; ++i) { const float t = m[i][k]; m[i][k] = m[i][piv]; m[i][piv] = t; }
                const int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t;
            }
            float temp[kLioMaxN];
            for (int j = 0; j < k; ++j) temp[j] = m[j][j] * m[k][j];
            if (k > 0) {
                float s = 0.0f;
                for (int j = 0; j < k; ++j) s += m[k][j] * temp[j];
                m[k][k] -= s;
                for (int i = k + 1; i < n; ++i) {
                    float t = 0.0f;
                    for (int j = 0; j < k; ++j) t += m[i][j] * temp[j];
                    m[i][k] -= t;
                }
            }
            const float d = m[k][k];
            if (fabsf(d) > 0.0f) {
                for (int i = k + 1; i < n; ++i) m[i][k] /= d;
            } else {
                for (int i = k + 1; i < n; ++i)
                    if (m[i][k] != 0.0f) ok = false;
            }
        }
        dmin = m[0][0];
        for (int i = 1; i < n; ++i) dmin = m[i][i] < dmin ? m[i][i] : dmin;
    }

    bool positive() const { return ok && dmin > 0.0f; }

    // x = A^-1 rhs (P^T L^-T D^-1 L^-1 P rhs); x may be rhs
    void solve(const float* rhs, float* x) const {
        float y[kLioMaxN];
        for (int i = 0; i < n; ++i) y[i] = rhs[perm[i]];
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < i; ++j) y[i] -= m[i][j] * y[j];
        for (int i = 0; i < n; ++i) y[i] = (fabsf(m[i][i]) > FLT_MIN) ? y[i] / m[i][i] : 0.0f;
        for (int i = n - 1; i >= 0; --i)
            for (int j = i + 1; j < n; ++j) y[i] -= m[j][i] * y[j];
        for (int i = 0; i < n; ++i) x[perm[i]] = y[i];
    }

    // solveInPlace(Identity): column by column
    void inverse(float* out) const {
        for (int c = 0; c < n; ++c) {
            float e[kLioMaxN];
            for (int i = 0; i < n; ++i) e[i] = (i == c) ? 1.0f : 0.0f;
            solve(e, out + c * n);
        }
    }
};

inline float dot_n(const float* a, const float* b, int n) {
    float s = 0.0f;
    for (int i = 0; i < n; ++i) s += a[i] * b[i];
    return s;
}
inline void matvec_n(const float* A, const float* v, float* out, int n) {  // out must not be v
    for (int i = 0; i < n; ++i) {
        float s = 0.0f;
        for (int j = 0; j < n; ++j) s += A[j * n + i] * v[j];
        out[i] = s;
    }
}

// compute_dogleg_step<N> (algorithms/registration/dogleg_step.hpp:33-102), the arithmetic of dogleg_step6 (sp_math.h) for any n
struct DoglegStepN {
    float p[kLioMaxN];
    float step_norm, predicted_reduction;
};
inline DoglegStepN dogleg_step_n(const float* H, const float* g, float radius, int n) {
    DoglegStepN r;
    for (int i = 0; i < kLioMaxN; ++i) r.p[i] = 0.0f;
    r.step_norm = 0.0f;
    r.predicted_reduction = 0.0f;
    float p_gn[kLioMaxN], ng[kLioMaxN];
    for (int i = 0; i < n; ++i) { p_gn[i] = 0.0f; ng[i] = -g[i]; }
    float norm_gn = 0.0f;
    bool has_gn = false;
    {
        LdltN ldlt;
        ldlt.compute(H, n);
        if (ldlt.positive()) {
            ldlt.solve(ng, p_gn);
            norm_gn = sqrtf(dot_n(p_gn, p_gn, n));
            has_gn = fabsf(norm_gn) <= FLT_MAX;  // std::isfinite
        }
    }
    const float g2 = dot_n(g, g, n);
    float Hg[kLioMaxN];
    matvec_n(H, g, Hg, n);
    const float gHg = dot_n(g, Hg, n);
    float p_sd[kLioMaxN];
    for (int i = 0; i < n; ++i) p_sd[i] = -g[i];
    if (gHg > FLT_EPSILON) {
        const float alpha = g2 / gHg;
        if (fabsf(alpha) <= FLT_MAX)
            for (int i = 0; i < n; ++i) p_sd[i] = -alpha * g[i];
    }
    const float norm_sd = sqrtf(dot_n(p_sd, p_sd, n));
    if (has_gn && norm_gn <= radius) {
        for (int i = 0; i < n; ++i) r.p[i] = p_gn[i];
        r.step_norm = norm_gn;
    } else if (norm_sd >= radius) {
        if (norm_sd > FLT_EPSILON) {
            const float sc = radius / norm_sd;
            for (int i = 0; i < n; ++i) r.p[i] = sc * p_sd[i];
        }
        r.step_norm = radius;
    } else if (has_gn) {
        float diff[kLioMaxN];
        for (int i = 0; i < n; ++i) diff[i] = p_gn[i] - p_sd[i];
        const float a = dot_n(diff, diff, n);
        const float b = 2.0f * dot_n(p_sd, diff, n);
        const float c = dot_n(p_sd, p_sd, n) - radius * radius;
        float disc = b * b - 4.0f * a * c;
        disc = disc < 0.0f ? 0.0f : disc;
        float tau = 0.0f;
        if (a > FLT_EPSILON) tau = (-b + sqrtf(disc)) / (2.0f * a);
        tau = tau < 0.0f ? 0.0f : (1.0f < tau ? 1.0f : tau);
        for (int i = 0; i < n; ++i) r.p[i] = p_sd[i] + tau * diff[i];
        r.step_norm = sqrtf(dot_n(r.p, r.p, n));
    } else {
        for (int i = 0; i < n; ++i) r.p[i] = p_sd[i];
        if (norm_sd > radius && norm_sd > FLT_EPSILON) {
            const float sc = radius / norm_sd;
            for (int i = 0; i < n; ++i) r.p[i] *= sc;
            r.step_norm = radius;
        } else {
            r.step_norm = norm_sd;
        }
    }
    float Hp[kLioMaxN];
    matvec_n(H, r.p, Hp, n);
    r.predicted_reduction = -(dot_n(g, r.p, n) + 0.5f * dot_n(r.p, Hp, n));
    return r;
}

}  // namespace sp
