// The finish of a Gauss-Newton iteration — the pivoted 6x6 LDL^T solve (ldlt6_solve, sp_math.h) and the pose update
// (gn_update_impl, registration_device.h) — on the lanes of ONE wave instead of one lane: lane r < 6 holds row r of the working
// matrix in six registers and the row's right-hand side, lane e < 16 ends with word e of the pose.
//
// The arithmetic is ldlt6_solve's and gn_update_impl's, operation for operation: the file is compiled with -ffp-contract=off, so
// every +, -, *, / below is one IEEE operation, and an operation gives the same bits on whichever lane it runs. Only what is
// independent runs side by side:
//   * step k of the left-looking factorisation: the dot products that update m[i][k], i >= k, and the divisions by the pivot;
//   * the six divisions by the diagonal between the two substitutions;
//   * sinf / cosf of the half and of the whole angle (two lanes, one argument each, instead of four calls in a row);
//   * the three rows of the translation's V matrix, the sixteen words of the updated pose.
// What stays a chain: the pivot choice (strict >, the lowest index wins a tie), the forward substitution, and the back
// substitution, whose terms are subtracted in ascending j for every i as ldlt6_solve does — it runs on values every lane holds.
//
// The schedule is written once, as steps over a lane's state (WaveLane) with exchange points between them, against a `Lanes`
// type that says what a wave is:
//   each(f)        run step f on every lane's state
//   get(l, g)      the value g(state) of lane l, the same for every lane (l is a constant once the loops are unrolled)
//   uniform(v)     an int every lane holds with the same value, as one value
// WaveLanesDevice: the state is the calling lane's registers, get is v_readlane_b32 — no LDS, no barrier.
// WaveLanesHost: sixteen states in an array, stepped in lockstep; tests/cpp/test_wave_solve.cpp checks the bits against
// ldlt6_solve and sp_gn_update_host on a machine without a GPU.
#pragma once
#include "sp_math.h"

// A step is a lambda; it is inlined into its caller before anything else looks at it, so that a lane's state and the values the steps
// share are registers from the start (a step compiled on its own sees them behind a pointer, and a choice among them by lane becomes
// an indexed load: the state would live in memory).
#define SP_LANE_STEP __attribute__((always_inline))

namespace sp {

constexpr int kWaveSolveLanes = 16;  // lanes with a part in the finish: 6 matrix rows, 16 words of the pose

struct WaveLane {
    int lane;    // 0 .. kWaveSolveLanes - 1 (the device's lanes past that carry a copy of the last one's work)
    int r;       // the matrix row this lane holds: min(lane, 5)
    float m[6];  // row r of the working matrix
    float y;     // right-hand side / solution entry of row r (it travels with the row when rows are exchanged)
    float dd;    // D's entry of row r, once step r is over
    int bad;     // a non-zero entry under a zero pivot was seen in this row
    float sn, cs;       // sinf, cosf of this lane's angle (lane 0: half the rotation angle, the others: the angle)
    float tv;           // lanes 0 .. 2: entry `lane` of se3_exp's translation
    float L[4];         // row (lane & 3) of the pose before the update: R[i][0 .. 2], t[i]
    float out;          // word `lane` of the updated pose (column-major 4x4)
    float d8;           // lanes 0 .. 7: word `lane` of delta_out8 (delta, converged, ok)
};

struct WaveLanesHost {
    WaveLane s[kWaveSolveLanes];
    WaveLanesHost() {
        for (int l = 0; l < kWaveSolveLanes; ++l) {
            s[l] = WaveLane{};
            s[l].lane = l;
            s[l].r = l < 5 ? l : 5;
        }
    }
    template <class F>
    void each(F f) {
        for (int l = 0; l < kWaveSolveLanes; ++l) f(s[l]);
    }
    template <class G>
    float get(int l, G g) const { return g(s[l]); }
    template <class G>
    int get_int(int l, G g) const { return g(s[l]); }
    static int uniform(int v) { return v; }
};

struct WaveLanesDevice {
    WaveLane s;
    __device__ __forceinline__ explicit WaveLanesDevice(unsigned lane_of_wave) {
        s.lane = lane_of_wave < (unsigned)kWaveSolveLanes ? (int)lane_of_wave : kWaveSolveLanes - 1;
        s.r = s.lane < 5 ? s.lane : 5;
        s.bad = 0;
        s.dd = 0.0f;
    }
    template <class F>
    __device__ __forceinline__ void each(F f) { f(s); }
    template <class G>
    __device__ __forceinline__ float get(int l, G g) const {
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g(s)), l));
    }
    template <class G>
    __device__ __forceinline__ int get_int(int l, G g) const { return __builtin_amdgcn_readlane(g(s), l); }
    static __device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
};

// c ? a : b on VALUES. (Written with ?: on two array elements, the choice is one between two addresses, and a chain of them by
// lane becomes a load at a run-time index: the array would have to live in memory.)
SP_HD float pick(bool c, float a, float b) { return c ? a : b; }

// Index of H(a, c) among the 21 totals of the upper triangle, row-major: a <= c.
SP_HD int tri6(int a, int c) { return a * 6 - a * (a - 1) / 2 + (c - a); }

// ldlt6_solve on a wave. In: lane r < 6 holds row r of H in s.m and rhs[r] in s.y. Out: x, the same six values on every lane;
// *dmin_out as ldlt6_solve gives it. REVERSED_BACK: the back substitution subtracts in descending j — NOT the library's
// arithmetic, only there so that a test can show that its inputs tell the two orders apart.
template <bool REVERSED_BACK = false, class Lanes>
SP_HD bool wave_ldlt6_solve(Lanes& w, float x[6], float* dmin_out = nullptr) {
    int perm[6];
    float dfin[6];  // the diagonal of D: m[k][k] is final once step k is over
#pragma unroll
    for (int i = 0; i < 6; ++i) perm[i] = i;
    bool zero_pivot = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        // the pivot: the diagonal entries of the rows not yet factored, from the lanes that hold them
        float D[6];
#pragma unroll
        for (int i = k; i < 6; ++i) D[i] = w.get(i, [=](const WaveLane& s) SP_LANE_STEP { return s.m[i]; });
        int piv = k;
        float best = fabsf(D[k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i)
            if (fabsf(D[i]) > best) { best = fabsf(D[i]); piv = i; }
        piv = w.uniform(piv);  // a scalar: `piv == p` is a uniform branch and only the taken exchange executes
#pragma unroll
        for (int p = k + 1; p < 6; ++p) {
            if (piv == p) {
                // rows k and p change lanes (with their right-hand sides), columns k and p change places inside every lane
                float rk[6], rp[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    rk[j] = w.get(k, [=](const WaveLane& s) SP_LANE_STEP { return s.m[j]; });
                    rp[j] = w.get(p, [=](const WaveLane& s) SP_LANE_STEP { return s.m[j]; });
                }
                const float yk = w.get(k, [](const WaveLane& s) SP_LANE_STEP { return s.y; });
                const float yp = w.get(p, [](const WaveLane& s) SP_LANE_STEP { return s.y; });
                w.each([&](WaveLane& s) SP_LANE_STEP {
#pragma unroll
                    for (int j = 0; j < 6; ++j) s.m[j] = pick(s.r == k, rp[j], pick(s.r == p, rk[j], s.m[j]));
                    s.y = pick(s.r == k, yp, pick(s.r == p, yk, s.y));
                    const float t = s.m[k]; s.m[k] = s.m[p]; s.m[p] = t;
                });
                const int t = perm[k]; perm[k] = perm[p]; perm[p] = t;
            }
        }
        if (k > 0) {
            float temp[6];  // m[j][j] * m[k][j]: every lane forms them, from row k
#pragma unroll
            for (int j = 0; j < k; ++j) temp[j] = dfin[j] * w.get(k, [=](const WaveLane& s) SP_LANE_STEP { return s.m[j]; });
            w.each([&](WaveLane& s) SP_LANE_STEP {
                float t = 0.0f;
#pragma unroll
                for (int j = 0; j < 5; ++j)  // (a constant bound: the step is a function of its own, k is not a constant in it)
                    if (j < k) t += s.m[j] * temp[j];
                s.m[k] = s.r >= k ? s.m[k] - t : s.m[k];
            });
        }
        const float d = w.get(k, [=](const WaveLane& s) SP_LANE_STEP { return s.m[k]; });
        dfin[k] = d;
        w.each([&](WaveLane& s) SP_LANE_STEP { s.dd = s.r == k ? d : s.dd; });
        if (fabsf(d) > 0.0f) {
            w.each([&](WaveLane& s) SP_LANE_STEP { s.m[k] = s.r > k ? s.m[k] / d : s.m[k]; });
        } else {
            zero_pivot = true;
            w.each([&](WaveLane& s) SP_LANE_STEP {
                if (s.r > k && s.m[k] != 0.0f) s.bad = 1;
            });
        }
    }
    if (dmin_out) {  // ldlt.vectorD().minCoeff()
        float dm = dfin[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) dm = dfin[i] < dm ? dfin[i] : dm;
        *dmin_out = dm;
    }
    bool ok = true;
    if (zero_pivot) {
#pragma unroll
        for (int i = 1; i < 6; ++i)
            if (w.get_int(i, [](const WaveLane& s) SP_LANE_STEP { return s.bad; }) != 0) ok = false;
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 6; ++i) x[i] = 0.0f;
        return false;
    }
    // forward substitution: y[j] goes to every lane as it becomes final, lane i subtracts in ascending j
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float yj = w.get(j, [](const WaveLane& s) SP_LANE_STEP { return s.y; });
        w.each([&](WaveLane& s) SP_LANE_STEP { s.y = s.r > j ? s.y - s.m[j] * yj : s.y; });
    }
    w.each([&](WaveLane& s) SP_LANE_STEP { s.y = (fabsf(s.dd) > FLT_MIN) ? s.y / s.dd : 0.0f; });
    // back substitution on values every lane holds, in ldlt6_solve's order
    float Y[6], Lt[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        Y[i] = w.get(i, [](const WaveLane& s) SP_LANE_STEP { return s.y; });
#pragma unroll
        for (int j = i + 1; j < 6; ++j) Lt[j][i] = w.get(j, [=](const WaveLane& s) SP_LANE_STEP { return s.m[i]; });
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        if (!REVERSED_BACK) {
#pragma unroll
            for (int j = i + 1; j < 6; ++j) Y[i] -= Lt[j][i] * Y[j];
        } else {
#pragma unroll
            for (int j = 5; j > i; --j) Y[i] -= Lt[j][i] * Y[j];
        }
    }
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        float v = 0.0f;
#pragma unroll
        for (int i = 0; i < 6; ++i) v = (perm[i] == t) ? Y[i] : v;
        x[t] = v;
    }
    return true;
}

// gn_update_impl on a wave, from the 30 totals of an iteration (tot: 21 sums of H's upper triangle row-major, 6 of b, ...):
// (H + lambda I) delta = -b, T <- T * se3_exp(delta) in place, delta_out8 = delta, converged, ok. delta (the raw solution of
// the LDL^T solve) is left in x on every lane. T and delta_out8 are read and written by the lanes side by side: on the device
// they may be LDS or global memory of the one wave that calls this.
template <bool REVERSED_BACK = false, class Lanes>
SP_HD void wave_gn_update(Lanes& w, const float* tot, float* T, float lambda, float crit_rot, float crit_trans, float* delta_out8,
                          float x[6]) {
    w.each([&](WaveLane& s) SP_LANE_STEP {
        const int pre = tri6(s.r, s.r) - s.r;  // tri6(r, c) = pre + c for r <= c
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float h = tot[s.r <= c ? pre + c : tri6(c, c) - c + s.r];
            s.m[c] = s.r == c ? h + lambda * 1.0f : h;
        }
        s.y = -tot[21 + s.r];
        s.bad = 0;
        // the pose before the update: lane e = 4 j + i needs row i
        const int i = (s.lane & 3) < 3 ? (s.lane & 3) : 2;
        s.L[0] = T[i]; s.L[1] = T[4 + i]; s.L[2] = T[8 + i]; s.L[3] = T[12 + i];
    });
    const bool ok = wave_ldlt6_solve<REVERSED_BACK>(w, x);
    const float nr = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    const float nt = sqrtf(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
    const bool conv = ok && (nr < crit_rot) && (nt < crit_trans);
    // se3_exp(x) (sp_math.h), the same expressions
    const float theta_sq = chain3(x[0], x[0], x[1], x[1], x[2], x[2]);
    const float theta = sqrtf(theta_sq);
    const float half = 0.5f * theta;
    float sin_half = 0.0f, cos_half = 0.0f, sin_theta = 0.0f, cos_theta = 0.0f;
    if (!(theta < 1e-6f)) {  // (the only case in which se3_exp or so3_exp call sinf / cosf)
        w.each([&](WaveLane& s) SP_LANE_STEP {
            const float a = s.lane == 0 ? half : theta;
            s.sn = sinf(a);
            s.cs = cosf(a);
        });
        sin_half = w.get(0, [](const WaveLane& s) SP_LANE_STEP { return s.sn; });
        cos_half = w.get(0, [](const WaveLane& s) SP_LANE_STEP { return s.cs; });
        sin_theta = w.get(1, [](const WaveLane& s) SP_LANE_STEP { return s.sn; });
        cos_theta = w.get(1, [](const WaveLane& s) SP_LANE_STEP { return s.cs; });
    }
    float imag, real;
    if (theta_sq < 1e-6f) {
        const float t4 = theta_sq * theta_sq;
        imag = 0.5f - 1.0f / 48.0f * theta_sq + 1.0f / 3840.0f * t4;
        real = 1.0f - 1.0f / 8.0f * theta_sq + 1.0f / 384.0f * t4;
    } else {
        imag = sin_half / theta;
        real = cos_half;
    }
    const float q[4] = {imag * x[0], imag * x[1], imag * x[2], real};
    float R[3][3];
    quat_to_rot(q, R);
    if (theta < 1e-6f) {
        w.each([&](WaveLane& s) SP_LANE_STEP {
            const int i = s.lane < 2 ? s.lane : 2;
            const float r0 = pick(i == 0, R[0][0], pick(i == 1, R[1][0], R[2][0]));
            const float r1 = pick(i == 0, R[0][1], pick(i == 1, R[1][1], R[2][1]));
            const float r2 = pick(i == 0, R[0][2], pick(i == 1, R[1][2], R[2][2]));
            s.tv = chain3(r0, x[3], r1, x[4], r2, x[5]);
        });
    } else {
        const float A = (1.0f - cos_theta) / theta_sq;
        const float B = (theta - sin_theta) / (theta_sq * theta);
        w.each([&](WaveLane& s) SP_LANE_STEP {  // lane i < 3: row i of O, of O * O, of V, then t[i]
            const int i = s.lane < 2 ? s.lane : 2;
            Mat3 O;
            O.m[0][0] = 0.0f;  O.m[0][1] = -x[2]; O.m[0][2] = x[1];
            O.m[1][0] = x[2];  O.m[1][1] = 0.0f;  O.m[1][2] = -x[0];
            O.m[2][0] = -x[1]; O.m[2][1] = x[0];  O.m[2][2] = 0.0f;
            float Oi[3], Vr[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) Oi[j] = pick(i == 0, O.m[0][j], pick(i == 1, O.m[1][j], O.m[2][j]));
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float o2 = chain3(Oi[0], O.m[0][j], Oi[1], O.m[1][j], Oi[2], O.m[2][j]);
                Vr[j] = ((i == j) ? 1.0f : 0.0f) + (Oi[j] * A + o2 * B);
            }
            s.tv = chain3(Vr[0], x[3], Vr[1], x[4], Vr[2], x[5]);
        });
    }
    float t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = w.get(i, [](const WaveLane& s) SP_LANE_STEP { return s.tv; });
    // rigid_mul(cur, upd) and store_rigid_colmajor: lane e = 4 j + i forms word e of the column-major 4x4
    w.each([&](WaveLane& s) SP_LANE_STEP {
        const int i = s.lane & 3, j = s.lane >> 2;
        const float c0 = pick(j == 0, R[0][0], pick(j == 1, R[0][1], pick(j == 2, R[0][2], t[0])));
        const float c1 = pick(j == 0, R[1][0], pick(j == 1, R[1][1], pick(j == 2, R[1][2], t[1])));
        const float c2 = pick(j == 0, R[2][0], pick(j == 1, R[2][1], pick(j == 2, R[2][2], t[2])));
        float v = 0.0f;
        v += s.L[0] * c0;
        v += s.L[1] * c1;
        v += s.L[2] * c2;
        v = j == 3 ? v + s.L[3] : v;
        s.out = i == 3 ? (j == 3 ? 1.0f : 0.0f) : v;
        T[s.lane] = s.out;
    });
    w.each([&](WaveLane& s) SP_LANE_STEP {
        float v = x[0];
#pragma unroll
        for (int e = 1; e < 6; ++e) v = pick(s.lane == e, x[e], v);
        v = s.lane == 6 ? (conv ? 1.0f : 0.0f) : v;
        v = s.lane == 7 ? (ok ? 1.0f : 0.0f) : v;
        s.d8 = v;
        if (delta_out8 && s.lane < 8) delta_out8[s.lane] = v;
    });
}

}  // namespace sp
