// The wave form of the iteration finish (csrc/sp_wave_solve.h) in its host lockstep form against the one-lane code it
// replaces, bit for bit: wave_ldlt6_solve against ldlt6_solve (x, dmin, the ok flag), wave_gn_update against
// sp_gn_update_host (T, delta8). A program with its own main; built with hipcc's host compiler only and -ffp-contract=off, as
// the library is (tests/test_wave_solve_cpu.py).
//   test_wave_solve              run the comparisons, print one summary line per group, exit 1 on any difference
//   test_wave_solve --dump FILE  also write every case as 49 floats (30 totals, T, lambda, crit_rot, crit_trans): the
//                                cases tests/test_gpu_wave_solve.py sends through the device's wave form
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../sycl_points_amd/csrc/sp_wave_solve.h"
#include "../../include/sycl_points_amd.h"

extern "C" int sp_gn_update_host(const sp_linearized* lin_host, float* T_host, float lambda, float crit_rotation,
                                 float crit_translation, float* delta_out8_host);
extern "C" void sp_se3_exp_host(const float* twist6, float* T_out16);

namespace {

struct System {
    float H[36];
    float rhs[6];
};
struct GnCase {
    float tot[30];
    float T[16];
    float lambda, crit_rot, crit_trans;
};

// The same bits — or NaN on both sides: IEEE 754 leaves the sign and the payload of a NaN result open, x86 hands on the FIRST NaN
// operand of an addition or a product, and a compiler may commute the two operands of either (seen here: nan against -nan in the
// translation of a pose whose rotation is NaN, where 0 * inf meets a NaN in one sum). Every other value must agree in every bit.
bool same_bits(const float* a, const float* b, int n) {
    for (int i = 0; i < n; ++i)
        if (std::memcmp(a + i, b + i, sizeof(float)) != 0 && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
    return true;
}

System make_system(const double Hd[6][6], const double* rhs) {
    System s;
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) s.H[i * 6 + j] = (float)Hd[std::min(i, j)][std::max(i, j)];
        s.rhs[i] = (float)rhs[i];
    }
    return s;
}
// a symmetric matrix with the given diagonal and small off-diagonal entries
System diagonal_system(const double d[6], std::mt19937& g, double off) {
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    double Hd[6][6] = {}, rhs[6];
    for (int i = 0; i < 6; ++i) {
        for (int j = i + 1; j < 6; ++j) Hd[i][j] = off * u(g);
        Hd[i][i] = d[i];
        rhs[i] = u(g);
    }
    return make_system(Hd, rhs);
}
// J^T J + I with J uniform in (-1, 1), 30 x 6, symmetrised in float: the systems of tests/test_cabi.py
System random_spd(std::mt19937& g) {
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    double J[30][6];
    for (auto& row : J)
        for (double& v : row) v = u(g);
    float Hf[6][6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = i == j ? 1.0 : 0.0;
            for (int k = 0; k < 30; ++k) s += J[k][i] * J[k][j];
            Hf[i][j] = (float)s;
        }
    System s;
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) s.H[i * 6 + j] = (Hf[i][j] + Hf[j][i]) * 0.5f;
        s.rhs[i] = (float)u(g);
    }
    return s;
}

struct Solved {
    float x[6];
    float dmin;
    bool ok;
};
Solved solve_one_lane(const System& s) {
    Solved r;
    sp::LdltScratch w;
    r.ok = sp::ldlt6_solve(s.H, s.rhs, r.x, w, &r.dmin);
    return r;
}
template <bool REVERSED>
Solved solve_wave(const System& s) {
    Solved r;
    sp::WaveLanesHost w;
    w.each([&](sp::WaveLane& l) {
        for (int c = 0; c < 6; ++c) l.m[c] = s.H[l.r * 6 + c];
        l.y = s.rhs[l.r];
    });
    r.ok = sp::wave_ldlt6_solve<REVERSED>(w, r.x, &r.dmin);
    return r;
}

GnCase gn_case_of(const System& s) {  // the solve as an iteration finish: H as it is (lambda 0), b = -rhs, the identity pose
    GnCase c{};
    for (int a = 0; a < 6; ++a) {
        for (int cc = a; cc < 6; ++cc) c.tot[sp::tri6(a, cc)] = s.H[a * 6 + cc];
        c.tot[21 + a] = -s.rhs[a];
    }
    c.tot[27] = 1.0f;
    c.T[0] = c.T[5] = c.T[10] = c.T[15] = 1.0f;
    return c;
}
sp_linearized lin_of(const GnCase& c) {
    sp_linearized lin{};
    for (int a = 0; a < 6; ++a) {
        for (int cc = a; cc < 6; ++cc) lin.H[a * 6 + cc] = lin.H[cc * 6 + a] = c.tot[sp::tri6(a, cc)];
        lin.b[a] = c.tot[21 + a];
    }
    lin.error = c.tot[27];
    return lin;
}
struct GnOut {
    float T[16];
    float d8[8];
};
GnOut gn_one_lane(const GnCase& c) {
    GnOut o;
    const sp_linearized lin = lin_of(c);
    std::memcpy(o.T, c.T, sizeof(o.T));
    sp_gn_update_host(&lin, o.T, c.lambda, c.crit_rot, c.crit_trans, o.d8);
    return o;
}
GnOut gn_wave(const GnCase& c) {
    GnOut o;
    std::memcpy(o.T, c.T, sizeof(o.T));
    sp::WaveLanesHost w;
    float x[6];
    sp::wave_gn_update(w, c.tot, o.T, c.lambda, c.crit_rot, c.crit_trans, o.d8, x);
    return o;
}

}  // namespace

int main(int argc, char** argv) {
    std::string dump;
    for (int i = 1; i + 1 < argc; ++i)
        if (std::string(argv[i]) == "--dump") dump = argv[i + 1];
    std::mt19937 g(20241);
    std::vector<System> sys;
    std::vector<std::pair<std::string, size_t>> groups;  // name, index one past the group's last system
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    {  // every ordering of the diagonal's magnitudes: every exchange target at every step
        int p[6] = {0, 1, 2, 3, 4, 5};
        do {
            double d[6];
            for (int i = 0; i < 6; ++i) d[i] = (double)(1 << p[i]) * 1.5;
            sys.push_back(diagonal_system(d, g, 0.05));
        } while (std::next_permutation(p, p + 6));
        groups.push_back({"orderings", sys.size()});
    }
    {  // equal |diagonal| pairs and triples with every sign pattern (the lowest index must win), all equal, all negative
        for (int i = 0; i < 6; ++i)
            for (int j = i + 1; j < 6; ++j)
                for (int sg = 0; sg < 4; ++sg) {
                    double d[6] = {1.0, 1.25, 1.5, 1.75, 2.0, 2.25};
                    d[i] = (sg & 1) ? -8.0 : 8.0;
                    d[j] = (sg & 2) ? -8.0 : 8.0;
                    sys.push_back(diagonal_system(d, g, 0.05));
                    for (int l = j + 1; l < 6; ++l) {
                        d[l] = (sg == 1) ? -8.0 : 8.0;
                        sys.push_back(diagonal_system(d, g, 0.05));
                        d[l] = 1.0 + 0.25 * l;
                    }
                }
        for (int sg = 0; sg < 64; ++sg) {
            double d[6];
            for (int i = 0; i < 6; ++i) d[i] = (sg >> i & 1) ? -3.0 : 3.0;
            sys.push_back(diagonal_system(d, g, sg % 2 ? 0.05 : 0.0));
        }
        groups.push_back({"ties and signs", sys.size()});
    }
    {  // zero pivots. A zero column under them: ok stays true, the guarded division gives y = 0
        const double rhs[6] = {1, -2, 3, -4, 5, -6};
        for (int rank = 0; rank < 6; ++rank) {
            double Hd[6][6] = {};
            for (int i = 0; i < rank; ++i) Hd[(i * 5 + 2) % 6][(i * 5 + 2) % 6] = 2.0 + i;
            sys.push_back(make_system(Hd, rhs));
        }
        {  // rank one with exact arithmetic: v v^T, v powers of two
            double Hd[6][6];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) Hd[i][j] = (double)(1 << i) * (double)(1 << j);
            sys.push_back(make_system(Hd, rhs));
        }
        groups.push_back({"zero pivot, zero column", sys.size()});
        // a non-zero column under a zero pivot, at every step: ok false, x = 0
        for (int k = 0; k < 5; ++k)
            for (int j = k + 1; j < 6; ++j) {
                double Hd[6][6] = {};
                for (int i = 0; i < k; ++i) Hd[i][i] = 8.0 - i;
                Hd[k][j] = 1.0;
                sys.push_back(make_system(Hd, rhs));
            }
        groups.push_back({"zero pivot, non-zero column", sys.size()});
    }
    {  // a diagonal entry of D at FLT_MIN and one ulp either side of it, either sign, in every position
        const float around[3] = {std::nextafterf(FLT_MIN, 0.0f), FLT_MIN, std::nextafterf(FLT_MIN, 1.0f)};
        for (int pos = 0; pos < 6; ++pos)
            for (float a : around)
                for (float sg : {1.0f, -1.0f}) {
                    double Hd[6][6] = {}, rhs[6];
                    for (int i = 0; i < 6; ++i) { Hd[i][i] = 1.0 + i; rhs[i] = 1.0 + 0.5 * i; }
                    Hd[pos][pos] = (double)(sg * a);
                    rhs[pos] = (double)FLT_MIN * 3.0;
                    sys.push_back(make_system(Hd, rhs));
                }
        groups.push_back({"FLT_MIN guard", sys.size()});
    }
    {  // tiny and huge entries; NaN and +-inf in H and in rhs
        for (int i = 0; i < 100; ++i) {
            System s = random_spd(g);
            const float sc = (i & 1) ? 1e30f : 1e-30f;
            for (float& v : s.H) v *= sc;
            if (i & 2) for (float& v : s.rhs) v *= sc;
            sys.push_back(s);
        }
        groups.push_back({"scaled 1e-30 / 1e30", sys.size()});
        const float bad[3] = {nan, inf, -inf};
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j)
                for (float v : bad) {
                    System s = random_spd(g);
                    s.H[i * 6 + j] = s.H[j * 6 + i] = v;
                    sys.push_back(s);
                }
        for (int i = 0; i < 6; ++i)
            for (float v : bad) {
                System s = random_spd(g);
                s.rhs[i] = v;
                sys.push_back(s);
            }
        groups.push_back({"NaN and inf", sys.size()});
    }
    const size_t random_begin = sys.size();
    for (int i = 0; i < 2000; ++i) sys.push_back(random_spd(g));
    groups.push_back({"random SPD", sys.size()});

    int failures = 0;
    size_t at = 0, reordered_differs = 0;
    for (const auto& grp : groups) {
        size_t differ = 0, not_ok = 0;
        const size_t begin = at;
        for (; at < grp.second; ++at) {
            const Solved a = solve_one_lane(sys[at]), b = solve_wave<false>(sys[at]);
            if (!(a.ok == b.ok && same_bits(a.x, b.x, 6) && same_bits(&a.dmin, &b.dmin, 1))) ++differ;
            if (!a.ok) ++not_ok;
            if (at >= random_begin) {
                const Solved c = solve_wave<true>(sys[at]);
                if (!same_bits(a.x, c.x, 6)) ++reordered_differs;
            }
        }
        std::printf("solve, %s: %zu systems, %zu differ, %zu not ok\n", grp.first.c_str(), grp.second - begin, differ, not_ok);
        failures += differ != 0;
    }
    std::printf("reordered back substitution (descending j) differs on %zu of %zu random systems\n", reordered_differs,
                sys.size() - random_begin);

    // ---- the Gauss-Newton update
    std::vector<GnCase> gn;
    for (const System& s : sys) gn.push_back(gn_case_of(s));
    const size_t gn_solver_cases = gn.size();
    std::uniform_real_distribution<float> uf(-1.0f, 1.0f);
    auto random_pose = [&](float* T) {
        float tw[6];
        for (int i = 0; i < 6; ++i) tw[i] = uf(g) * (i < 3 ? 1.5f : 10.0f);
        sp_se3_exp_host(tw, T);
    };
    size_t small_theta = 0, mid_theta = 0, big_theta = 0, conv_set = 0;
    // |delta| from far below the theta < 1e-6 branch to theta of order 1 (and beyond pi); criteria 0 and ordinary ones
    const float scales[] = {1e-9f, 1e-8f, 3e-7f, 9e-7f, 1.1e-6f, 3e-6f, 1e-5f, 3e-4f, 9e-4f, 1.1e-3f, 1e-2f, 0.1f, 0.5f, 1.0f, 2.0f, 4.0f};
    for (float sc : scales)
        for (int rep = 0; rep < 40; ++rep) {
            const System s = random_spd(g);
            GnCase c = gn_case_of(s);
            // H = J^T J + I has eigenvalues of order 10: b of order 10 * sc gives a step of order sc
            for (int a = 0; a < 6; ++a) c.tot[21 + a] = s.rhs[a] * 10.0f * sc;
            random_pose(c.T);
            c.lambda = (rep & 1) ? 1e-6f : 0.5f;
            c.crit_rot = (rep & 2) ? 0.0f : 1e-3f;
            c.crit_trans = (rep & 2) ? 0.0f : 1e-3f;
            gn.push_back(c);
            // ... and the criteria at |delta| exactly and one ulp either side of it
            const GnOut o = gn_one_lane(c);
            const float nr = std::sqrt(o.d8[0] * o.d8[0] + o.d8[1] * o.d8[1] + o.d8[2] * o.d8[2]);
            const float nt = std::sqrt(o.d8[3] * o.d8[3] + o.d8[4] * o.d8[4] + o.d8[5] * o.d8[5]);
            if (rep < 6) {
                for (int e = 0; e < 9; ++e) {
                    GnCase c2 = c;
                    const float cr[3] = {std::nextafterf(nr, 0.0f), nr, std::nextafterf(nr, inf)};
                    const float ct[3] = {std::nextafterf(nt, 0.0f), nt, std::nextafterf(nt, inf)};
                    c2.crit_rot = cr[e % 3];
                    c2.crit_trans = ct[e / 3];
                    gn.push_back(c2);
                }
            }
            if (nr < 1e-6f) ++small_theta;
            else if (nr * nr < 1e-6f) ++mid_theta;
            else ++big_theta;
        }
    size_t gn_differ = 0;
    for (size_t i = 0; i < gn.size(); ++i) {
        const GnOut a = gn_one_lane(gn[i]), b = gn_wave(gn[i]);
        if (!(same_bits(a.T, b.T, 16) && same_bits(a.d8, b.d8, 8))) {
            if (++gn_differ <= 4) {
                std::printf("update case %zu differs:", i);
                for (int e = 0; e < 16; ++e)
                    if (!same_bits(a.T + e, b.T + e, 1)) std::printf(" T[%d] %a / %a", e, a.T[e], b.T[e]);
                for (int e = 0; e < 8; ++e)
                    if (!same_bits(a.d8 + e, b.d8 + e, 1)) std::printf(" d8[%d] %a / %a", e, a.d8[e], b.d8[e]);
                std::printf("\n");
            }
        }
        if (i >= gn_solver_cases && a.d8[6] > 0.5f) ++conv_set;
    }
    std::printf("update: %zu cases (%zu of them the systems above), %zu differ; theta < 1e-6: %zu, theta^2 < 1e-6: %zu, larger: %zu; "
                "converged flag set in %zu\n", gn.size(), gn_solver_cases, gn_differ, small_theta, mid_theta, big_theta, conv_set);
    failures += gn_differ != 0;

    if (!dump.empty()) {
        FILE* f = std::fopen(dump.c_str(), "wb");
        if (!f) { std::perror("dump"); return 2; }
        for (const GnCase& c : gn) {
            std::fwrite(c.tot, sizeof(float), 30, f);
            std::fwrite(c.T, sizeof(float), 16, f);
            const float p[3] = {c.lambda, c.crit_rot, c.crit_trans};
            std::fwrite(p, sizeof(float), 3, f);
        }
        std::fclose(f);
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
