// Device code shared by the translation units of the registration path (registration.hip: K11 / K12 / K13, the prepared
// iteration, the per-iteration and the persistent Gauss-Newton launches; registration_opt.hip: the device-resident optimiser
// loop for Levenberg-Marquardt / Powell dog-leg / annealed robust scales). Everything here is inline / template code in an
// anonymous namespace, or a plain struct: each translation unit gets its own copy, nothing is exported.
#ifndef SP_REGISTRATION_DEVICE_H
#define SP_REGISTRATION_DEVICE_H

#include "grid_device.h"
#include "radix_sort.h"
#include "sp_linearize.h"
#include "sp_xchg.h"

#include <type_traits>

void sp_set_error(const char* msg);

#include "sp_internal.h"

namespace sp {
namespace {

constexpr int kAcc = 29;       // 21 H (upper, row-major) + 6 b + error + count
constexpr int kPartial = 32;   // floats per workgroup partial
constexpr int kMaxBlocks = 1024;

// Sum NV lane values over the workgroup in a fixed order and let lane e < NV of wave 0 write partial[e].
// count_as_float: the count slot holds the VALUE as a float (exact below 2^24) instead of the uint32 bit pattern, so
// that partial rows can be summed across ranks by a float all-reduce.
// `extra` is a second integer (the number of points this launch had to search for, fused kernels only); its sum goes to slot
// NV + 1 as a float VALUE (exact below 2^24), so it survives the float row sums of the next prologue / an all-reduce.
// SC1: the row is stored write-through at agent scope (global_store ... sc1) because another workgroup of the SAME launch
// will read it (the fan-in of the sharded loop, fanin_reduce below); plain stores otherwise.
template <bool SC1>
__device__ __forceinline__ void store_row_word(float* p, float v) {
    if (SC1) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
template <bool SC1>
__device__ __forceinline__ float load_row_word(const float* p) {
    return SC1 ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
constexpr bool lanes_hold_row(int nv) {  // after wave_reduce_transposed: value l in lane l, the two integers in lanes nv, nv + 1
    for (int l = 0; l < nv; ++l)
        if (wave_transposed_value(nv, (unsigned)l) != l) return false;
    return wave_transposed_value(2, (unsigned)nv) == 0 && wave_transposed_value(2, (unsigned)nv + 1) == 1;
}
// First stage of both block reductions: the wave's NV sums and its two integers into row[0 .. NV + 1] (the integers as bit
// patterns). One value: the ladder to lane 63. More: wave_reduce_transposed (sp_common.h: the ladder's tree, the same bits),
// after which lane l < NV holds the total of value l and lanes NV, NV + 1, which only repeat sums, take the two integers; each
// of these lanes writes its one word.
template <int NV>
__device__ __forceinline__ void wave_sums_to_row(float (&acc)[NV], unsigned cnt, unsigned extra, unsigned lane, float* __restrict__ row) {
    if constexpr (NV == 1) {
        acc[0] = wave_sum_to_lane63(acc[0]);
        cnt = wave_sum_u32_to_lane63(cnt);
        extra = wave_sum_u32_to_lane63(extra);
        if (lane == kWave - 1) {
            row[0] = acc[0];
            row[1] = __uint_as_float(cnt);
            row[2] = __uint_as_float(extra);
        }
    } else {
        static_assert(NV + 2 <= kPartial && lanes_hold_row(NV), "lane l < NV must hold value l, lanes NV and NV + 1 the integers 0 and 1");
        unsigned c[2] = {cnt, extra};
        const float s = wave_reduce_transposed(acc, lane);
        const unsigned k = wave_reduce_transposed(c, lane);
        if (lane < NV + 2) row[lane] = lane < NV ? s : __uint_as_float(k);
    }
}

template <int NV, int BLOCK = kBlock, bool SC1 = false>
__device__ __forceinline__ void block_reduce_store(float (&acc)[NV], unsigned cnt, float* __restrict__ partial,
                                                   bool count_as_float = false, unsigned extra = 0) {
    __shared__ float red[BLOCK / kWave][kPartial];
    const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    wave_sums_to_row<NV>(acc, cnt, extra, lane, red[wave]);
    __syncthreads();
    if (threadIdx.x < NV) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < BLOCK / kWave; ++w) s += red[w][threadIdx.x];
        store_row_word<SC1>(partial + threadIdx.x, s);
    } else if (threadIdx.x == NV) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / kWave; ++w) c += __float_as_uint(red[w][NV]);
        store_row_word<SC1>(partial + NV, count_as_float ? (float)c : __uint_as_float(c));
    } else if (threadIdx.x == NV + 1) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / kWave; ++w) c += __float_as_uint(red[w][NV + 1]);
        store_row_word<SC1>(partial + NV + 1, (float)c);
    }
}

// Second stage: one workgroup of 1024 lanes sums the per-workgroup partials in a fixed order:
// lane = (part, slot); a part covers a contiguous range of workgroups (independent loads, summed in order),
// then lanes 0..31 add the 32 parts in order. nv = number of float slots (28 for K11, 1 for K12); slot nv holds the
// uint32 count.
constexpr int kFinalThreads = 1024;

__host__ __device__ inline void gn_update_impl(sp_linearized* lin, float* T, float lambda, float crit_rot,
                                               float crit_trans, float* delta_out8, bool fold_inlier, LdltScratch& w);

// Sum `rows` partial rows with a 1024-lane workgroup in a fixed order: lane = (part, slot); the 32 parts cover
// contiguous row ranges (independent loads, added in row order), then lanes 0..31 add the 32 parts in order.
// On return (after a barrier) red[0][e] holds the totals; slot nv is the uint32 count.
// `after_loads` runs once the row loads have been issued (and before the first barrier): the per-iteration kernel stores
// the previous state there, which it loaded BEFORE the rows, so that both arrive in the same memory round trip.
// AT_MOST_256: the caller's rows never exceed 256 (the per-iteration kernel's grid), so only the first form is compiled — with
// both, loads that `after_loads` issues in one form count as pending in the other and the compiler drains them there.
template <bool SC1 = false, bool AT_MOST_256 = false, typename Hook>
__device__ __forceinline__ void reduce_rows_1024(const float* __restrict__ partials, unsigned rows, int nv,
                                                 float (*red)[kPartial], bool count_is_float, Hook after_loads) {
    constexpr unsigned kParts = kFinalThreads / 32;
    const unsigned e = threadIdx.x & 31, part = threadIdx.x >> 5;
    const unsigned per = (rows + kParts - 1) / kParts;
    const unsigned lo = part * per, hi = min(rows, lo + per);
    float s = 0.0f;
    unsigned c = 0;
    const bool is_count = ((int)e == nv);
    if (AT_MOST_256 || per <= 8) {  // at most 256 rows (the per-iteration kernel): all loads of a lane in flight at once
        float v[8];
#pragma unroll
        for (unsigned j = 0; j < 8; ++j)
            v[j] = (lo + j < hi) ? load_row_word<SC1>(partials + (size_t)(lo + j) * kPartial + e) : 0.0f;
        after_loads();
#pragma unroll
        for (unsigned j = 0; j < 8; ++j) {
            if (lo + j < hi) {
                if (is_count) c += count_is_float ? (unsigned)v[j] : __float_as_uint(v[j]);
                else s += v[j];
            }
        }
    } else {
#pragma unroll 8
        for (unsigned b = lo; b < hi; ++b) {
            const float v = load_row_word<SC1>(partials + (size_t)b * kPartial + e);
            if (is_count) c += count_is_float ? (unsigned)v : __float_as_uint(v);
            else s += v;
        }
        after_loads();
    }
    red[part][e] = is_count ? __uint_as_float(c) : s;
    __syncthreads();
    if (threadIdx.x < 32) {
        float t = 0.0f;
        unsigned ct = 0;
#pragma unroll
        for (unsigned p = 0; p < kParts; ++p) {
            const float v = red[p][e];
            if (is_count) ct += __float_as_uint(v);
            else t += v;
        }
        red[0][e] = is_count ? __uint_as_float(ct) : t;
    }
    __syncthreads();
}
template <bool SC1 = false>
__device__ __forceinline__ void reduce_rows_1024(const float* __restrict__ partials, unsigned rows, int nv,
                                                 float (*red)[kPartial], bool count_is_float = false) {
    reduce_rows_1024<SC1>(partials, rows, nv, red, count_is_float, [] {});
}

// reduce_rows_1024 for a workgroup of BLOCK lanes (a multiple of 64): lane = (part, slot) with BLOCK / 32 parts, every part sums
// its contiguous range of rows in order, lanes 0..31 add the parts in order. Fixed order: bit-reproducible for a given BLOCK.
template <int BLOCK, bool SC1>
__device__ __forceinline__ void reduce_rows_block(const float* __restrict__ partials, unsigned rows, int nv, float (*red)[kPartial]) {
    constexpr unsigned kParts = BLOCK / 32;
    const unsigned e = threadIdx.x & 31, part = threadIdx.x >> 5;
    const unsigned per = (rows + kParts - 1) / kParts;
    const unsigned lo = part * per, hi = min(rows, lo + per);
    float s = 0.0f;
    unsigned c = 0;
    const bool is_count = ((int)e == nv);
#pragma unroll 4
    for (unsigned b = lo; b < hi; ++b) {
        const float v = load_row_word<SC1>(partials + (size_t)b * kPartial + e);
        if (is_count) c += __float_as_uint(v);
        else s += v;
    }
    red[part][e] = is_count ? __uint_as_float(c) : s;
    __syncthreads();
    if (threadIdx.x < 32) {
        float t = 0.0f;
        unsigned ct = 0;
#pragma unroll
        for (unsigned p = 0; p < kParts; ++p) {
            const float v = red[p][e];
            if (is_count) ct += __float_as_uint(v);
            else t += v;
        }
        red[0][e] = is_count ? __uint_as_float(ct) : t;
    }
    __syncthreads();
}

// totals (21 upper-triangle H, 6 b, error | error only) + count -> sp_linearized
__device__ __forceinline__ void unpack_totals(const float* tot, int nv, sp_linearized* out) {
    if (nv == kAcc - 1) {
        // (unrolled: one lane runs this between two steps of a device-resident loop, and a rolled loop is 21 dependent LDS round
        // trips — read a total, store it twice — where the unrolled form issues the 27 reads back to back)
        float v[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) v[k] = tot[k];
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int cc = a; cc < 6; ++cc) {
                out->H[a * 6 + cc] = v[k];
                out->H[cc * 6 + a] = v[k];
                ++k;
            }
#pragma unroll
        for (int a = 0; a < 6; ++a) out->b[a] = v[21 + a];
        out->error = tot[27];
    } else {
        out->error = tot[0];
    }
    const unsigned cnt = __float_as_uint(tot[nv]);
    out->inlier = cnt;
    out->inlier_lo = (float)(cnt & 4095u);
    out->inlier_hi = (float)(cnt >> 12);
    out->pad[0] = out->pad[1] = 0.0f;
}

// optimize_gauss_newton (registration.hpp:803-828) + solve_linear_system (:791-801) + is_converged (:407-410)
__host__ __device__ inline void gn_update_impl(sp_linearized* lin, float* T, float lambda, float crit_rot,
                                               float crit_trans, float* delta_out8, bool fold_inlier, LdltScratch& w) {
    if (fold_inlier) lin->inlier = (uint32_t)lin->inlier_hi * 4096u + (uint32_t)lin->inlier_lo;  // integer fold: exact
    float H[36], nb[6], delta[6];
#pragma unroll
    for (int i = 0; i < 36; ++i) H[i] = lin->H[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        H[i * 6 + i] = lin->H[i * 6 + i] + lambda * 1.0f;
        nb[i] = -lin->b[i];
    }
    const bool ok = ldlt6_solve(H, nb, delta, w);
    const float nr = sqrtf(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
    const float nt = sqrtf(delta[3] * delta[3] + delta[4] * delta[4] + delta[5] * delta[5]);
    const bool conv = ok && (nr < crit_rot) && (nt < crit_trans);
    const Rigid cur = load_rigid_colmajor(T);
    const Rigid upd = rigid_mul(cur, se3_exp(delta));
    store_rigid_colmajor(upd, T);
    if (delta_out8) {
        for (int i = 0; i < 6; ++i) delta_out8[i] = delta[i];
        delta_out8[6] = conv ? 1.0f : 0.0f;
        delta_out8[7] = ok ? 1.0f : 0.0f;
    }
}

__device__ __forceinline__ Sym3 load_sym(const float4* __restrict__ p) {
    const float4 a = p[0], b = p[1];
    return Sym3{a.x, a.y, a.z, a.w, b.x, b.y};
}

// The prepared source lies in WAVE TILES: 64 consecutive prepared points are one contiguous block of kSrcTileWords floats
// (2304 bytes), sub-plane k (x y z | xx xy xz yy yz zz) at word 64 k of the block, the point's lane l = i % 64 at word l of the
// sub-plane. A point has ONE address, base + (i / 64) * 2304 + (i % 64) * 4 bytes; its nine words are nine loads of that
// address at the immediate offsets 0, 256, ..., 2048, each still one coalesced 256-byte request of a wave, all in one run of
// memory. Whole tiles are allocated (src_tile_words); the unused lanes of the last one are never read. POINT_TO_DISTRIBUTION
// has no source covariance: the same tile, its six covariance sub-planes neither written nor read.
constexpr unsigned kSrcPlanes = 9;
constexpr unsigned kSrcTileWords = kSrcPlanes * kWave;
__host__ __device__ inline size_t src_tile_words(size_t n) { return (n + kWave - 1) / kWave * kSrcTileWords; }

struct FusedParams {
    const float* src;      // prepared source in wave tiles (src_words)
    const float4* tpts;    // grid-ordered target points
    const unsigned* tstart;
    const float4* tcovp;   // grid-ordered prepared target covariances
    const float4* tnb;     // grid order: second certificate of the reuse test (certificate_kernel), may be null
    GridDesc g;
    unsigned n;
    float max_d2, scale;
    QueryPose pose;
    const unsigned* perm;  // prepared-source order -> original source index (for the optional neighbour outputs)
    float4* ccache;        // per prepared source point: its previous correspondence (point, covariance row), 3 x float4; never null
    int cache_valid;       // 0: first linearisation after sp_gicp_source_prepare, the cache holds nothing yet
    int32_t* nn_idx;
    float* nn_d2;
};

// The nine words of prepared source point i: the one address, then the words at fixed offsets from it.
__device__ __forceinline__ const float* src_words(const FusedParams& P, unsigned i) {
    return P.src + ((size_t)(i / kWave) * kSrcTileWords + (i % kWave));
}
__device__ __forceinline__ float4 src_point(const float* __restrict__ w) {
    return make_float4(w[0], w[kWave], w[2 * kWave], 1.0f);
}
__device__ __forceinline__ Sym3 src_cov(const float* __restrict__ w) {
    return Sym3{w[3 * kWave], w[4 * kWave], w[5 * kWave], w[6 * kWave], w[7 * kWave], w[8 * kWave]};
}

// Linearisation of one correspondence (source point s with q = T s, winner nn, packed covariances) and accumulation. The
// algebra is linearize_terms (sp_linearize.h: one body for GICP / P2D / ERR_ONLY and every loss).
// ERR_ONLY: only the robust error and the count, into acc[0] — the K12 of a trial pose (sp_gicp_error_prepared).
template <int LOSS, bool P2D = false, bool ERR_ONLY = false, int NACC = kAcc - 1>
__device__ __forceinline__ void fused_math(const FusedParams& P, const Rigid& T, const float4 s, float qx, float qy,
                                           float qz, const Nearest& nn, const Sym3& Cs, const Sym3& Ct,
                                           float (&acc)[NACC], unsigned& cnt) {
    float t[NACC];
    linearize_terms<LOSS, P2D, ERR_ONLY>(T, s.x, s.y, s.z, qx, qy, qz, nn.x, nn.y, nn.z, Cs, Ct, P.scale, t);
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] += t[e];
    ++cnt;
}

// The cached correspondence of a source point: 3 x float4 in SOURCE order (sp_gicp_source::ccache)
//   row[0] = (t.x, t.y, t.z, rho_t^2)                  what the reuse certificate needs comes first
//   row[1] = (xx, xy, xz, yy)                          prepared covariance row of t ...
//   row[2] = (yz, zz, index bits, grid position bits)  ... index -1 (and rho^2 = 0): nothing found, searched again next time
// Written by whoever searched for the point (fused_point inline, or gicp_search_kernel); the winner's prepared row is
// gathered here, next to the points the search has just scanned.
// NOTHING FOUND below the search bound (idx = -1): the row records WHERE the search was made, q, and the margin m by which its
// bound exceeded max_correspondence_distance B (search_margin2: squared, shrunk against rounding; 0 when there was none). No
// target lies within B + m of q, so while the point stays within m of q no target lies within B of it: the same "no
// correspondence" a fresh search would return, proven by the first test of the certificate (|q' - q|^2 < m^2) with no search —
// a source point outside the overlap is searched once, not in every iteration, and it is the dearest search there is (the
// whole ball of the bound).
__device__ __forceinline__ void store_correspondence(float4* __restrict__ row, const FusedParams& P, const Nearest& nn,
                                                     Sym3& Ct, float qx = 0.0f, float qy = 0.0f, float qz = 0.0f,
                                                     float margin2 = 0.0f) {
    float4 r0 = make_float4(qx, qy, qz, margin2), r1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f),
           r2 = make_float4(0.0f, 0.0f, __int_as_float(-1), 0.0f);
    if (nn.idx >= 0) {
        const float4 c0 = P.tcovp[2 * (size_t)nn.pos], c1 = P.tcovp[2 * (size_t)nn.pos + 1];
        r0 = make_float4(nn.x, nn.y, nn.z, c1.z);
        r1 = c0;
        r2 = make_float4(c1.x, c1.y, __int_as_float(nn.idx), __uint_as_float(nn.pos));
        Ct = Sym3{c0.x, c0.y, c0.z, c0.w, c1.x, c1.y};
    }
    row[0] = r0;
    row[1] = r1;
    row[2] = r2;
}

// Reuse certificate. Correspondences rarely change from one iteration to the next. The previous winner t is PROVABLY still
// the nearest neighbour — same index, same distance as a fresh search — when |q - t| < rho_t, half the distance from t to
// its nearest other target point: any other target u then has |q - u| >= |t - u| - |q - t| > 2 rho_t - rho_t > |q - t|.
// Second chance (t has a close neighbour u1, so rho_t is tiny — such points would be searched in EVERY iteration): t is
// also certified when |q - t| < |q - u1| and |q - t| < d(t, u2) / 2, u2 being t's second-nearest other point — every target
// u other than t and u1 then has |q - u| >= |t - u| - |q - t| >= d(t, u2) - |q - t| > |q - t|. One 16-byte gather.
// (rho^2 carries a 1e-3 margin against rounding, certificate_kernel.)
__device__ __forceinline__ bool certified(const FusedParams& P, float d, float rho2, float qx, float qy, float qz,
                                          unsigned pos) {
    if (d < rho2) return true;
    if (!P.tnb || !(rho2 > 0.0f)) return false;
    const float4 nb = P.tnb[pos];
    return d < nb.w && d < dist2(qx, qy, qz, nb.x, nb.y, nb.z);
}

// The search of one query as the prepared paths run it. Nobody reads the neighbours when there is no nn_idx output: a
// correspondence beyond max_correspondence_distance is rejected whatever it is, so the search need not find it. The next
// float above max_d2 keeps a neighbour at exactly that distance.
__device__ __forceinline__ float search_bound2(const FusedParams& P) {
    return (P.nn_idx == nullptr && P.max_d2 < FLT_MAX) ? __uint_as_float(__float_as_uint(P.max_d2) + 1u) : FLT_MAX;
}
// The same bound widened by a margin of a quarter of max_correspondence_distance, for the searches whose failure is recorded in
// the correspondence cache (store_correspondence): margin2 = what the row's certificate may use (squared, 2 % short of the
// margin: the bound's ball and the point's motion are compared in float arithmetic).
__device__ __forceinline__ float search_bound2_margin(const FusedParams& P, float& margin2) {
    margin2 = 0.0f;
    if (P.nn_idx != nullptr || !(P.max_d2 < FLT_MAX) || P.ccache == nullptr) return search_bound2(P);
    const float B = sqrtf(P.max_d2), m = 0.25f * B;
    const float wide = (B + m) * (B + m);
    if (!(wide < FLT_MAX)) return search_bound2(P);
    margin2 = (0.98f * m) * (0.98f * m);
    return wide;
}

// What a lane loads first of point i, whatever the pose: its three coordinate words and, when the cache is valid, its
// correspondence row — 15 words whose addresses depend on i alone. gicp_align_kernel requests them for the workgroup's first
// trip while the previous iteration is still being finished (align_prologue) and hands them to fused_point.
struct PointHead {
    float x, y, z;
    float4 r0, r1, r2;
};
// The six loads stand on EVERY path, with no branch around them: a load that is issued on one path only counts as pending on
// all of them, and the compiler then drains every load (s_waitcnt vmcnt(0)) where it could have counted the older ones in.
// So a lane without a point (i >= n) asks for point n - 1 again, and while the cache holds nothing every lane asks for row 0:
// addresses inside the n points and the n rows of this source (a source of no points still owns one tile and one row,
// sp_gicp_source_create), values nobody reads.
__device__ __forceinline__ void point_head_load(const FusedParams& P, unsigned i, PointHead& h) {
    const unsigned ic = min(i, max(P.n, 1u) - 1u);
    const float* const sw = src_words(P, ic);
    h.x = sw[0]; h.y = sw[kWave]; h.z = sw[2 * kWave];
    const float4* const row = P.ccache + 3 * (size_t)(P.cache_valid ? ic : 0u);
    h.r0 = row[0]; h.r1 = row[1]; h.r2 = row[2];
}

// One source point of the fused iteration: q = T p -> correspondence (cache row by certificate, else exact NN on the target
// grid) -> linearise -> accumulate.
// P.cache_valid: 0 the cache holds nothing (every point is searched), 1 a row is used when its certificate holds: while
// correspondences hold, an iteration is a pure coalesced stream of 84 bytes per point (12 p + 24 Cs' of its wave tile + 48
// cache row) with no search and no gather, and a wave whose lanes all pass never enters the search code.
// SEED: a point whose certificate fails starts its search from the previous winner (grid_nn1_fast's `seed`).
// NEG: a search that finds nothing is made with the widened bound and recorded as a negative certificate (store_correspondence).
// PRE (gicp_align_kernel): `head` holds the point's first loads already (point_head_load, issued behind the prologue's row
// loads) and `use_head`, uniform over the workgroup, says whether this trip takes them — the workgroup's first trip — or
// loads as every other caller does. From the certificate on, one text for both.
template <int LOSS, bool FAST_NN, bool P2D = false, bool SEED = true, bool NEG = true, bool PRE = false>
__device__ __forceinline__ void fused_point(const FusedParams& P, const Rigid& T, unsigned i, float (&acc)[kAcc - 1],
                                            unsigned& cnt, unsigned& searched, const PointHead* head = nullptr,
                                            bool use_head = false) {
    const float* const sw = src_words(P, i);
    float4* const row = P.ccache + 3 * (size_t)i;  // (a prepared source always has its cache rows)
    float4 s;
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;  // (read only where P.cache_valid has filled them)
    if constexpr (PRE) {
        if (use_head) {  // (a scalar branch)
            s = make_float4(head->x, head->y, head->z, 1.0f);
            r0 = head->r0; r1 = head->r1; r2 = head->r2;
        } else {
            s = src_point(sw);
            if (P.cache_valid) { r0 = row[0]; r1 = row[1]; r2 = row[2]; }
        }
    } else {
        s = src_point(sw);
    }
    float qx, qy, qz;
    transform_point(T, s.x, s.y, s.z, qx, qy, qz);
    Nearest nn;
    Sym3 Ct{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool hit = false;
    bool seeded = false;
    Nearest seed;
    seed.d2 = FLT_MAX; seed.idx = -1; seed.pos = 0; seed.x = seed.y = seed.z = 0.0f;
    if (P.cache_valid) {
        if constexpr (!PRE) { r0 = row[0]; r1 = row[1]; r2 = row[2]; }
        const float d = dist2(qx, qy, qz, r0.x, r0.y, r0.z);
        const unsigned pos = __float_as_uint(r2.w);
        if (certified(P, d, r0.w, qx, qy, qz, pos)) {
            hit = true;
            nn.idx = __float_as_int(r2.z); nn.pos = pos; nn.x = r0.x; nn.y = r0.y; nn.z = r0.z;
            nn.d2 = nn.idx >= 0 ? d : FLT_MAX;
            Ct = Sym3{r1.x, r1.y, r1.z, r1.w, r2.x, r2.y};
        } else if (SEED && __float_as_int(r2.z) >= 0) {  // the previous winner: a real point, an upper bound
            seed.d2 = d; seed.idx = __float_as_int(r2.z); seed.pos = pos; seed.x = r0.x; seed.y = r0.y; seed.z = r0.z;
            seeded = true;
        }
    }
    if (!hit) {
        ++searched;
        float margin2 = 0.0f;
        const float bound2 = NEG ? search_bound2_margin(P, margin2) : search_bound2(P);
        seeded = seeded && seed.d2 < bound2;
        if (!seeded) { seed.d2 = bound2; seed.idx = -1; seed.pos = 0; seed.x = seed.y = seed.z = 0.0f; }
        if (FAST_NN) {
            nn = grid_nn1_auto(P.tpts, P.tstart, P.g, qx, qy, qz, bound2, &seed);
        } else {
            nn = grid_nn1(P.tpts, P.tstart, P.g, qx, qy, qz, &seed, 0);
        }
        if (NEG) store_correspondence(row, P, nn, Ct, qx, qy, qz, margin2);
        else store_correspondence(row, P, nn, Ct);
    }
    if (P.nn_idx) {
        const unsigned o = P.perm[i];
        P.nn_idx[o] = nn.idx;
        P.nn_d2[o] = nn.d2;
    }
    if (nn.idx < 0 || nn.d2 > P.max_d2) return;
    // What the arithmetic reads of the source is requested HERE, the coordinates a second time with the covariance (one trip,
    // the same tile that the loop's head has just brought in), from an address formed again from i: neither the three
    // coordinates nor the address then occupy registers across the search, which at the kernels' 128-register budget is the
    // difference between no spill and up to three in the GICP instantiations. (The empty asm only keeps the compiler from
    // merging this address, and with it these loads, with the ones at the head.)
    unsigned i_again = i;
    asm volatile("" : "+v"(i_again));
    const float* const sw_again = src_words(P, i_again);
    const Sym3 Cs = P2D ? Sym3{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f} : src_cov(sw_again);
    fused_math<LOSS, P2D>(P, T, src_point(sw_again), qx, qy, qz, nn, Cs, Ct, acc, cnt);
}

// fused_point with the wave working together where a lane alone would hold it up: EVERY lane of the wave calls this
// (`valid`: the lane has a point), the first two search stages run per lane as in fused_point, and the queries still open
// after them (nothing proven inside the 4x4x4 block: points outside the overlap, holes, the rim) are finished one at a time
// by all 64 lanes (grid_nn1_ball_wave). Same correspondences, same sums per point as fused_point.
#ifdef SP_OPT_TIMING
__device__ unsigned long long g_sp_dbg[24 * 16];
__device__ unsigned g_sp_step;
__device__ unsigned long long g_sp_wg[24 * 8];
#define SP_PSTAMP(k) if (blockIdx.x == 0 && threadIdx.x == 0 && g_sp_step < 24) g_sp_dbg[g_sp_step * 16 + (k)] = wall_clock64()
#else
#define SP_PSTAMP(k)
#endif
template <int LOSS, bool P2D = false>
__device__ __forceinline__ void fused_point_wave(const FusedParams& P, const Rigid& T, unsigned i, bool valid,
                                                 float (&acc)[kAcc - 1], unsigned& cnt, unsigned& searched) {
    const unsigned ii = valid ? i : 0u;
    SP_PSTAMP(0);
    const float* const sw = src_words(P, ii);
    const float4 s = src_point(sw);
    float qx, qy, qz;
    transform_point(T, s.x, s.y, s.z, qx, qy, qz);
    Nearest nn;
    nn.d2 = FLT_MAX; nn.idx = -1; nn.pos = 0; nn.x = nn.y = nn.z = 0.0f;
    Sym3 Ct{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool hit = false;
    float4* const row = P.ccache + 3 * (size_t)ii;
    Nearest seed;
    seed.d2 = FLT_MAX; seed.idx = -1; seed.pos = 0; seed.x = seed.y = seed.z = 0.0f;
    if (valid && P.cache_valid) {
        const float4 r0 = row[0], r1 = row[1], r2 = row[2];
        const float d = dist2(qx, qy, qz, r0.x, r0.y, r0.z);
        const unsigned pos = __float_as_uint(r2.w);
        if (certified(P, d, r0.w, qx, qy, qz, pos)) {
            hit = true;
            nn.idx = __float_as_int(r2.z); nn.pos = pos; nn.x = r0.x; nn.y = r0.y; nn.z = r0.z;
            nn.d2 = nn.idx >= 0 ? d : FLT_MAX;
            Ct = Sym3{r1.x, r1.y, r1.z, r1.w, r2.x, r2.y};
        } else if (__float_as_int(r2.z) >= 0) {  // the previous winner: a real point, an upper bound (grid_nn1_fast's seed)
            seed.d2 = d; seed.idx = __float_as_int(r2.z); seed.pos = pos; seed.x = r0.x; seed.y = r0.y; seed.z = r0.z;
        }
    }
    const bool search = valid && !hit;
    SP_PSTAMP(1);
    float margin2 = 0.0f;
    const float bound2 = search_bound2_margin(P, margin2);
    bool open = false;
    bool fast_ok = true;
    // (a point with a previous winner starts from it, grid_nn1_fast's seed. Sending it straight to the ball scan of that
    // distance instead of through the block stages was measured on the reference's example: slower, 462 against 397 us per
    // alignment — the ball scan's batches of four dependent loads cost more than the first block's batches of eight.)
    const bool seeded = search && seed.d2 < bound2;
    if (search) {
        ++searched;
        if (!seeded) { seed.d2 = bound2; seed.idx = -1; seed.pos = 0; seed.x = seed.y = seed.z = 0.0f; }
        fast_ok = grid_nn1_fast(P.tpts, P.tstart, P.g, qx, qy, qz, nn, bound2, &seed);
    }
    SP_PSTAMP(2);
    if (search && !fast_ok) open = !grid_nn1_block4(P.tpts, P.tstart, P.g, qx, qy, qz, nn);
    SP_PSTAMP(3);
#ifdef SP_OPT_TIMING
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const unsigned long long a = __ballot(search), b = __ballot(search && !fast_ok), c = __ballot(open);
        const unsigned long long sd = __ballot(seeded);
        if (threadIdx.x == 0 && g_sp_step < 24) {
            unsigned long long* const d = g_sp_dbg + g_sp_step * 16;
            d[8] = __popcll(a); d[9] = __popcll(b); d[10] = __popcll(c); d[11] = __popcll(sd);
        }
    }
#endif
    if (__ballot(open)) {  // (uniform)
        if (open && !(nn.d2 < FLT_MAX)) {  // no bound at all (the caller wants the neighbour whatever its distance): the lane's own walk
            const Nearest seed = nn;
            nn = grid_nn1(P.tpts, P.tstart, P.g, qx, qy, qz, &seed, 2);
            open = false;
        }
        grid_nn1_ball_wave(P.tpts, P.tstart, P.g, open, qx, qy, qz, nn);
    }
    SP_PSTAMP(4);
    if (search) store_correspondence(row, P, nn, Ct, qx, qy, qz, margin2);
    SP_PSTAMP(5);
    if (valid && P.nn_idx) {
        const unsigned o = P.perm[ii];
        P.nn_idx[o] = nn.idx;
        P.nn_d2[o] = nn.d2;
    }
    if (!valid || nn.idx < 0 || nn.d2 > P.max_d2) return;
    const Sym3 Cs = P2D ? Sym3{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f} : src_cov(sw);
    fused_math<LOSS, P2D>(P, T, s, qx, qy, qz, nn, Cs, Ct, acc, cnt);
    SP_PSTAMP(6);
}

// One source point, the WHOLE WAVE (every lane calls it with the same i; what it returns in acc / cnt / searched is the same on
// every lane: the caller keeps one lane's). For sources of a few thousand points — the reference pipeline aligns a random sample
// of 1000 — there are more SIMDs than queries, and what a linearisation costs is the longest chain of dependent loads any one
// lane runs into. Here a query is: cache row + certificates, else ONE ball scan by all 64 lanes (grid_nn1_query_wave) of
//   the previous winner's distance (a seed: a real point, so the scan is exact and its ball a fraction of a cell), or
//   half a cell when there is no previous winner (anything found inside is the nearest neighbour), then the search bound's ball,
// the winner's prepared row, the arithmetic of fused_point (same correspondences, same per-point terms).
//
// MARGIN CERTIFICATE (qcert, optional: a float4 per source point beside its cache row). The rho certificate asks how near the
// query is to its winner against the spacing of the TARGET; on a real scan — returns millimetres apart, the two clouds
// centimetres — it never holds, and every iteration searched every point although the pose had stopped moving. The scan knows
// more: d1, the winner's distance, and a lower bound d2 of every other target's (the runner-up it met, or its own radius).
// With the query at q_s then and at q' now: |q' - u| >= d2 - |q' - q_s| for every other target u and |q' - t| <= d1 + |q' - q_s|,
// so while the point has moved less than (d2 - d1) / 2 since it was searched, t is still the strict nearest neighbour — the
// winner a fresh search would return, at the distance computed here. qcert = (q_s, margin^2), the margin shrunk against
// rounding; a seeded scan reaches a little past its seed (twice the point's last move) so that there is a runner-up to measure.
//
// rows_out / qc_out (optional): the rows this linearisation LEAVES — another set than the one it reads when the step is
// speculative (registration_opt.hip: an LM / dog-leg trial and the linearisation at its pose in one step; the rows read stay
// what the trial's frozen correspondences are). Every point's rows are then written: found anew, or copied when a certificate held.
template <int LOSS, bool P2D = false>
__device__ __forceinline__ void fused_query_wave(const FusedParams& P, const Rigid& T, unsigned i, float (&acc)[kAcc - 1],
                                                 unsigned& cnt, unsigned& searched, float4* rows_out = nullptr,
                                                 const float4* qc_in = nullptr, float4* qc_out = nullptr) {
    SP_PSTAMP(0);
    const float* const sw = src_words(P, i);
    const float4 s = src_point(sw);
    float qx, qy, qz;
    transform_point(T, s.x, s.y, s.z, qx, qy, qz);
    Nearest nn;
    nn.d2 = FLT_MAX; nn.idx = -1; nn.pos = 0; nn.x = nn.y = nn.z = 0.0f;
    Sym3 Ct{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool hit = false, seeded = false;
    float moved2 = 0.0f;  // how far the point is from where it was last searched (squared)
    float4* const row = P.ccache + 3 * (size_t)i;
    float4* const row_out = rows_out ? rows_out + 3 * (size_t)i : row;
    if (qc_in != nullptr && qc_out == nullptr) qc_out = const_cast<float4*>(qc_in);
    if (P.cache_valid) {
        const float4 r0 = row[0], r1 = row[1], r2 = row[2];
        const float4 qc = qc_in ? qc_in[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float d = dist2(qx, qy, qz, r0.x, r0.y, r0.z);
        const unsigned pos = __float_as_uint(r2.w);
        const bool real = __float_as_int(r2.z) >= 0;
        if (qc_in) moved2 = dist2(qx, qy, qz, qc.x, qc.y, qc.z);
        if (certified(P, d, r0.w, qx, qy, qz, pos) || (qc_in && real && moved2 < qc.w)) {
            hit = true;
            nn.idx = __float_as_int(r2.z); nn.pos = pos; nn.x = r0.x; nn.y = r0.y; nn.z = r0.z;
            nn.d2 = nn.idx >= 0 ? d : FLT_MAX;
            Ct = Sym3{r1.x, r1.y, r1.z, r1.w, r2.x, r2.y};
            if (row_out != row) { row_out[0] = r0; row_out[1] = r1; row_out[2] = r2; }
            if (qc_out && qc_out != qc_in) qc_out[i] = qc;
        } else if (real) {  // the previous winner: a real point, an upper bound
            nn.d2 = d; nn.idx = __float_as_int(r2.z); nn.pos = pos; nn.x = r0.x; nn.y = r0.y; nn.z = r0.z;
            seeded = true;
        }
    }
    SP_PSTAMP(1);
    if (!hit) {  // (uniform)
        ++searched;
        float margin2 = 0.0f;
        const float bound2 = search_bound2_margin(P, margin2);
        float second2 = 0.0f, d1 = 0.0f;
        if (seeded && nn.d2 < bound2) {
            // (a little past the seed — twice the point's last move, a quarter of a cell at most: room for a runner-up that tells
            // how far the point may move before its winner can change)
            const float pad = qc_in ? fminf(2.0f * sqrtf(moved2), 0.25f * P.g.h) : 0.0f;
            const float reach = sqrtf(nn.d2) + pad;
            grid_nn1_query_wave(P.tpts, P.tstart, P.g, qx, qy, qz, fminf(reach * reach, bound2), nn, second2);
        } else {
            const float half = 0.5f * P.g.h;
            const float first2 = fminf(half * half, bound2);
            nn.d2 = first2; nn.idx = -1; nn.pos = 0; nn.x = nn.y = nn.z = 0.0f;
            grid_nn1_query_wave(P.tpts, P.tstart, P.g, qx, qy, qz, first2, nn, second2);
            if (nn.idx < 0 && first2 < bound2) {
                nn.d2 = bound2;
                grid_nn1_query_wave(P.tpts, P.tstart, P.g, qx, qy, qz, bound2, nn, second2);
            }
        }
        d1 = nn.d2;
        if (nn.idx < 0) nn.d2 = FLT_MAX;
        SP_PSTAMP(2); SP_PSTAMP(3); SP_PSTAMP(4);
        store_correspondence(row_out, P, nn, Ct, qx, qy, qz, margin2);  // (64 lanes, one address each, the same bits)
        if (qc_out) {
            // margin = (d2 - d1) / 2, 5 % short and less the rounding of the three distances involved (a difference of coordinates
            // of size s is off by an ulp of s, 6e-8 s: 2e-6 s covers them several times); never more than a cell (a second
            // target may simply not exist)
            float m = 0.0f;
            if (nn.idx >= 0) {
                const float scale = fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fmaxf(fabsf(qz), 1.0f));
                m = 0.475f * (sqrtf(second2) - sqrtf(d1)) - 2.0e-6f * scale;
                m = fminf(fmaxf(m, 0.0f), P.g.h);
            }
            qc_out[i] = make_float4(qx, qy, qz, m * m);
        }
        SP_PSTAMP(5);
    }
    if (nn.idx < 0 || nn.d2 > P.max_d2) return;
    const Sym3 Cs = P2D ? Sym3{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f} : src_cov(sw);
    fused_math<LOSS, P2D>(P, T, s, qx, qy, qz, nn, Cs, Ct, acc, cnt);
    SP_PSTAMP(6);
}

// One source point of the K12 on the prepared path (Registration::compute_error_parallel_reduction, registration.hpp:678-777, as
// the LM and dog-leg trial steps call it, :854, :933): the error at the TRIAL pose T with the correspondence FROZEN at that
// of the last linearisation (pose TL) — read from the point's cache row, not from neighbour arrays. The inlier gate uses the
// distance at TL (nn_d2 in the reference), recomputed with the search's own arithmetic, i.e. the same bits.
template <int LOSS, bool P2D>
__device__ __forceinline__ void error_prepared_point(const FusedParams& P, const Rigid& T, const Rigid& TL, unsigned i,
                                                     float (&acc)[1], unsigned& cnt) {
    const float* const sw = src_words(P, i);
    const float4 s = src_point(sw);
    const float4* const row = P.ccache + 3 * (size_t)i;
    const float4 tp = row[0], c0 = row[1], c1 = row[2];
    if (__float_as_int(c1.z) < 0) return;  // no neighbour found
    float lx, ly, lz;
    transform_point(TL, s.x, s.y, s.z, lx, ly, lz);
    if (dist2(lx, ly, lz, tp.x, tp.y, tp.z) > P.max_d2) return;  // registration.hpp:716-718
    float qx, qy, qz;
    transform_point(T, s.x, s.y, s.z, qx, qy, qz);
    Nearest nn;
    nn.x = tp.x; nn.y = tp.y; nn.z = tp.z; nn.idx = __float_as_int(c1.z); nn.pos = 0; nn.d2 = 0.0f;
    Sym3 Cs{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (!P2D) Cs = src_cov(sw);
    const Sym3 Ct{c0.x, c0.y, c0.z, c0.w, c1.x, c1.y};
    fused_math<LOSS, P2D, true, 1>(P, T, s, qx, qy, qz, nn, Cs, Ct, acc, cnt);
}

// block_reduce_store for a launch of ONE workgroup: the totals go straight to tot[0 .. NV + 1] in LDS (NV sums, the uint32
// count, the second integer as a float value) instead of a partial row in memory that the same workgroup would read back.
// Ends with a barrier.
template <int NV, int BLOCK>
__device__ __forceinline__ void block_reduce_lds(float (&acc)[NV], unsigned cnt, unsigned extra, float* __restrict__ tot) {
    __shared__ float red[BLOCK / kWave][kPartial];
    const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    wave_sums_to_row<NV>(acc, cnt, extra, lane, red[wave]);
    __syncthreads();
    if (threadIdx.x < NV) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < BLOCK / kWave; ++w) s += red[w][threadIdx.x];
        tot[threadIdx.x] = s;
    } else if (threadIdx.x == NV || threadIdx.x == NV + 1) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / kWave; ++w) c += __float_as_uint(red[w][threadIdx.x]);
        tot[threadIdx.x] = threadIdx.x == NV ? __uint_as_float(c) : (float)c;
    }
    __syncthreads();
}

constexpr int kAlignBlock = 1024;      // 16 waves: one workgroup per CU at 4 waves/SIMD -> 256 partial rows
constexpr int kAlignMaxBlocks = 256;
constexpr int kSearchedLog = 64;       // launches of an alignment whose searched-point counts are kept
// Whether a point whose certificate failed starts its search from the previous winner (fused_point's SEED) in the per-iteration
// kernels of registration.hip. Off: at their 128-register budget it costs the benchmarked instantiation one spilled register.
#ifndef SP_SEED_SEARCHES
#define SP_SEED_SEARCHES 1
#endif
constexpr bool kSeedSearches = SP_SEED_SEARCHES != 0;
#ifndef SP_NEG_CERT
#define SP_NEG_CERT 0
#endif
constexpr bool kNegCert = SP_NEG_CERT != 0;  // negative certificates in the per-iteration kernels of registration.hip (fused_point's NEG)

// The pose of a launch into scalar registers (it is uniform; it would otherwise occupy 12 VGPRs for the whole loop).
__device__ __forceinline__ Rigid uniform_pose(const float* sT) {
    Rigid T = load_rigid_colmajor(sT);
    auto uniform = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T.R[r][c] = uniform(T.R[r][c]);
        T.t[r] = uniform(T.t[r]);
    }
    return T;
}
// XCD-aware tile order: workgroup b runs on XCD b % 8, so give every XCD one contiguous eighth of the
// (cell-ordered) source: the target cells it reads then stay in that XCD's own L2 from one grid row / layer to the next
__device__ __forceinline__ unsigned xcd_tile() {
    unsigned tile = blockIdx.x;
    if ((gridDim.x & 7u) == 0u) tile = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    return tile;
}

// The grid-wide hand-off between two steps of a persistent launch (gicp_align_persistent_kernel, and gicp_optimize_kernel where a
// lane has a point to itself): every workgroup stores a partial row, then every workgroup reads all of them. An arrival counter
// sharded over kTicketShards lines, zero when the launch starts and never reset in it, separates the two
// (MI355X_MICROARCH.md, hand-off table, first row; cdna_hip_programming.md Guideline 16, the counter form with sc1 loads in place
// of an acquire). Its conditions:
//   * every word of the row was stored write-through at agent scope (store_row_word<true>: global_store ... sc1) by lanes of
//     wave 0 of the workgroup,
//   * grid_arrive (every lane of the workgroup calls it): wave 0 drains those stores (s_waitcnt vmcnt(0)) and only then lane 0
//     adds 1 to the shard of its XCD — one lane signals for all its workgroup's stores; relaxed, agent scope,
//   * grid_wait (ONE lane calls it): polls the shards with relaxed agent-scope loads and s_sleep until they add up to `want`
//     (= grid * steps so far), bounded by `budget` wall_clock64 ticks — false when the bound ran out: a grid that is not fully
//     resident ends with its error word set by the caller, never hangs,
//   * after the poll has matched, the rows are read with sc1 loads only (load_row_word<true>, never a plain load of another
//     workgroup's bytes): the polling wave after its poll, the others behind a workgroup barrier it joins.
constexpr int kTicketShards = 8;
constexpr int kTicketStride = 32;  // uint32 words between two shards (128 bytes: a line each)
__device__ __forceinline__ void grid_arrive(unsigned* tickets) {
    if (threadIdx.x < kWave) {  // the storing lanes all sit in wave 0
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0)
            __hip_atomic_fetch_add(tickets + (blockIdx.x & (kTicketShards - 1)) * kTicketStride, 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ bool grid_wait(unsigned* tickets, unsigned want, unsigned long long budget) {
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        unsigned have = 0;
#pragma unroll
        for (int sh = 0; sh < kTicketShards; ++sh)
            have += __hip_atomic_load(tickets + sh * kTicketStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (have >= want) return true;
        if (wall_clock64() - t0 > budget) return false;
        __builtin_amdgcn_s_sleep(2);
    }
}

}  // namespace
}  // namespace sp

struct sp_gicp_target {
    const sp_grid* grid = nullptr;  // borrowed: must outlive this object
    float4* covp = nullptr;         // 2 x float4 per target point, grid order: (xx,xy,xz,yy | yz,zz,rho^2,0)
    float* rho2 = nullptr;          // per target point (original order): squared safe radius of the reuse test
    float4* nb = nullptr;           // per target point (grid order): second certificate (nearest neighbour, second radius)
    unsigned long long version = 0; // bumped by every sp_gicp_target_update (cached copies of rows become stale)
    int reg_type = SP_REG_GICP;     // what the rows hold: plane(Ct) for GICP, inverse(Ct) for POINT_TO_DISTRIBUTION
    size_t n = 0;
    mutable sp::StreamSet streams;  // streams the rows (and the borrowed grid) have been used on
    void note(hipStream_t st) const { streams.note(st); if (grid) sp::grid_use(grid, st); }
};
namespace sp {
// Tagged partial rows of the wave-per-point optimiser launch: 2 (step parity) x kAlignMaxBlocks rows x 32 granules of
// {float value, uint32 tag} (registration_opt.hip, tagged_rows_exchange).
constexpr size_t kOptRowsBytes = 2 * (size_t)256 * 32 * sizeof(unsigned long long);
}  // namespace sp
struct sp_gicp_source {
    size_t n_max = 0, n = 0;
    float* tiles = nullptr;   // the prepared points and covariances in wave tiles (src_tile_words(n_max) floats, see FusedParams)
    unsigned* perm = nullptr; // prepared position -> original index
    float4* ccache = nullptr;      // 3 x float4 per prepared point: its previous correspondence (see fused_point)
    float4* qcert = nullptr;       // margin certificates of the wave-per-point optimiser launch (fused_query_wave), qcert_points of them
    float4* qcert2 = nullptr;      // ... and of the other row set of fused steps (min(n_max, 2048) points)
    size_t qcert_points = 0;
    mutable bool qcert_valid = false;  // the margin certificates belong to the cache rows as they are (only a wave-per-point launch keeps them so)
    float4* ccache2 = nullptr;     // a second set of cache rows for sp_gicp_align_optimize's fused trial + linearisation steps (min(n_max, 2048) points)
    unsigned long long* opt_rows = nullptr;  // sp_gicp_align_optimize, wave-per-point launches: tagged partial rows (kOptRowsBytes)
    mutable unsigned opt_epoch = 0;          // ... and the epoch of the latest such launch (12 bits of every row tag)
    mutable bool cache_valid = false;  // set by the first linearisation after prepare
    const sp_gicp_target* cache_target = nullptr;  // the copies are of this target ...
    unsigned long long cache_version = 0;           // ... at this covariance version
    bool sorted = false;
    // measurement / tuning switches (sp_internal.h; not part of the C ABI), per prepared source:
    int opt_stage_mask = 3;  // bit 0 = per-iteration kernel, bit 1 = final reduce (+ solve) / finish kernel
    int opt_reuse = 2;       // 0 always search, 1 reuse on the first certificate, 2 also the second
    int opt_fast_nn = -1;    // -1: automatic (2x2x2 fast path when the source is cell-sorted), 0 / 1: forced
    int opt_persistent = 1;  // sp_gicp_align_fused: 1 the tail of an alignment as one launch when the grid is resident, 0 a launch per iteration
    int opt_persistent_from = 4;  // first iteration of that tail
    int opt_fuse_trials = 1; // sp_gicp_align_optimize, wave-per-point launches: LM / dog-leg trial steps also linearise at the trial pose (sp_internal.h)
    int opt_wave_query = 1;  // sp_gicp_align_optimize, small sources: one wave per point in the linearisation steps
    unsigned *keys_in = nullptr, *keys_out = nullptr, *vals_in = nullptr;
    void* sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
};

namespace sp {
namespace {
FusedParams make_fused_params(const sp_gicp_target* target, const sp_gicp_source* source, const sp_factor_params* params,
                              const float* transT, int transT_on_device, int32_t* nn_idx_out, float* nn_d2_out) {
    const size_t n = source->n;
    FusedParams P;
    P.src = source->tiles;
    P.tpts = target->grid->d_pts;
    P.tstart = target->grid->d_start;
    P.tcovp = target->covp;
    P.tnb = source->opt_reuse > 1 ? target->nb : nullptr;  // (null too when the target has no certificates)
    P.g = grid_desc(target->grid);
    P.n = (unsigned)n;
    P.max_d2 = params->max_correspondence_distance * params->max_correspondence_distance;
    P.scale = params->robust_scale;
    P.pose = query_pose(transT, transT_on_device);
    P.perm = source->perm;
    // the cache rows are always written (sp_gicp_error_prepared reads the frozen correspondences from them); the reuse
    // switch only decides whether a later linearisation may trust them instead of searching
    P.ccache = source->ccache;  // (a target without certificates still fills the rows: every linearisation then searches, seeded)
    P.cache_valid = (source->opt_reuse && source->cache_valid && source->cache_target == target &&
                     source->cache_version == target->version) ? 1 : 0;
    P.nn_idx = (nn_idx_out && nn_d2_out) ? nn_idx_out : nullptr;
    P.nn_d2 = nn_d2_out;
    return P;
}

// The prepared forms exist for RegType::GICP and POINT_TO_DISTRIBUTION; the target's rows must be of the factor asked for.
int check_prepared_reg(const sp_gicp_target* target, const sp_factor_params* params) {
    if (params->reg_type != SP_REG_GICP && params->reg_type != SP_REG_POINT_TO_DISTRIBUTION) {
        sp_set_error("[sp_gicp_*] only RegType::GICP and RegType::POINT_TO_DISTRIBUTION have a prepared/fused form");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (params->reg_type != target->reg_type) {
        sp_set_error("[sp_gicp_*] the prepared target holds the rows of another RegType: call sp_gicp_target_prepare");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (params->rotation_constraint_enable) {
        sp_set_error("[sp_gicp_*] the rotation constraint needs the raw covariances: use sp_gicp_linearize");
        return SP_ERR_INVALID_ARGUMENT;
    }
    return SP_OK;
}

int check_workspace(const void* workspace, size_t workspace_bytes, size_t n) {
    if (!workspace || workspace_bytes < sp_gicp_workspace_bytes(n)) {
        sp_set_error("[Registration] workspace too small (sp_gicp_workspace_bytes)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    return SP_OK;
}

unsigned align_grid(size_t n) {
    unsigned grid = div_up(n, kAlignBlock);
    return grid > (unsigned)kAlignMaxBlocks ? (unsigned)kAlignMaxBlocks : (grid ? grid : 1u);
}

// Which search a lane runs. Unsorted lanes touch unrelated cells: the ring walk (fewest cache lines per query) wins. Cell-sorted
// lanes share their lines: the branch-light 2x2x2 walk wins (profiles/README.md, r01_c).
bool source_fast_nn(const sp_gicp_source* source) {
    return source->opt_fast_nn < 0 ? source->sorted : (source->opt_fast_nn != 0);
}

// Run-time choices -> template arguments (Registration::dispatch, registration.hpp:372-405): f gets the choice as a
// std::integral_constant / std::bool_constant, instantiates its kernel with it, launches, and returns a status.
// SP_DEV_MIN (development builds only, scratch/devbuild.sh: one instantiation of every kernel, a fraction of the compile time)
// builds the first robust loss and, of a with_bool<DEV>, the DEV side only; everything else is an error at run time.
#ifdef SP_DEV_MIN
constexpr bool kDevMin = true;
#else
constexpr bool kDevMin = false;
#endif
inline int not_in_dev_build() {
    sp_set_error("SP_DEV_MIN build: only GICP / NONE / sorted source / one GPU");
    return SP_ERR_RUNTIME;
}
inline int unknown_combination() {  // (a RegType or robust loss outside the enums)
    sp_set_error("[Registration::dispatch] Combination not found in tags!");
    return SP_ERR_RUNTIME;
}
template <typename F>
int with_loss(int robust_type, F&& f) {
    if constexpr (kDevMin) {
        return robust_type == SP_LOSS_NONE ? f(std::integral_constant<int, LOSS_NONE>{}) : not_in_dev_build();
    } else {
        switch (robust_type) {
            case SP_LOSS_NONE: return f(std::integral_constant<int, LOSS_NONE>{});
            case SP_LOSS_HUBER: return f(std::integral_constant<int, LOSS_HUBER>{});
            case SP_LOSS_TUKEY: return f(std::integral_constant<int, LOSS_TUKEY>{});
            case SP_LOSS_CAUCHY: return f(std::integral_constant<int, LOSS_CAUCHY>{});
            case SP_LOSS_GEMAN_MCCLURE: return f(std::integral_constant<int, LOSS_GEMAN_MCCLURE>{});
        }
        return unknown_combination();
    }
}
template <bool DEV, typename F>
int with_bool(bool b, F&& f) {
    if constexpr (kDevMin) return b == DEV ? f(std::bool_constant<DEV>{}) : not_in_dev_build();
    else return b ? f(std::true_type{}) : f(std::false_type{});
}
// The three choices every prepared-path kernel has: f(loss, FAST_NN, P2D).
template <typename F>
int with_variant(int robust_type, bool fast, bool p2d, F&& f) {
    return with_loss(robust_type, [&](auto loss) {
        return with_bool<true>(fast, [&](auto fast_c) {
            return with_bool<false>(p2d, [&](auto p2d_c) { return f(loss, fast_c, p2d_c); });
        });
    });
}

}  // namespace
}  // namespace sp


#include <mutex>
namespace sp {
// One persistent launch (a kernel whose workgroups wait for each other: gicp_align_persistent_kernel, gicp_optimize_kernel) at a
// time per DEVICE of this process: two in flight on different streams would each hold CUs the other one is waiting for, and
// both would run into their time limit. persist_acquire() returns the device's guard LOCKED when such a launch may go onto
// `st` now — its grid fits the device's CUs, `st` is not capturing, and no other stream's persistent launch can still be
// running — or nullptr. The caller launches and calls persist_release(), which records the completion event and unlocks:
// check and launch are one critical section. (Other processes on the device and CU-masked streams are not seen by this guard:
// the kernels' waits are bounded and a wait that runs out is reported — sp_align_result::status, sp_gicp_align_status.)
struct PersistGuard {
    std::mutex m;
    hipStream_t last = nullptr;
    hipEvent_t done = nullptr;
    bool used = false;
    int cus = -1;
};
PersistGuard* persist_acquire(hipStream_t st, unsigned grid);
void persist_release(PersistGuard* g, hipStream_t st);
constexpr size_t kTicketOffsetBytes = 96 * 1024;  // in the workspace, behind everything align_ws() lays out (< 66 KB)
}  // namespace sp

#endif  // SP_REGISTRATION_DEVICE_H
