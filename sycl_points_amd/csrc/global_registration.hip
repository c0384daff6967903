// Global registration for gfx950 (MI355X extension): initial guesses for sp_gicp_align_batch from the data.
//   sp_fpfh_compute          FPFH descriptors of a cloud with oriented normals and a kNN result on itself (two launches)
//   sp_feature_match         nearest neighbour in descriptor space, the products on the f32 matrix cores
//   sp_feature_match_mutual  both directions, the mutual pairs compacted in ascending source index
//   sp_ransac_score          one lane per hypothesis: a pose from three matches, scored by the matches it explains
//   sp_ransac_select_host    the best hypotheses, their poses recomputed in double
// The definitions are include/sycl_points_amd.h's. No float atomic anywhere: every result is the same bits on every call.
//
// SPFH (spfh_kernel): a wave per point, a lane per neighbour (k <= 64). Every lane bins its pair; the 33 counts are taken by
// ballots (count[b] = popcount(ballot(bin == b)), a scalar, selected into lane b), so no lane indexes a histogram by a runtime
// value and nothing goes to scratch. The counts are integers: the order of summation does not exist. v = d x n_i is a difference
// of products evaluated with the fmaf remainder (Kahan), so that |v| small against |d| does not lose the direction of v.
// Bytes per point: 4 k (index row) + 32 k (gathered point and normal) + 32 (own) + 144 (row out).
//
// FPFH (fpfh_kernel): a wave per point, a lane per bin. Lane p holds list entry p; the loop over the list broadcasts (j, 1 / d2)
// from lane p and every lane adds one bin of SPFH_j: a 144-byte row per neighbour, one 4-byte read per lane. The group sums are
// taken by every lane in bin order (11 reads across the wave). Bytes per point: 8 k + 144 k (gathered rows) + 144.
//
// Match (match_kernel): |a|^2 + |b|^2 - 2 a.b. The norms are summed in double over the 33 bins and rounded once
// (norms_kernel). The products: v_mfma_f32_32x32x2_f32 with the TARGET rows as the A operand and the QUERY rows as the B
// operand, so D[target][query] has the query on the lane (lane & 31) and 16 targets in the lane's registers
// (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)): the running (minimum, index) of a query is one pair of registers per lane,
// updated in ascending target order with a strict <, and lanes l and l + 32 are combined once at the end. K: the 33 bins in 17
// steps; both operands use the same assignment of bins to (step, lane half) — steps 4 g .. 4 g + 3 take bins 8 g + 4 h .. + 3 (one
// 16-byte read), step 16 takes bin 32 in half 0 and a zero in half 1 — the pad floats are never read. A workgroup is 4 waves
// with 64 queries each (two B operands, 34 registers, loaded once) and walks its chunk of the targets in stages of 128 rows staged
// through LDS (row stride 36 floats = the rows as they lie in memory: conflict-free for 16-byte reads), the next stage fetched
// into registers while this one is multiplied. grid.y splits the targets so that a small query set still fills the device;
// chunks are combined by atomicMin on (bits of d2) << 32 | index, an integer minimum: order-independent, ties to the lowest index.
//
// Compiled with -ffp-contract=off: every fused multiply-add is an explicit fmaf; sqrt and division are correctly rounded.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sp_common.h"
#include "sp_math.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

constexpr unsigned kStride = SP_FPFH_STRIDE;  // floats per descriptor row
constexpr unsigned kBins = SP_FPFH_BINS;
constexpr size_t kMaxCloud = (size_t)1 << 31;

// ------------------------------------------------------------------------------------------------------------------ FPFH
// a * b - c * d with one rounding of the result's size (Kahan): w = c d rounded, e = its remainder, f = a b - w fused
__device__ __forceinline__ float diff_of_products(float a, float b, float c, float d) {
    const float w = c * d;
    const float e = fmaf(-c, d, w);
    const float f = fmaf(a, b, -w);
    return f + e;
}
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}
__device__ __forceinline__ int bin11(float scaled) {  // floor, clamped to 0..10
    const int b = (int)floorf(scaled);
    return b < 0 ? 0 : (b > 10 ? 10 : b);
}

__global__ __launch_bounds__(kBlock) void spfh_kernel(const float4* __restrict__ points, const float4* __restrict__ normals,
                                                      unsigned n, const int32_t* __restrict__ knn_idx, unsigned k,
                                                      float* __restrict__ spfh, uint16_t* __restrict__ counts_out,
                                                      uint16_t* __restrict__ m_out) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr unsigned kWaves = kBlock / kWave;
    for (unsigned i = blockIdx.x * kWaves + wave; i < n; i += gridDim.x * kWaves) {  // uniform across the wave
        const int j = lane < k ? knn_idx[(size_t)i * k + lane] : -1;
        const bool is_nb = j >= 0 && (unsigned)j < n && (unsigned)j != i;
        const unsigned m = (unsigned)__popcll(__ballot(is_nb));
        int b1 = -1, b2 = -1, b3 = -1;
        if (is_nb) {
            const float4 pi = points[i], ni = normals[i];
            const float4 pj = points[j], nj = normals[j];
            const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
            const float dist = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
            float vx = diff_of_products(dy, ni.z, dz, ni.y);  // v = d x n_i
            float vy = diff_of_products(dz, ni.x, dx, ni.z);
            float vz = diff_of_products(dx, ni.y, dy, ni.x);
            const float vn = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
            if (dist > 0.0f && vn > 0.0f) {  // (false for NaN too)
                const float f3 = dot3(ni.x, ni.y, ni.z, dx, dy, dz) / dist;
                vx /= vn, vy /= vn, vz /= vn;
                const float wx = diff_of_products(ni.y, vz, ni.z, vy);  // w = n_i x v
                const float wy = diff_of_products(ni.z, vx, ni.x, vz);
                const float wz = diff_of_products(ni.x, vy, ni.y, vx);
                const float f2 = dot3(vx, vy, vz, nj.x, nj.y, nj.z);
                const float f1 = sp_atan2f(dot3(wx, wy, wz, nj.x, nj.y, nj.z), dot3(ni.x, ni.y, ni.z, nj.x, nj.y, nj.z));
                if (isfinite(f1) && isfinite(f2) && isfinite(f3)) {
                    constexpr float kPi = 3.14159265358979323846f;
                    b1 = bin11(11.0f * (f1 + kPi) / (2.0f * kPi));
                    b2 = bin11(11.0f * (f2 + 1.0f) * 0.5f);
                    b3 = bin11(11.0f * (f3 + 1.0f) * 0.5f);
                }
            }
        }
        unsigned cnt = 0;
#pragma unroll
        for (int b = 0; b < 11; ++b) {
            const unsigned c1 = (unsigned)__popcll(__ballot(b1 == b));
            const unsigned c2 = (unsigned)__popcll(__ballot(b2 == b));
            const unsigned c3 = (unsigned)__popcll(__ballot(b3 == b));
            cnt = lane == (unsigned)b ? c1 : cnt;
            cnt = lane == (unsigned)(11 + b) ? c2 : cnt;
            cnt = lane == (unsigned)(22 + b) ? c3 : cnt;
        }
        const float scale = m ? 100.0f / (float)m : 0.0f;
        if (lane < kStride) spfh[(size_t)i * kStride + lane] = lane < kBins ? (float)cnt * scale : 0.0f;
        if (counts_out && lane < kBins) counts_out[(size_t)i * kBins + lane] = (uint16_t)cnt;
        if (m_out && lane == 0) m_out[i] = (uint16_t)m;
    }
}

__global__ __launch_bounds__(kBlock) void fpfh_kernel(const float* __restrict__ spfh, unsigned n, const int32_t* __restrict__ knn_idx,
                                                      const float* __restrict__ knn_d2, unsigned k, float* __restrict__ fpfh) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr unsigned kWaves = kBlock / kWave;
    const unsigned bin = lane < kBins ? lane : 0u;          // lanes 33 .. 63 ride along on bin 0
    const unsigned group = bin / 11u;
    for (unsigned i = blockIdx.x * kWaves + wave; i < n; i += gridDim.x * kWaves) {
        int j = lane < k ? knn_idx[(size_t)i * k + lane] : -1;
        const float d2 = lane < k ? knn_d2[(size_t)i * k + lane] : 0.0f;
        if (!(j >= 0 && (unsigned)j < n && (unsigned)j != i) || d2 == 0.0f) j = -1;
        const float w = j >= 0 ? 1.0f / d2 : 0.0f;
        float f = 0.0f;
        for (unsigned p = 0; p < k; ++p) {
            const int jp = __shfl(j, (int)p, 64);
            const float wp = __shfl(w, (int)p, 64);
            if (jp >= 0) f = fmaf(wp, spfh[(size_t)jp * kStride + bin], f);  // (jp is uniform)
        }
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t < 11; ++t) s += __shfl(f, (int)(group * 11u) + t, 64);
        const float out = s != 0.0f ? f * (100.0f / s) : 0.0f;
        if (lane < kStride) fpfh[(size_t)i * kStride + lane] = lane < kBins ? out : 0.0f;
    }
}

// ----------------------------------------------------------------------------------------------------------------- match
constexpr unsigned kQueriesPerWave = 64;                       // two B operands
constexpr unsigned kQueriesPerBlock = 4 * kQueriesPerWave;     // 256
constexpr unsigned kStageRows = 128;                           // target rows per LDS stage: four 32-row tiles
constexpr unsigned kStageVec = kStageRows * kStride / 4;       // float4s per stage: 1152
constexpr unsigned kStageLoads = (kStageVec + kBlock - 1) / kBlock;  // per lane: 5 (the last one half used)
constexpr unsigned kKSteps = 17;
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(kBlock) void norms_kernel(const float* __restrict__ rows, unsigned n, float* __restrict__ norms) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        double s = 0.0;
        for (unsigned b = 0; b < kBins; ++b) {
            const double v = (double)rows[(size_t)i * kStride + b];
            s += v * v;
        }
        norms[i] = (float)s;
    }
}

__global__ __launch_bounds__(kBlock) void fill_keys_kernel(unsigned long long* __restrict__ keys, unsigned n) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) keys[i] = ~0ull;
}

__global__ __launch_bounds__(kBlock) void unpack_keys_kernel(const unsigned long long* __restrict__ keys, unsigned n,
                                                             int32_t* __restrict__ idx_out, float* __restrict__ d2_out) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const unsigned long long key = keys[i];
        const bool none = key == ~0ull;
        idx_out[i] = none ? -1 : (int32_t)(unsigned)(key & 0xffffffffull);
        if (d2_out) d2_out[i] = none ? 3.402823466e+38f : __uint_as_float((unsigned)(key >> 32));
    }
}

// The operand of (row, lane half h): bins 8 g + 4 h .. + 3 for g = 0 .. 3, then bin 32 (h = 0) or zero (h = 1).
__device__ __forceinline__ void load_operand(const float* row, unsigned h, float (&x)[kKSteps]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(row + 8 * g + 4 * h);
        x[4 * g + 0] = v.x, x[4 * g + 1] = v.y, x[4 * g + 2] = v.z, x[4 * g + 3] = v.w;
    }
    const float last = row[32];
    x[16] = h ? 0.0f : last;
}

// queries: the rows the minimum is taken FOR (nq of them); targets: the rows it is taken OVER (nt), rows [chunk_rows * blockIdx.y,
// + chunk_rows) of them in this workgroup. chunk_rows is a multiple of kStageRows.
__global__ __launch_bounds__(kBlock) void match_kernel(const float* __restrict__ queries, const float* __restrict__ qnorms, unsigned nq,
                                                       const float* __restrict__ targets, const float* __restrict__ tnorms, unsigned nt,
                                                       unsigned chunk_rows, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) float s_rows[2][kStageRows * kStride];
    __shared__ __attribute__((aligned(16))) float s_norm[2][kStageRows];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, col = lane & 31u, h = lane >> 5;
    const unsigned t_begin = blockIdx.y * chunk_rows;
    const unsigned t_end = min(nt, t_begin + chunk_rows);
    if (t_begin >= t_end) return;  // (uniform)
    const unsigned n_stages = (t_end - t_begin + kStageRows - 1) / kStageRows;

    // this wave's queries, as two B operands
    float qb[2][kKSteps], qn[2];
    unsigned qrow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        qrow[t] = blockIdx.x * kQueriesPerBlock + wave * kQueriesPerWave + 32u * t + col;
        const unsigned r = min(qrow[t], nq - 1u);  // (a row past the end reads the last row; its result is not stored)
        load_operand(queries + (size_t)r * kStride, h, qb[t]);
        qn[t] = qnorms[r];
    }
    float best[2] = {INFINITY, INFINITY};
    int best_idx[2] = {-1, -1};

    float4 pre[kStageLoads];
    float pre_norm = 0.0f;
    auto fetch = [&](unsigned stage) {  // rows [r0, r0 + kStageRows) of the targets into registers; zeros / +inf past t_end
        const unsigned r0 = t_begin + stage * kStageRows;
        const unsigned rows_here = min(kStageRows, t_end - r0);
        const float4* src = reinterpret_cast<const float4*>(targets + (size_t)r0 * kStride);
#pragma unroll
        for (unsigned u = 0; u < kStageLoads; ++u) {
            const unsigned v = tid + u * kBlock;
            pre[u] = v < rows_here * (kStride / 4) ? src[v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        if (tid < kStageRows) pre_norm = tid < rows_here ? tnorms[r0 + tid] : INFINITY;
    };
    auto stash = [&](unsigned buf) {
#pragma unroll
        for (unsigned u = 0; u < kStageLoads; ++u) {
            const unsigned v = tid + u * kBlock;
            if (v < kStageVec) reinterpret_cast<float4*>(s_rows[buf])[v] = pre[u];
        }
        if (tid < kStageRows) s_norm[buf][tid] = pre_norm;
    };
    fetch(0);
    stash(0);
    __syncthreads();
    for (unsigned stage = 0; stage < n_stages; ++stage) {
        const unsigned buf = stage & 1u;
        if (stage + 1 < n_stages) fetch(stage + 1);
        const unsigned stage_row0 = t_begin + stage * kStageRows;
#pragma unroll 1
        for (unsigned tile = 0; tile < kStageRows / 32; ++tile) {
            if (stage_row0 + tile * 32 >= t_end) break;  // (uniform)
            float ta[kKSteps];
            load_operand(&s_rows[buf][(tile * 32 + col) * kStride], h, ta);
            float tn[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(&s_norm[buf][tile * 32 + 8 * q + 4 * h]);
                tn[4 * q + 0] = v.x, tn[4 * q + 1] = v.y, tn[4 * q + 2] = v.z, tn[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x16 acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (unsigned s = 0; s < kKSteps; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[s], qb[t][s], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) {  // ascending target row
                    float d = fmaf(-2.0f, acc[r], qn[t] + tn[r]);
                    d = d < 0.0f ? 0.0f : d;
                    const int row = (int)(stage_row0 + tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h);
                    const bool better = d < best[t];  // (false for NaN and for the +inf of a row past the end)
                    best[t] = better ? d : best[t];
                    best_idx[t] = better ? row : best_idx[t];
                }
            }
        }
        if (stage + 1 < n_stages) stash(buf ^ 1u);
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        unsigned long long key = best_idx[t] < 0 ? ~0ull
                                                 : ((unsigned long long)__float_as_uint(best[t]) << 32) | (unsigned)best_idx[t];
        const unsigned long long other = __shfl_xor(key, 32, 64);
        key = other < key ? other : key;
        if (h == 0 && qrow[t] < nq && key != ~0ull) atomicMin(&keys[qrow[t]], key);
    }
}

struct MatchPlan {
    unsigned chunk_rows, chunks;
    size_t keys_off, qn_off, tn_off, bytes;
};
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
MatchPlan match_plan(size_t nq, size_t nt) {
    MatchPlan p{};
    const size_t qblocks = (nq + kQueriesPerBlock - 1) / kQueriesPerBlock;
    const size_t stages = (nt + kStageRows - 1) / kStageRows;
    size_t chunks = qblocks ? (2 * (size_t)kNumCU + qblocks - 1) / qblocks : 1;  // two workgroups per CU when the queries are few
    chunks = std::max<size_t>(1, std::min(chunks, std::max<size_t>(stages, 1)));
    const size_t stages_per_chunk = (std::max<size_t>(stages, 1) + chunks - 1) / chunks;
    p.chunk_rows = (unsigned)(stages_per_chunk * kStageRows);
    p.chunks = (unsigned)((std::max<size_t>(stages, 1) + stages_per_chunk - 1) / stages_per_chunk);
    p.keys_off = 0;
    p.qn_off = align16(8 * nq);
    p.tn_off = p.qn_off + align16(4 * nq);
    p.bytes = p.tn_off + align16(4 * nt);
    return p;
}

int match_enqueue(const float* a, size_t na, const float* b, size_t nb, int32_t* idx_out, float* d2_out, void* workspace,
                  hipStream_t st) {
    const MatchPlan p = match_plan(na, nb);
    char* ws = static_cast<char*>(workspace);
    auto* keys = reinterpret_cast<unsigned long long*>(ws + p.keys_off);
    float* qn = reinterpret_cast<float*>(ws + p.qn_off);
    float* tn = reinterpret_cast<float*>(ws + p.tn_off);
    fill_keys_kernel<<<stream_grid(na), kBlock, 0, st>>>(keys, (unsigned)na);
    if (nb) {
        norms_kernel<<<stream_grid(na), kBlock, 0, st>>>(a, (unsigned)na, qn);
        norms_kernel<<<stream_grid(nb), kBlock, 0, st>>>(b, (unsigned)nb, tn);
        const dim3 grid(div_up(na, kQueriesPerBlock), p.chunks);
        match_kernel<<<grid, kBlock, 0, st>>>(a, qn, (unsigned)na, b, tn, (unsigned)nb, p.chunk_rows, keys);
    }
    unpack_keys_kernel<<<stream_grid(na), kBlock, 0, st>>>(keys, (unsigned)na, idx_out, d2_out);
    return launch_status();
}

// pairs[i] = (i, s2t[i]); flags[i] = 1 when t2s[s2t[i]] == i
__global__ __launch_bounds__(kBlock) void mutual_flags_kernel(const int32_t* __restrict__ s2t, const int32_t* __restrict__ t2s,
                                                              unsigned ns, unsigned nt, int2* __restrict__ pairs,
                                                              uint8_t* __restrict__ flags) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < ns; i += gridDim.x * kBlock) {
        const int j = s2t[i];
        const bool ok = j >= 0 && (unsigned)j < nt && t2s[j] == (int)i;
        pairs[i] = make_int2((int)i, j);
        flags[i] = ok ? 1 : 0;
    }
}

struct MutualPlan {
    size_t match_off, s2t_off, t2s_off, pairs_off, pairs_out_off, flags_off, count_off, compact_off, compact_bytes, bytes;
};
MutualPlan mutual_plan(size_t ns, size_t nt) {
    MutualPlan p{};
    const size_t match_bytes = std::max(match_plan(ns, nt).bytes, match_plan(nt, ns).bytes);
    p.match_off = 0;
    p.s2t_off = align16(match_bytes);
    p.t2s_off = p.s2t_off + align16(4 * ns);
    p.pairs_off = p.t2s_off + align16(4 * nt);
    p.pairs_out_off = p.pairs_off + align16(8 * ns);
    p.flags_off = p.pairs_out_off + align16(8 * ns);
    p.count_off = p.flags_off + align16(ns);
    p.compact_off = p.count_off + 16;
    p.compact_bytes = sp_compact_workspace_bytes(ns);
    p.bytes = p.compact_off + align16(p.compact_bytes);
    return p;
}

__global__ __launch_bounds__(kBlock) void copy_pairs_kernel(const int2* __restrict__ in, const uint32_t* __restrict__ count,
                                                            unsigned cap, int2* __restrict__ out) {
    const unsigned n = min(*count, cap);
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) out[i] = in[i];
}

__global__ __launch_bounds__(kBlock) void correspondence_points_kernel(const float4* __restrict__ src, unsigned ns,
                                                                       const float4* __restrict__ tgt, unsigned nt,
                                                                       const int2* __restrict__ corr, unsigned m,
                                                                       float4* __restrict__ cs, float4* __restrict__ ct) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock) {
        const int2 c = corr[i];
        const bool s_ok = c.x >= 0 && (unsigned)c.x < ns, t_ok = c.y >= 0 && (unsigned)c.y < nt;  // (ns, nt >= 1)
        float4 a = src[s_ok ? c.x : 0], b = tgt[t_ok ? c.y : 0];
        if (!s_ok) a.x = a.y = a.z = a.w = NAN;  // an index outside its cloud matches nothing
        if (!t_ok) b.x = b.y = b.z = b.w = NAN;
        cs[i] = a;
        ct[i] = b;
    }
}

// ---------------------------------------------------------------------------------------------------------------- RANSAC
__host__ __device__ inline uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline void draw_triplet(uint64_t seed, uint64_t h, uint64_t m, uint32_t (&out)[3]) {
    for (int j = 0; j < 3; ++j) {
        const uint64_t r = splitmix64(seed + 3ull * h + (uint64_t)j);
        out[j] = (uint32_t)(((r >> 32) * m) >> 32);
    }
}

__host__ __device__ inline float sp_sqrt(float x) { return sqrtf(x); }
__host__ __device__ inline double sp_sqrt(double x) { return sqrt(x); }
__host__ __device__ inline float sp_fma(float a, float b, float c) { return fmaf(a, b, c); }
__host__ __device__ inline double sp_fma(double a, double b, double c) { return fma(a, b, c); }

template <class T>
__host__ __device__ inline T dot(const T (&a)[3], const T (&b)[3]) { return sp_fma(a[2], b[2], sp_fma(a[1], b[1], a[0] * b[0])); }
template <class T>
__host__ __device__ inline void cross(const T (&a)[3], const T (&b)[3], T (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// The frame [e1 e2 e3] (columns) of the triangle p0, p1, p2 and its centroid; false when a length vanishes or is not finite.
template <class T>
__host__ __device__ inline bool triangle_frame(const T (&p)[3][3], T (&F)[3][3], T (&c)[3]) {
    T e[3], f[3], n[3], e2[3];
    for (int a = 0; a < 3; ++a) e[a] = p[1][a] - p[0][a], f[a] = p[2][a] - p[0][a], c[a] = (p[0][a] + p[1][a] + p[2][a]) / (T)3;
    const T le = sp_sqrt(dot(e, e));
    if (!(le > (T)0) || !(le < (T)INFINITY)) return false;
    for (int a = 0; a < 3; ++a) e[a] /= le;
    cross(e, f, n);
    const T ln = sp_sqrt(dot(n, n));
    if (!(ln > (T)0) || !(ln < (T)INFINITY)) return false;
    for (int a = 0; a < 3; ++a) n[a] /= ln;
    cross(n, e, e2);
    for (int a = 0; a < 3; ++a) F[a][0] = e[a], F[a][1] = e2[a], F[a][2] = n[a];
    return true;
}
// The gates of a hypothesis (the header's list) on the two triangles.
template <class T>
__host__ __device__ inline bool triangle_gates(const T (&ps)[3][3], const T (&pt)[3][3], T min_edge, T edge_ratio) {
    const int ea[3] = {0, 0, 1}, eb[3] = {1, 2, 2};
    for (int k = 0; k < 3; ++k) {
        T ds[3], dt[3];
        for (int a = 0; a < 3; ++a) ds[a] = ps[eb[k]][a] - ps[ea[k]][a], dt[a] = pt[eb[k]][a] - pt[ea[k]][a];
        const T ls = sp_sqrt(dot(ds, ds)), lt = sp_sqrt(dot(dt, dt));
        if (!(ls > min_edge)) return false;
        const T lo = ls < lt ? ls : lt, hi = ls < lt ? lt : ls;
        if (!(lo >= edge_ratio * hi)) return false;
    }
    for (int s = 0; s < 2; ++s) {
        const T(&p)[3][3] = s ? pt : ps;
        T e[3], f[3], n[3];
        for (int a = 0; a < 3; ++a) e[a] = p[1][a] - p[0][a], f[a] = p[2][a] - p[0][a];
        cross(e, f, n);
        if (!(dot(n, n) >= (T)0.04 * dot(e, e) * dot(f, f))) return false;
    }
    return true;
}
// R (row-major) and t of the pose that takes the source triangle's frame onto the target triangle's.
template <class T>
__host__ __device__ inline bool triangle_pose(const T (&ps)[3][3], const T (&pt)[3][3], T (&R)[9], T (&t)[3]) {
    T Fs[3][3], Ft[3][3], cs[3], ct[3];
    if (!triangle_frame(ps, Fs, cs) || !triangle_frame(pt, Ft, ct)) return false;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[3 * a + b] = sp_fma(Ft[a][2], Fs[b][2], sp_fma(Ft[a][1], Fs[b][1], Ft[a][0] * Fs[b][0]));
    for (int a = 0; a < 3; ++a) t[a] = ct[a] - sp_fma(R[3 * a + 2], cs[2], sp_fma(R[3 * a + 1], cs[1], R[3 * a] * cs[0]));
    return true;
}

constexpr unsigned kScoreTile = kBlock;  // matches per LDS tile

__global__ __launch_bounds__(kBlock) void ransac_score_kernel(const float4* __restrict__ cs, const float4* __restrict__ ct, unsigned m,
                                                              unsigned hypotheses, uint64_t seed, float tau2, float min_edge,
                                                              float edge_ratio, uint32_t* __restrict__ score) {
    __shared__ float4 s_cs[kScoreTile], s_ct[kScoreTile];
    const unsigned tid = threadIdx.x;
    const unsigned hyp = blockIdx.x * kBlock + tid;
    bool ok = false;
    float R[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, t[3] = {0.0f, 0.0f, 0.0f};
    if (hyp < hypotheses) {
        uint32_t id[3];
        draw_triplet(seed, hyp, m, id);  // (every index < m)
        if (id[0] != id[1] && id[0] != id[2] && id[1] != id[2]) {
            float ps[3][3], pt[3][3];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const float4 a = cs[id[v]], b = ct[id[v]];
                ps[v][0] = a.x, ps[v][1] = a.y, ps[v][2] = a.z;
                pt[v][0] = b.x, pt[v][1] = b.y, pt[v][2] = b.z;
            }
            ok = triangle_gates(ps, pt, min_edge, edge_ratio) && triangle_pose(ps, pt, R, t);
        }
    }
    unsigned count = 0;
    for (unsigned base = 0; base < m; base += kScoreTile) {
        __syncthreads();
        if (base + tid < m) s_cs[tid] = cs[base + tid], s_ct[tid] = ct[base + tid];
        __syncthreads();
        const unsigned lim = min(kScoreTile, m - base);
        if (ok) {
            for (unsigned c = 0; c < lim; ++c) {  // (every lane reads the same address: a broadcast)
                const float4 a = s_cs[c], b = s_ct[c];
                const float rx = fmaf(R[2], a.z, fmaf(R[1], a.y, fmaf(R[0], a.x, t[0]))) - b.x;
                const float ry = fmaf(R[5], a.z, fmaf(R[4], a.y, fmaf(R[3], a.x, t[1]))) - b.y;
                const float rz = fmaf(R[8], a.z, fmaf(R[7], a.y, fmaf(R[6], a.x, t[2]))) - b.z;
                count += fmaf(rz, rz, fmaf(ry, ry, rx * rx)) < tau2 ? 1u : 0u;
            }
        }
    }
    if (hyp < hypotheses) score[hyp] = ok ? count : 0u;
}

__global__ __launch_bounds__(kBlock) void zero_u32_kernel(uint32_t* __restrict__ p, unsigned n) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) p[i] = 0u;
}

}  // namespace
}  // namespace sp

extern "C" size_t sp_fpfh_workspace_bytes(size_t n) { return n < sp::kMaxCloud ? n * sp::kStride * sizeof(float) : 0; }

extern "C" int sp_fpfh_compute(const float* points, const float* normals, size_t n, const int32_t* knn_idx, const float* knn_d2,
                               size_t k, float* fpfh_out, uint16_t* spfh_counts_out_opt, uint16_t* spfh_m_out_opt, void* workspace,
                               size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (k == 0 || k > SP_FPFH_MAX_K) {
        sp_set_error("[sp_fpfh_compute] k must be in 1..SP_FPFH_MAX_K (64): a wave holds a point's neighbours, one per lane");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (n >= kMaxCloud) {
        sp_set_error("[sp_fpfh_compute] n >= 2^31: neighbour indices are int32");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return SP_OK;
    if (!points || !normals || !knn_idx || !knn_d2 || !fpfh_out || !workspace) {
        sp_set_error("[sp_fpfh_compute] null argument (points, normals, knn_idx, knn_d2, fpfh_out, workspace)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (workspace_bytes < sp_fpfh_workspace_bytes(n) || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
        sp_set_error("[sp_fpfh_compute] the workspace is smaller than sp_fpfh_workspace_bytes(n) or not 16-byte aligned");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    float* spfh = static_cast<float*>(workspace);
    const unsigned grid = stream_grid(n, kBlock / kWave);  // a wave per point
    spfh_kernel<<<grid, kBlock, 0, st>>>(reinterpret_cast<const float4*>(points), reinterpret_cast<const float4*>(normals), (unsigned)n,
                                         knn_idx, (unsigned)k, spfh, spfh_counts_out_opt, spfh_m_out_opt);
    fpfh_kernel<<<grid, kBlock, 0, st>>>(spfh, (unsigned)n, knn_idx, knn_d2, (unsigned)k, fpfh_out);
    return launch_status();
}

extern "C" size_t sp_feature_match_workspace_bytes(size_t na, size_t nb) {
    if (na > SP_FEATURE_MATCH_MAX || nb > SP_FEATURE_MATCH_MAX) return 0;
    return std::max<size_t>(sp::match_plan(na, nb).bytes, 16);
}

namespace {
int check_match_args(const char* who, const float* a, size_t na, const float* b, size_t nb, const void* out, const void* workspace) {
    char msg[256];
    if (na > SP_FEATURE_MATCH_MAX || nb > SP_FEATURE_MATCH_MAX) {
        snprintf(msg, sizeof msg, "[%s] more than SP_FEATURE_MATCH_MAX (2^20) rows", who);
        sp_set_error(msg);
        return SP_ERR_INVALID_ARGUMENT;
    }
    if ((na && (!a || !out || !workspace)) || (na && nb && !b)) {
        snprintf(msg, sizeof msg, "[%s] null argument", who);
        sp_set_error(msg);
        return SP_ERR_INVALID_ARGUMENT;
    }
    if ((na && reinterpret_cast<uintptr_t>(a) % 16 != 0) || (nb && reinterpret_cast<uintptr_t>(b) % 16 != 0) ||
        reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
        snprintf(msg, sizeof msg, "[%s] descriptor rows and workspace must be 16-byte aligned", who);
        sp_set_error(msg);
        return SP_ERR_INVALID_ARGUMENT;
    }
    return SP_OK;
}
}  // namespace

extern "C" int sp_feature_match(const float* a, size_t na, const float* b, size_t nb, int32_t* idx_out, float* d2_out_opt,
                                void* workspace, size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (const int rc = check_match_args("sp_feature_match", a, na, b, nb, idx_out, workspace); rc != SP_OK) return rc;
    if (na == 0) return SP_OK;
    if (workspace_bytes < sp_feature_match_workspace_bytes(na, nb)) {
        sp_set_error("[sp_feature_match] the workspace is smaller than sp_feature_match_workspace_bytes(na, nb)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    return match_enqueue(a, na, b, nb, idx_out, d2_out_opt, workspace, as_stream(stream));
}

extern "C" size_t sp_feature_match_mutual_workspace_bytes(size_t ns, size_t nt) {
    if (ns > SP_FEATURE_MATCH_MAX || nt > SP_FEATURE_MATCH_MAX) return 0;
    return std::max<size_t>(sp::mutual_plan(ns, nt).bytes, 16);
}

extern "C" int sp_feature_match_mutual(const float* src, size_t ns, const float* tgt, size_t nt, int32_t* corr_out,
                                       uint32_t* count_out_host, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (!count_out_host) {
        sp_set_error("[sp_feature_match_mutual] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (const int rc = check_match_args("sp_feature_match_mutual", src, ns, tgt, nt, corr_out, workspace); rc != SP_OK) return rc;
    if (ns && nt && workspace_bytes < sp_feature_match_mutual_workspace_bytes(ns, nt)) {
        sp_set_error("[sp_feature_match_mutual] the workspace is smaller than sp_feature_match_mutual_workspace_bytes(ns, nt)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    *count_out_host = 0;
    if (ns == 0 || nt == 0) return SP_OK;
    hipStream_t st = as_stream(stream);
    const MutualPlan p = mutual_plan(ns, nt);
    char* ws = static_cast<char*>(workspace);
    auto* s2t = reinterpret_cast<int32_t*>(ws + p.s2t_off);
    auto* t2s = reinterpret_cast<int32_t*>(ws + p.t2s_off);
    auto* pairs = reinterpret_cast<int2*>(ws + p.pairs_off);
    auto* pairs_out = reinterpret_cast<int2*>(ws + p.pairs_out_off);
    auto* flags = reinterpret_cast<uint8_t*>(ws + p.flags_off);
    auto* count = reinterpret_cast<uint32_t*>(ws + p.count_off);
    if (const int rc = match_enqueue(src, ns, tgt, nt, s2t, nullptr, ws + p.match_off, st); rc != SP_OK) return rc;
    if (const int rc = match_enqueue(tgt, nt, src, ns, t2s, nullptr, ws + p.match_off, st); rc != SP_OK) return rc;
    mutual_flags_kernel<<<stream_grid(ns), kBlock, 0, st>>>(s2t, t2s, (unsigned)ns, (unsigned)nt, pairs, flags);
    if (const int rc = sp_compact_by_flags(pairs, ns, sizeof(int2), flags, pairs_out, nullptr, count, ws + p.compact_off,
                                           p.compact_bytes, stream);
        rc != SP_OK)
        return rc;
    const unsigned cap = (unsigned)std::min(ns, nt);  // (a mutual match is an injection both ways)
    copy_pairs_kernel<<<stream_grid(cap), kBlock, 0, st>>>(pairs_out, count, cap, reinterpret_cast<int2*>(corr_out));
    if (const int rc = launch_status(); rc != SP_OK) return rc;
    uint32_t host_count = 0;
    hipError_t e = hipMemcpyAsync(&host_count, count, sizeof host_count, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        sp_set_error(hipGetErrorString(e));
        return SP_ERR_HIP;
    }
    *count_out_host = std::min<uint32_t>(host_count, cap);
    return SP_OK;
}

extern "C" int sp_correspondence_points(const float* src_points, size_t ns, const float* tgt_points, size_t nt, const int32_t* corr,
                                        size_t m, float* cs_out, float* ct_out, void* stream) {
    using namespace sp;
    if (m == 0) return SP_OK;
    if (!src_points || !tgt_points || !corr || !cs_out || !ct_out || ns == 0 || nt == 0 || ns >= kMaxCloud || nt >= kMaxCloud ||
        m >= kMaxCloud) {
        sp_set_error("[sp_correspondence_points] null argument, an empty cloud with m > 0, or more than 2^31 rows");
        return SP_ERR_INVALID_ARGUMENT;
    }
    correspondence_points_kernel<<<stream_grid(m), kBlock, 0, as_stream(stream)>>>(
        reinterpret_cast<const float4*>(src_points), (unsigned)ns, reinterpret_cast<const float4*>(tgt_points), (unsigned)nt,
        reinterpret_cast<const int2*>(corr), (unsigned)m, reinterpret_cast<float4*>(cs_out), reinterpret_cast<float4*>(ct_out));
    return launch_status();
}

extern "C" int sp_ransac_score(const float* cs, const float* ct, size_t m, size_t hypotheses, uint64_t seed, float inlier_distance,
                               float min_edge, float edge_ratio, uint32_t* score_out, void* stream) {
    using namespace sp;
    if (hypotheses > SP_RANSAC_MAX_HYPOTHESES || m >= kMaxCloud) {
        sp_set_error("[sp_ransac_score] more than SP_RANSAC_MAX_HYPOTHESES (2^20) hypotheses or 2^31 matches");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (hypotheses == 0) return SP_OK;
    if (!score_out || (m >= 3 && (!cs || !ct))) {
        sp_set_error("[sp_ransac_score] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (!(inlier_distance >= 0.0f) || !(min_edge >= 0.0f) || !(edge_ratio >= 0.0f && edge_ratio <= 1.0f)) {
        sp_set_error("[sp_ransac_score] inlier_distance and min_edge must not be negative, edge_ratio must lie in [0, 1]");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    if (m < 3) {
        zero_u32_kernel<<<stream_grid(hypotheses), kBlock, 0, st>>>(score_out, (unsigned)hypotheses);
        return launch_status();
    }
    ransac_score_kernel<<<div_up(hypotheses, kBlock), kBlock, 0, st>>>(reinterpret_cast<const float4*>(cs),
                                                                      reinterpret_cast<const float4*>(ct), (unsigned)m,
                                                                      (unsigned)hypotheses, seed, inlier_distance * inlier_distance,
                                                                      min_edge, edge_ratio, score_out);
    return launch_status();
}

extern "C" int sp_ransac_triplets_host(uint64_t seed, size_t first_hypothesis, size_t count, size_t m, uint32_t* triplets_out) {
    if (count && !triplets_out) {
        sp_set_error("[sp_ransac_triplets_host] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (m >= sp::kMaxCloud) {
        sp_set_error("[sp_ransac_triplets_host] more than 2^31 matches");
        return SP_ERR_INVALID_ARGUMENT;
    }
    for (size_t h = 0; h < count; ++h) {
        uint32_t id[3];
        sp::draw_triplet(seed, first_hypothesis + h, m, id);
        for (int j = 0; j < 3; ++j) triplets_out[3 * h + j] = id[j];
    }
    return SP_OK;
}

extern "C" int sp_ransac_select_host(const uint32_t* scores_host, size_t hypotheses, const float* cs_host, const float* ct_host,
                                     size_t m, uint64_t seed, size_t guesses, double* poses_out, uint32_t* hyp_out_opt,
                                     size_t* count_out) {
    using namespace sp;
    if (!count_out) {
        sp_set_error("[sp_ransac_select_host] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    *count_out = 0;
    if (hypotheses > SP_RANSAC_MAX_HYPOTHESES || m >= kMaxCloud) {
        sp_set_error("[sp_ransac_select_host] more than SP_RANSAC_MAX_HYPOTHESES (2^20) hypotheses or 2^31 matches");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (guesses == 0 || hypotheses == 0 || m < 3) return SP_OK;
    if (!scores_host || !cs_host || !ct_host || !poses_out) {
        sp_set_error("[sp_ransac_select_host] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    std::vector<uint32_t> order;
    order.reserve(hypotheses);
    for (size_t h = 0; h < hypotheses; ++h)
        if (scores_host[h]) order.push_back((uint32_t)h);
    const size_t want = std::min(guesses, order.size());
    std::partial_sort(order.begin(), order.begin() + want, order.end(), [&](uint32_t a, uint32_t b) {
        return scores_host[a] != scores_host[b] ? scores_host[a] > scores_host[b] : a < b;
    });
    size_t written = 0;
    for (size_t g = 0; g < want; ++g) {
        uint32_t id[3];
        draw_triplet(seed, order[g], m, id);
        double ps[3][3], pt[3][3], R[9], t[3];
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) ps[v][a] = (double)cs_host[4 * (size_t)id[v] + a], pt[v][a] = (double)ct_host[4 * (size_t)id[v] + a];
        if (!triangle_pose(ps, pt, R, t)) continue;  // (a degenerate triangle cannot have scored)
        double* T = poses_out + 16 * written;
        for (int c = 0; c < 3; ++c) {
            for (int r = 0; r < 3; ++r) T[4 * c + r] = R[3 * r + c];
            T[4 * c + 3] = 0.0;
        }
        T[12] = t[0], T[13] = t[1], T[14] = t[2], T[15] = 1.0;
        if (hyp_out_opt) hyp_out_opt[written] = order[g];
        ++written;
    }
    *count_out = written;
    return SP_OK;
}
