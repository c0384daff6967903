// Compatibility-graph guesses for gfx950 (MI355X extension): initial guesses for sp_gicp_align_batch where the
// inliers are a few per cent of the matches and random triplets (sp_ransac_score) find none.
//   sp_compat_seeds        C (who is compatible with whom), s = row sums of C o (C C^T) on the int8 matrix cores, the best seeds
//   sp_compat_consensus    row a of S for the seeds only (a second, small matrix-core launch), the k best companions of each
//   sp_compat_poses_host   least-squares pose of each consensus set (Horn, double)
//   sp_pose_score          one lane per pose: the matches it explains (sp_ransac_score's residual expression)
//   sp_compat_select_host  the best-scoring poses
//   sp_compat_seeds_host, sp_compat_consensus_host: the twins on host memory, bit rows and popcounts.
// The definitions are include/sycl_points_amd.h's. Integers and one fixed f32 predicate: every result is the same bits on every call.
//
// C in memory as BYTES, Mp x Mp (Mp = M rounded up to 128, the pad zero), not as bits expanded in registers: a 0/1 byte IS an int8
// matrix-core operand, so a lane's 16-byte read is a fragment with no vector work between the load and the MFMA. Expanding bits
// costs at least one v_perm/v_and per 4 operand bytes: 4 vector instructions per fragment where the MFMA that consumes two
// fragments takes 8 passes; and evaluating the predicate in the product kernel (16 pairs per lane per operand) costs ~400
// vector cycles per 32-cycle MFMA. 64 MiB at M = 8192 stays in the Infinity Cache.
//
// Product (second_order_kernel): D[i][j] = sum_k A[i][k] B[k][j] with A[i][k] = C[ra + i][k] and B[k][j] = C[rb + j][k] (C is
// symmetric, so BOTH operands read rows): lane (r = lane & 31, h = lane >> 5) holds 16 bytes of row r. The assignment of those
// bytes to the instruction's k index does not matter as long as both operands use the same one, so a lane reads 64 contiguous
// bytes of its row per 128-wide K chunk (bytes [64 h, 64 h + 64)) and the j-th 16 of them feed the j-th MFMA of the chunk. A wave
// holds a 64 x 64 block of D (four 32 x 32 accumulators), a workgroup 128 x 128. D has the B row on the lane and 16 A rows in the
// lane's registers (row = (reg & 3) + 8 (reg >> 2) + 4 h): the lane masks each with C[b][a] (one 4-byte read per 4 registers,
// again by symmetry), adds them up (the column sum of S, which is the row sum of the symmetric S), adds the other lane half and
// issues one integer atomicAdd per column. S is never stored.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sp_common.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

constexpr unsigned kPad = 128;         // rows and row length of C are padded to this: the block tile of the product, its K chunk
constexpr unsigned kSeedRows = SP_COMPAT_MAX_SEEDS;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

inline size_t padded(size_t m) { return (m + kPad - 1) / kPad * kPad; }

// ---------------------------------------------------------------------------------------------------------- 1. the predicate
// s_a, s_b: the two source points; t_a, t_b: the two target points (x, y, z). t2 = tau^2, e2 = min_edge^2, both rounded once.
__host__ __device__ inline bool compatible(const float* sa, const float* sb, const float* ta, const float* tb, float t2, float e2) {
    const float dx = sa[0] - sb[0], dy = sa[1] - sb[1], dz = sa[2] - sb[2];
    const float gx = ta[0] - tb[0], gy = ta[1] - tb[1], gz = ta[2] - tb[2];
    const float u = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const float v = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
    const float q = (u + v) - t2;
    return u > e2 && v > e2 && (q < 0.0f || q * q < (4.0f * u) * v);  // (false for NaN)
}

// One row of C per blockIdx.y, four columns per lane, written as one 32-bit word; rows and columns >= m are zero.
__global__ __launch_bounds__(kBlock) void compat_kernel(const float4* __restrict__ cs, const float4* __restrict__ ct, unsigned m,
                                                        unsigned mp, float t2, float e2, uint32_t* __restrict__ c_words,
                                                        uint32_t* __restrict__ degree) {
    const unsigned a = blockIdx.y;
    const unsigned word = blockIdx.x * kBlock + threadIdx.x;  // of the row
    const unsigned words = mp / 4;
    unsigned bits = 0, cnt = 0;
    if (a < m && word < words) {
        const float4 pa = cs[a], qa = ct[a];
        const float sa[3] = {pa.x, pa.y, pa.z}, ta[3] = {qa.x, qa.y, qa.z};
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
            const unsigned b = 4 * word + j;
            if (b < m && b != a) {
                const float4 pb = cs[b], qb = ct[b];
                const float sb[3] = {pb.x, pb.y, pb.z}, tb[3] = {qb.x, qb.y, qb.z};
                if (compatible(sa, sb, ta, tb, t2, e2)) bits |= 1u << (8 * j), ++cnt;
            }
        }
    }
    if (word < words) c_words[(size_t)a * words + word] = bits;
    cnt = wave_sum_u32(cnt);
    if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(&degree[a], cnt);  // (a < m here: cnt is 0 otherwise)
}

// ------------------------------------------------------------------------------------------------------- 2. the second order
__device__ __forceinline__ i32x4 as_fragment(const uint4& v) {
    i32x4 f;
    f[0] = (int)v.x, f[1] = (int)v.y, f[2] = (int)v.z, f[3] = (int)v.w;
    return f;
}

// grid (mp / 128, mp / 128): blockIdx.y the A rows (summed over in the epilogue), blockIdx.x the B rows (the columns whose sums are
// written). Every index is below mp by construction: no bounds checks. A K chunk (128 A rows and 128 B rows of 128 bytes) goes
// through LDS: eight consecutive lanes fetch one row's 128 bytes (one cache line), the next chunk is fetched into registers while
// this one is multiplied, and a wave reads its fragments from LDS rows of 144 bytes (the 16-byte pad spreads the 32 rows of a
// fragment read over the banks). Read straight from memory, a fragment load touches 32 cache lines for 16 bytes each and the
// kernel waits on the texture addresser, not the matrix cores (measured at M = 8192: 2 079 us so, 505 us through LDS).
constexpr unsigned kLdsRow = kPad + 16;  // bytes
__global__ __launch_bounds__(kBlock) void second_order_kernel(const uint8_t* __restrict__ c, unsigned mp, uint32_t* __restrict__ s) {
    __shared__ __attribute__((aligned(16))) uint8_t s_a[kPad * kLdsRow], s_b[kPad * kLdsRow];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, h = lane >> 5;
    const unsigned a0 = blockIdx.y * kPad, b0 = blockIdx.x * kPad;
    const unsigned ra = (wave >> 1) * 64u, rb = (wave & 1u) * 64u;  // of the wave's 64 x 64 block inside the workgroup's
    // lane -> (row, 16-byte segment) of the four fetches: v = tid + 256 u, row = v / 8, segment = v % 8
    const uint8_t* src_a = c + (size_t)(a0 + (tid >> 3)) * mp + 16u * (tid & 7u);
    const uint8_t* src_b = c + (size_t)(b0 + (tid >> 3)) * mp + 16u * (tid & 7u);
    const size_t src_step = (size_t)32 * mp;  // 256 lanes are 32 rows
    const unsigned dst = (tid >> 3) * kLdsRow + 16u * (tid & 7u), dst_step = 32u * kLdsRow;
    uint4 pa0, pa1, pa2, pa3, pb0, pb1, pb2, pb3;
#define SP_COMPAT_FETCH(kb)                                                 \
    pa0 = *reinterpret_cast<const uint4*>(src_a + (kb));                    \
    pa1 = *reinterpret_cast<const uint4*>(src_a + src_step + (kb));         \
    pa2 = *reinterpret_cast<const uint4*>(src_a + 2 * src_step + (kb));     \
    pa3 = *reinterpret_cast<const uint4*>(src_a + 3 * src_step + (kb));     \
    pb0 = *reinterpret_cast<const uint4*>(src_b + (kb));                    \
    pb1 = *reinterpret_cast<const uint4*>(src_b + src_step + (kb));         \
    pb2 = *reinterpret_cast<const uint4*>(src_b + 2 * src_step + (kb));     \
    pb3 = *reinterpret_cast<const uint4*>(src_b + 3 * src_step + (kb));
    i32x16 acc[2][2];
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ta][tb][e] = 0;
    SP_COMPAT_FETCH(0u)
    for (unsigned kb = 0; kb < mp; kb += kPad) {
        __syncthreads();  // the chunk before has been read
        *reinterpret_cast<uint4*>(s_a + dst) = pa0, *reinterpret_cast<uint4*>(s_a + dst + dst_step) = pa1;
        *reinterpret_cast<uint4*>(s_a + dst + 2 * dst_step) = pa2, *reinterpret_cast<uint4*>(s_a + dst + 3 * dst_step) = pa3;
        *reinterpret_cast<uint4*>(s_b + dst) = pb0, *reinterpret_cast<uint4*>(s_b + dst + dst_step) = pb1;
        *reinterpret_cast<uint4*>(s_b + dst + 2 * dst_step) = pb2, *reinterpret_cast<uint4*>(s_b + dst + 3 * dst_step) = pb3;
        __syncthreads();
        if (kb + kPad < mp) {
            SP_COMPAT_FETCH(kb + kPad)
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint4 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *reinterpret_cast<const uint4*>(s_a + (ra + 32u * t + r) * kLdsRow + 64u * h + 16u * j);
                b[t] = *reinterpret_cast<const uint4*>(s_b + (rb + 32u * t + r) * kLdsRow + 64u * h + 16u * j);
            }
#pragma unroll
            for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
                    acc[ta][tb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(as_fragment(a[ta]), as_fragment(b[tb]), acc[ta][tb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
        const unsigned col = b0 + rb + 32u * tb + r;
        const uint8_t* mask_row = c + (size_t)col * mp + a0 + ra;  // C[col][a] == C[a][col]
        unsigned sum = 0;
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(mask_row + 32u * ta + 8u * g + 4u * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) sum += ((w >> (8 * e)) & 1u) ? (unsigned)acc[ta][tb][4 * g + e] : 0u;
            }
        sum += (unsigned)__shfl_xor((int)sum, 32, 64);
        if (h == 0 && sum) atomicAdd(&s[col], sum);
    }
#undef SP_COMPAT_FETCH
}

// ------------------------------------------------------------------------------------------------------------------ 3. seeds
__global__ __launch_bounds__(kBlock) void fill_i32_kernel(int32_t* __restrict__ p, unsigned n, int32_t value) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) p[i] = value;
}

// The rank of match a under the key (s descending, a ascending) is the number of matches that come before it; the keys are all
// different, so the ranks below `seeds` are taken exactly once each. One lane per match; blockIdx.y takes a chunk of 1 024 rivals
// (through LDS, four a read; the pad of the last chunk holds zeros, which come before nothing that can be a seed) and the chunks'
// counts meet in an integer atomicAdd. (One workgroup row walking all M rivals took 221 us at M = 8192.)
constexpr unsigned kRankChunk = 1024;
__global__ __launch_bounds__(kBlock) void seed_rank_kernel(const uint32_t* __restrict__ s, unsigned m, uint32_t* __restrict__ rank) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[kRankChunk];
    const unsigned a = blockIdx.x * kBlock + threadIdx.x, base = blockIdx.y * kRankChunk;
    const uint32_t mine = a < m ? s[a] : 0u;
    for (unsigned j = threadIdx.x; j < kRankChunk; j += kBlock) s_tile[j] = base + j < m ? s[base + j] : 0u;
    __syncthreads();
    unsigned before = 0;
    const unsigned lim = min(kRankChunk, (m - base + 3u) & ~3u);  // (base < m: the grid has no empty chunk)
#pragma unroll 8
    for (unsigned j = 0; j < lim; j += 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(&s_tile[j]);
        const uint32_t other[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (unsigned e = 0; e < 4; ++e) before += (other[e] > mine || (other[e] == mine && base + j + e < a)) ? 1u : 0u;
    }
    if (a < m && mine && before) atomicAdd(&rank[a], before);
}
__global__ __launch_bounds__(kBlock) void seed_scatter_kernel(const uint32_t* __restrict__ s, const uint32_t* __restrict__ degree,
                                                              const uint32_t* __restrict__ rank, unsigned m, unsigned seeds,
                                                              int32_t* __restrict__ seed_idx, uint32_t* __restrict__ seed_s,
                                                              uint32_t* __restrict__ degree_out, uint32_t* __restrict__ s_out) {
    const unsigned a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= m) return;
    const uint32_t mine = s[a], r = rank[a];
    if (mine && r < seeds) seed_idx[r] = (int32_t)a, seed_s[r] = mine;
    if (degree_out) degree_out[a] = degree[a];
    if (s_out) s_out[a] = mine;
}

// -------------------------------------------------------------------------------------------------------------- 4. consensus
// S[a][.] for the seeds: grid (mp / 128, seed tiles of 32). The A operand holds the rows of 32 seeds (zeros for an empty slot), a
// wave's B operand 32 rows of C; two accumulators take the even and the odd K steps and are added. Row (slot) x column (b) of the
// result is masked with C[a_slot][b] and stored: for one register the lanes of a half write 32 consecutive words.
__global__ __launch_bounds__(kBlock) void seed_rows_kernel(const uint8_t* __restrict__ c, unsigned mp, const int32_t* __restrict__ seed_idx,
                                                           unsigned seeds, unsigned m, uint32_t* __restrict__ rows_out) {
    __shared__ int32_t s_seed[32];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, r = lane & 31u, h = lane >> 5;
    const unsigned slot0 = blockIdx.y * 32u;
    if (threadIdx.x < 32u) {
        const int32_t a = slot0 + threadIdx.x < seeds ? seed_idx[slot0 + threadIdx.x] : -1;
        s_seed[threadIdx.x] = a >= 0 && (unsigned)a < m ? a : -1;
    }
    __syncthreads();
    const int32_t mine = s_seed[r];
    const unsigned col = blockIdx.x * kPad + wave * 32u + r;
    const uint8_t* arow = c + (size_t)(mine < 0 ? 0 : mine) * mp + 64u * h;
    const uint8_t* brow = c + (size_t)col * mp + 64u * h;
    i32x16 acc0, acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc0[e] = 0, acc1[e] = 0;
    const unsigned keep = mine < 0 ? 0u : ~0u;  // an empty slot multiplies zeros
    for (unsigned kb = 0; kb < mp; kb += kPad) {
        uint4 a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = reinterpret_cast<const uint4*>(arow + kb)[j];
            b[j] = reinterpret_cast<const uint4*>(brow + kb)[j];
            a[j].x &= keep, a[j].y &= keep, a[j].z &= keep, a[j].w &= keep;
        }
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(as_fragment(a[0]), as_fragment(b[0]), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(as_fragment(a[1]), as_fragment(b[1]), acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(as_fragment(a[2]), as_fragment(b[2]), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(as_fragment(a[3]), as_fragment(b[3]), acc1, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const unsigned slot = (e & 3) + 8 * (e >> 2) + 4 * h;
        const int32_t a = s_seed[slot];
        const unsigned masked = a >= 0 && c[(size_t)a * mp + col] ? (unsigned)(acc0[e] + acc1[e]) : 0u;
        rows_out[(size_t)(slot0 + slot) * mp + col] = masked;
    }
}

constexpr unsigned kRowMax = SP_COMPAT_MAX_MATCHES;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

// One workgroup per seed rank: k rounds of a maximum over the key S << 32 | ~b (S descending, b ascending; the keys are all
// different), the winner taken out of the row in LDS.
__global__ __launch_bounds__(kBlock) void consensus_kernel(const uint32_t* __restrict__ rows, unsigned mp, unsigned m,
                                                           const int32_t* __restrict__ seed_idx, unsigned k,
                                                           int32_t* __restrict__ cons, uint32_t* __restrict__ cons_s) {
    __shared__ uint32_t s_row[kRowMax];
    __shared__ unsigned long long s_best[kBlock / kWave];
    const unsigned rank = blockIdx.x, tid = threadIdx.x;
    const int32_t a = seed_idx[rank];
    const bool live = a >= 0 && (unsigned)a < m;  // (uniform)
    for (unsigned b = tid; b < m; b += kBlock) s_row[b] = live ? rows[(size_t)rank * mp + b] : 0u;
    __syncthreads();
    for (unsigned round = 0; round < k; ++round) {
        unsigned long long best = 0;
        for (unsigned b = tid; b < m; b += kBlock) {
            const uint32_t v = s_row[b];
            const unsigned long long key = v ? ((unsigned long long)v << 32) | (uint32_t)~b : 0ull;
            best = key > best ? key : best;
        }
        best = wave_max_u64(best);
        if ((tid & 63u) == 0) s_best[tid >> 6] = best;
        __syncthreads();
#pragma unroll
        for (unsigned w = 0; w < kBlock / kWave; ++w) best = s_best[w] > best ? s_best[w] : best;
        const unsigned b_best = ~(uint32_t)(best & 0xffffffffull);
        if (tid == 0) {
            cons[(size_t)rank * k + round] = best ? (int32_t)b_best : -1;
            if (cons_s) cons_s[(size_t)rank * k + round] = (uint32_t)(best >> 32);
            if (best) s_row[b_best] = 0u;
        }
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------------------------------------- 6. scores
constexpr unsigned kScoreTile = kBlock;  // matches per LDS tile

// poses: 16 floats each, column-major. The counting loop is sp_ransac_score's, expression for expression. blockIdx.y takes
// `tiles_per_block` tiles of the matches, so that a few poses still fill the device; the counts of the chunks meet in an integer
// atomicAdd on the zeroed scores.
__global__ __launch_bounds__(kBlock) void pose_score_kernel(const float4* __restrict__ cs, const float4* __restrict__ ct, unsigned m,
                                                            const float* __restrict__ poses, unsigned count, float tau2,
                                                            unsigned tiles_per_block, uint32_t* __restrict__ score) {
    __shared__ float4 s_cs[kScoreTile], s_ct[kScoreTile];
    const unsigned tid = threadIdx.x;
    const unsigned p = blockIdx.x * kBlock + tid;
    const bool ok = p < count;
    float R[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, t[3] = {0.0f, 0.0f, 0.0f};
    if (ok) {
        const float* T = poses + 16 * (size_t)p;
#pragma unroll
        for (int row = 0; row < 3; ++row) {
#pragma unroll
            for (int col = 0; col < 3; ++col) R[3 * row + col] = T[4 * col + row];
            t[row] = T[12 + row];
        }
    }
    unsigned n = 0;
    const unsigned first = blockIdx.y * tiles_per_block * kScoreTile;
    const unsigned last = min(m, first + tiles_per_block * kScoreTile);
    for (unsigned base = first; base < last; base += kScoreTile) {
        __syncthreads();
        if (base + tid < last) s_cs[tid] = cs[base + tid], s_ct[tid] = ct[base + tid];
        __syncthreads();
        const unsigned lim = min(kScoreTile, last - base);
        if (ok) {
            for (unsigned i = 0; i < lim; ++i) {  // (every lane reads the same address: a broadcast)
                const float4 a = s_cs[i], b = s_ct[i];
                const float rx = fmaf(R[2], a.z, fmaf(R[1], a.y, fmaf(R[0], a.x, t[0]))) - b.x;
                const float ry = fmaf(R[5], a.z, fmaf(R[4], a.y, fmaf(R[3], a.x, t[1]))) - b.y;
                const float rz = fmaf(R[8], a.z, fmaf(R[7], a.y, fmaf(R[6], a.x, t[2]))) - b.z;
                n += fmaf(rz, rz, fmaf(ry, ry, rx * rx)) < tau2 ? 1u : 0u;
            }
        }
    }
    if (ok && n) atomicAdd(&score[p], n);
}

// ---------------------------------------------------------------------------------------------------------------- host twins
struct HostGraph {  // C as bit rows
    size_t m = 0, words = 0;
    std::vector<uint64_t> bits;
    const uint64_t* row(size_t a) const { return bits.data() + a * words; }
    bool at(size_t a, size_t b) const { return (row(a)[b >> 6] >> (b & 63)) & 1ull; }
};
HostGraph host_graph(const float* cs, const float* ct, size_t m, float tau, float min_edge) {
    HostGraph g;
    g.m = m, g.words = (m + 63) / 64;
    g.bits.assign(m * g.words, 0ull);
    const float t2 = tau * tau, e2 = min_edge * min_edge;
    for (size_t a = 0; a < m; ++a)
        for (size_t b = 0; b < m; ++b)
            if (a != b && compatible(cs + 4 * a, cs + 4 * b, ct + 4 * a, ct + 4 * b, t2, e2)) g.bits[a * g.words + (b >> 6)] |= 1ull << (b & 63);
    return g;
}
inline uint32_t common_neighbours(const HostGraph& g, size_t a, size_t b) {
    uint32_t n = 0;
    const uint64_t *ra = g.row(a), *rb = g.row(b);
    for (size_t w = 0; w < g.words; ++w) n += (uint32_t)__builtin_popcountll(ra[w] & rb[w]);
    return n;
}

// Jacobi eigenvalue iteration on a symmetric N x N matrix in double: A is overwritten by the diagonal form, V receives the
// eigenvectors as columns.
template <int N>
void jacobi_eigen(double (&A)[N][N], double (&V)[N][N]) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) (i == j ? diag : off) += A[i][j] * A[i][j];
        if (!(off > 1e-40 * diag)) break;  // (also leaves on NaN)
        for (int p = 0; p < N; ++p)
            for (int q = p + 1; q < N; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cth = 1.0 / std::sqrt(t * t + 1.0), sth = t * cth;
                for (int i = 0; i < N; ++i) {  // A <- A J
                    const double aip = A[i][p], aiq = A[i][q];
                    A[i][p] = cth * aip - sth * aiq, A[i][q] = sth * aip + cth * aiq;
                }
                for (int i = 0; i < N; ++i) {  // A <- J^T A
                    const double api = A[p][i], aqi = A[q][i];
                    A[p][i] = cth * api - sth * aqi, A[q][i] = sth * api + cth * aqi;
                }
                A[p][q] = A[q][p] = 0.0;  // (what the rotation was chosen for)
                for (int i = 0; i < N; ++i) {
                    const double vip = V[i][p], viq = V[i][q];
                    V[i][p] = cth * vip - sth * viq, V[i][q] = sth * vip + cth * viq;
                }
            }
    }
}

// false when the points (rows of 3) are collinear, coincident or not finite: the middle eigenvalue of the scatter matrix
bool spans_a_plane(const std::vector<double>& p, const double (&mean)[3]) {
    double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, V[3][3];
    for (size_t i = 0; i < p.size() / 3; ++i)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) A[r][c] += (p[3 * i + r] - mean[r]) * (p[3 * i + c] - mean[c]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(A[r][c])) return false;
    jacobi_eigen(A, V);
    double ev[3] = {A[0][0], A[1][1], A[2][2]};
    std::sort(ev, ev + 3);
    return ev[2] > 0.0 && ev[1] > 1e-10 * ev[2];
}

// Horn's closed form: T (16 doubles, column-major) takes the source points onto the target points in the least-squares sense.
bool horn_pose(const std::vector<double>& ps, const std::vector<double>& pt, double* T) {
    const size_t n = ps.size() / 3;
    double ms[3] = {0.0, 0.0, 0.0}, mt[3] = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) ms[a] += ps[3 * i + a], mt[a] += pt[3 * i + a];
    for (int a = 0; a < 3; ++a) ms[a] /= (double)n, mt[a] /= (double)n;
    if (!spans_a_plane(ps, ms) || !spans_a_plane(pt, mt)) return false;
    double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // S[a][b] = sum (s - ms)_a (t - mt)_b
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) S[a][b] += (ps[3 * i + a] - ms[a]) * (pt[3 * i + b] - mt[b]);
    double N[4][4] = {{S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
                      {0.0, S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
                      {0.0, 0.0, -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
                      {0.0, 0.0, 0.0, -S[0][0] - S[1][1] + S[2][2]}};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < i; ++j) N[i][j] = N[j][i];
    double V[4][4];
    jacobi_eigen(N, V);
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (N[i][i] > N[best][best]) best = i;
    double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
    const double len = std::sqrt(w * w + x * x + y * y + z * z);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    w /= len, x /= len, y /= len, z /= len;
    const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                            {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                            {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
    for (int c = 0; c < 3; ++c) {
        for (int r = 0; r < 3; ++r) T[4 * c + r] = R[r][c];
        T[4 * c + 3] = 0.0;
    }
    for (int r = 0; r < 3; ++r) T[12 + r] = mt[r] - (R[r][0] * ms[0] + R[r][1] * ms[1] + R[r][2] * ms[2]);
    T[15] = 1.0;
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(T[i])) return false;
    return true;
}

struct Plan {
    size_t mp, c_off, degree_off, s_off, rank_off, rows_off, bytes;
};
Plan plan(size_t m) {
    Plan p{};
    p.mp = padded(m);
    p.c_off = 0;
    p.degree_off = p.mp * p.mp;
    p.s_off = p.degree_off + 4 * p.mp;
    p.rank_off = p.s_off + 4 * p.mp;
    p.rows_off = p.rank_off + 4 * p.mp;
    p.bytes = p.rows_off + (size_t)kSeedRows * p.mp * 4;
    return p;
}

int invalid(const char* msg) {
    sp_set_error(msg);
    return SP_ERR_INVALID_ARGUMENT;
}

}  // namespace
}  // namespace sp

extern "C" size_t sp_compat_workspace_bytes(size_t m) {
    if (m > SP_COMPAT_MAX_MATCHES) return 0;
    return sp::plan(std::max<size_t>(m, 1)).bytes;
}

extern "C" int sp_compat_seeds(const float* cs, const float* ct, size_t m, float tau, float min_edge, size_t seeds, int32_t* seed_idx_out,
                               uint32_t* seed_s_out, uint32_t* degree_out_opt, uint32_t* s_out_opt, void* workspace,
                               size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (m > SP_COMPAT_MAX_MATCHES) return invalid("[sp_compat_seeds] more than SP_COMPAT_MAX_MATCHES (8192) matches");
    if (seeds > SP_COMPAT_MAX_SEEDS) return invalid("[sp_compat_seeds] more than SP_COMPAT_MAX_SEEDS (256) seeds");
    if (!(tau > 0.0f) || !(min_edge >= 0.0f) || !std::isfinite(tau) || !std::isfinite(min_edge))
        return invalid("[sp_compat_seeds] tau must be finite and > 0, min_edge finite and not negative");
    if (seeds && (!seed_idx_out || !seed_s_out)) return invalid("[sp_compat_seeds] null argument (seed_idx_out, seed_s_out)");
    if (m >= 3) {
        if (!cs || !ct || !workspace) return invalid("[sp_compat_seeds] null argument (cs, ct, workspace)");
        if (workspace_bytes < sp_compat_workspace_bytes(m) || reinterpret_cast<uintptr_t>(workspace) % 16 != 0)
            return invalid("[sp_compat_seeds] the workspace is smaller than sp_compat_workspace_bytes(m) or not 16-byte aligned");
    }
    hipStream_t st = as_stream(stream);
    if (seeds) {
        fill_i32_kernel<<<1, kBlock, 0, st>>>(seed_idx_out, (unsigned)seeds, -1);
        fill_i32_kernel<<<1, kBlock, 0, st>>>(reinterpret_cast<int32_t*>(seed_s_out), (unsigned)seeds, 0);
    }
    if (m < 3) {
        if (m && degree_out_opt) fill_i32_kernel<<<1, kBlock, 0, st>>>(reinterpret_cast<int32_t*>(degree_out_opt), (unsigned)m, 0);
        if (m && s_out_opt) fill_i32_kernel<<<1, kBlock, 0, st>>>(reinterpret_cast<int32_t*>(s_out_opt), (unsigned)m, 0);
        return launch_status();
    }
    const Plan p = plan(m);
    char* ws = static_cast<char*>(workspace);
    auto* c = reinterpret_cast<uint8_t*>(ws + p.c_off);
    auto* degree = reinterpret_cast<uint32_t*>(ws + p.degree_off);
    auto* s = reinterpret_cast<uint32_t*>(ws + p.s_off);
    const unsigned mp = (unsigned)p.mp;
    auto* rank = reinterpret_cast<uint32_t*>(ws + p.rank_off);
    if (const int rc = zero_async(degree, 12 * p.mp, st); rc != SP_OK) return rc;  // degree, s and rank lie side by side
    compat_kernel<<<dim3(div_up(mp / 4, kBlock), mp), kBlock, 0, st>>>(reinterpret_cast<const float4*>(cs), reinterpret_cast<const float4*>(ct),
                                                                      (unsigned)m, mp, tau * tau, min_edge * min_edge,
                                                                      reinterpret_cast<uint32_t*>(c), degree);
    second_order_kernel<<<dim3(mp / kPad, mp / kPad), kBlock, 0, st>>>(c, mp, s);
    seed_rank_kernel<<<dim3(div_up(m, kBlock), div_up(m, kRankChunk)), kBlock, 0, st>>>(s, (unsigned)m, rank);
    seed_scatter_kernel<<<div_up(m, kBlock), kBlock, 0, st>>>(s, degree, rank, (unsigned)m, (unsigned)seeds, seed_idx_out, seed_s_out,
                                                             degree_out_opt, s_out_opt);
    return launch_status();
}

extern "C" int sp_compat_consensus(size_t m, const int32_t* seed_idx, size_t seeds, size_t k, int32_t* cons_out, uint32_t* cons_s_out_opt,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (m > SP_COMPAT_MAX_MATCHES) return invalid("[sp_compat_consensus] more than SP_COMPAT_MAX_MATCHES (8192) matches");
    if (seeds > SP_COMPAT_MAX_SEEDS || k > SP_COMPAT_MAX_K)
        return invalid("[sp_compat_consensus] more than SP_COMPAT_MAX_SEEDS (256) seeds or SP_COMPAT_MAX_K (64) companions");
    if (seeds == 0 || k == 0) return SP_OK;
    if (!seed_idx || !cons_out) return invalid("[sp_compat_consensus] null argument (seed_idx, cons_out)");
    if (m >= 3) {
        if (!workspace) return invalid("[sp_compat_consensus] null argument (workspace)");
        if (workspace_bytes < sp_compat_workspace_bytes(m) || reinterpret_cast<uintptr_t>(workspace) % 16 != 0)
            return invalid("[sp_compat_consensus] the workspace is smaller than sp_compat_workspace_bytes(m) or not 16-byte aligned");
    }
    hipStream_t st = as_stream(stream);
    if (m < 3) {
        fill_i32_kernel<<<stream_grid(seeds * k), kBlock, 0, st>>>(cons_out, (unsigned)(seeds * k), -1);
        if (cons_s_out_opt) fill_i32_kernel<<<stream_grid(seeds * k), kBlock, 0, st>>>(reinterpret_cast<int32_t*>(cons_s_out_opt), (unsigned)(seeds * k), 0);
        return launch_status();
    }
    const Plan p = plan(m);
    char* ws = static_cast<char*>(workspace);
    const auto* c = reinterpret_cast<const uint8_t*>(ws + p.c_off);
    auto* rows = reinterpret_cast<uint32_t*>(ws + p.rows_off);
    const unsigned mp = (unsigned)p.mp;
    seed_rows_kernel<<<dim3(mp / kPad, div_up(seeds, 32)), kBlock, 0, st>>>(c, mp, seed_idx, (unsigned)seeds, (unsigned)m, rows);
    consensus_kernel<<<(unsigned)seeds, kBlock, 0, st>>>(rows, mp, (unsigned)m, seed_idx, (unsigned)k, cons_out, cons_s_out_opt);
    return launch_status();
}

extern "C" int sp_compat_seeds_host(const float* cs_host, const float* ct_host, size_t m, float tau, float min_edge, size_t seeds,
                                    int32_t* seed_idx_out, uint32_t* seed_s_out, uint32_t* degree_out_opt, uint32_t* s_out_opt) {
    using namespace sp;
    if (m > SP_COMPAT_MAX_MATCHES) return invalid("[sp_compat_seeds_host] more than SP_COMPAT_MAX_MATCHES (8192) matches");
    if (seeds > SP_COMPAT_MAX_SEEDS) return invalid("[sp_compat_seeds_host] more than SP_COMPAT_MAX_SEEDS (256) seeds");
    if (!(tau > 0.0f) || !(min_edge >= 0.0f) || !std::isfinite(tau) || !std::isfinite(min_edge))
        return invalid("[sp_compat_seeds_host] tau must be finite and > 0, min_edge finite and not negative");
    if (seeds && (!seed_idx_out || !seed_s_out)) return invalid("[sp_compat_seeds_host] null argument (seed_idx_out, seed_s_out)");
    if (m >= 3 && (!cs_host || !ct_host)) return invalid("[sp_compat_seeds_host] null argument (cs_host, ct_host)");
    for (size_t r = 0; r < seeds; ++r) seed_idx_out[r] = -1, seed_s_out[r] = 0u;
    if (m < 3) {
        for (size_t a = 0; a < m; ++a) {
            if (degree_out_opt) degree_out_opt[a] = 0u;
            if (s_out_opt) s_out_opt[a] = 0u;
        }
        return SP_OK;
    }
    const HostGraph g = host_graph(cs_host, ct_host, m, tau, min_edge);
    std::vector<uint32_t> s(m, 0u);
    for (size_t a = 0; a < m; ++a) {
        uint32_t degree = 0, sum = 0;
        for (size_t b = 0; b < m; ++b)
            if (g.at(a, b)) ++degree, sum += common_neighbours(g, a, b);
        s[a] = sum;
        if (degree_out_opt) degree_out_opt[a] = degree;
        if (s_out_opt) s_out_opt[a] = sum;
    }
    std::vector<uint32_t> order;
    for (size_t a = 0; a < m; ++a)
        if (s[a]) order.push_back((uint32_t)a);
    const size_t want = std::min(seeds, order.size());
    std::partial_sort(order.begin(), order.begin() + want, order.end(),
                      [&](uint32_t a, uint32_t b) { return s[a] != s[b] ? s[a] > s[b] : a < b; });
    for (size_t r = 0; r < want; ++r) seed_idx_out[r] = (int32_t)order[r], seed_s_out[r] = s[order[r]];
    return SP_OK;
}

extern "C" int sp_compat_consensus_host(const float* cs_host, const float* ct_host, size_t m, float tau, float min_edge,
                                        const int32_t* seed_idx, size_t seeds, size_t k, int32_t* cons_out, uint32_t* cons_s_out_opt) {
    using namespace sp;
    if (m > SP_COMPAT_MAX_MATCHES) return invalid("[sp_compat_consensus_host] more than SP_COMPAT_MAX_MATCHES (8192) matches");
    if (seeds > SP_COMPAT_MAX_SEEDS || k > SP_COMPAT_MAX_K)
        return invalid("[sp_compat_consensus_host] more than SP_COMPAT_MAX_SEEDS (256) seeds or SP_COMPAT_MAX_K (64) companions");
    if (!(tau > 0.0f) || !(min_edge >= 0.0f) || !std::isfinite(tau) || !std::isfinite(min_edge))
        return invalid("[sp_compat_consensus_host] tau must be finite and > 0, min_edge finite and not negative");
    if (seeds == 0 || k == 0) return SP_OK;
    if (!seed_idx || !cons_out) return invalid("[sp_compat_consensus_host] null argument (seed_idx, cons_out)");
    if (m >= 3 && (!cs_host || !ct_host)) return invalid("[sp_compat_consensus_host] null argument (cs_host, ct_host)");
    for (size_t i = 0; i < seeds * k; ++i) {
        cons_out[i] = -1;
        if (cons_s_out_opt) cons_s_out_opt[i] = 0u;
    }
    if (m < 3) return SP_OK;
    const HostGraph g = host_graph(cs_host, ct_host, m, tau, min_edge);
    std::vector<uint32_t> row(m), order;
    for (size_t r = 0; r < seeds; ++r) {
        const int32_t a = seed_idx[r];
        if (a < 0 || (size_t)a >= m) continue;
        order.clear();
        for (size_t b = 0; b < m; ++b) {
            row[b] = g.at((size_t)a, b) ? common_neighbours(g, (size_t)a, b) : 0u;
            if (row[b]) order.push_back((uint32_t)b);
        }
        const size_t want = std::min(k, order.size());
        std::partial_sort(order.begin(), order.begin() + want, order.end(),
                          [&](uint32_t x, uint32_t y) { return row[x] != row[y] ? row[x] > row[y] : x < y; });
        for (size_t i = 0; i < want; ++i) {
            cons_out[r * k + i] = (int32_t)order[i];
            if (cons_s_out_opt) cons_s_out_opt[r * k + i] = row[order[i]];
        }
    }
    return SP_OK;
}

extern "C" int sp_compat_poses_host(const float* cs_host, const float* ct_host, size_t m, const int32_t* seed_idx, const int32_t* cons,
                                    size_t seeds, size_t k, double* poses_out, uint32_t* rank_out_opt, size_t* count_out) {
    using namespace sp;
    if (!count_out) return invalid("[sp_compat_poses_host] null argument (count_out)");
    *count_out = 0;
    if (m > SP_COMPAT_MAX_MATCHES) return invalid("[sp_compat_poses_host] more than SP_COMPAT_MAX_MATCHES (8192) matches");
    if (seeds > SP_COMPAT_MAX_SEEDS || k > SP_COMPAT_MAX_K)
        return invalid("[sp_compat_poses_host] more than SP_COMPAT_MAX_SEEDS (256) seeds or SP_COMPAT_MAX_K (64) companions");
    if (seeds == 0 || k < 2 || m < 3) return SP_OK;
    if (!cs_host || !ct_host || !seed_idx || !cons || !poses_out) return invalid("[sp_compat_poses_host] null argument");
    std::vector<double> ps, pt;
    size_t written = 0;
    for (size_t r = 0; r < seeds; ++r) {
        const int32_t a = seed_idx[r];
        if (a < 0 || (size_t)a >= m) continue;
        ps.clear(), pt.clear();
        auto push = [&](size_t i) {
            for (int d = 0; d < 3; ++d) ps.push_back((double)cs_host[4 * i + d]), pt.push_back((double)ct_host[4 * i + d]);
        };
        push((size_t)a);
        for (size_t i = 0; i < k; ++i) {
            const int32_t b = cons[r * k + i];
            if (b >= 0 && (size_t)b < m && b != a) push((size_t)b);
        }
        if (ps.size() < 9) continue;  // fewer than two companions
        if (!horn_pose(ps, pt, poses_out + 16 * written)) continue;
        if (rank_out_opt) rank_out_opt[written] = (uint32_t)r;
        ++written;
    }
    *count_out = written;
    return SP_OK;
}

extern "C" int sp_pose_score(const float* cs, const float* ct, size_t m, const float* poses, size_t count, float inlier_distance,
                             uint32_t* score_out, void* stream) {
    using namespace sp;
    if (count > SP_RANSAC_MAX_HYPOTHESES || m >= ((size_t)1 << 31))
        return invalid("[sp_pose_score] more than SP_RANSAC_MAX_HYPOTHESES (2^20) poses or 2^31 matches");
    if (count == 0) return SP_OK;
    if (!score_out || !poses || (m && (!cs || !ct))) return invalid("[sp_pose_score] null argument");
    if (!(inlier_distance >= 0.0f)) return invalid("[sp_pose_score] inlier_distance must not be negative");
    hipStream_t st = as_stream(stream);
    if (const int rc = zero_async(score_out, 4 * count, st); rc != SP_OK) return rc;
    if (m == 0) return SP_OK;
    const unsigned pose_blocks = div_up(count, kBlock), tiles = div_up(m, kScoreTile);
    const unsigned chunks = std::max(1u, std::min(tiles, (2u * kNumCU + pose_blocks - 1) / pose_blocks));  // two workgroups per CU when the poses are few
    const unsigned tiles_per_block = (tiles + chunks - 1) / chunks;
    pose_score_kernel<<<dim3(pose_blocks, div_up(tiles, tiles_per_block)), kBlock, 0, st>>>(
        reinterpret_cast<const float4*>(cs), reinterpret_cast<const float4*>(ct), (unsigned)m, poses, (unsigned)count,
        inlier_distance * inlier_distance, tiles_per_block, score_out);
    return launch_status();
}

extern "C" int sp_compat_select_host(const uint32_t* scores_host, const double* poses_in, const uint32_t* rank_in_opt, size_t count,
                                     size_t guesses, double* poses_out, uint32_t* rank_out_opt, size_t* count_out) {
    using namespace sp;
    if (!count_out) return invalid("[sp_compat_select_host] null argument (count_out)");
    *count_out = 0;
    if (count > SP_RANSAC_MAX_HYPOTHESES) return invalid("[sp_compat_select_host] more than SP_RANSAC_MAX_HYPOTHESES (2^20) poses");
    if (count == 0 || guesses == 0) return SP_OK;
    if (!scores_host || !poses_in || !poses_out) return invalid("[sp_compat_select_host] null argument");
    std::vector<uint32_t> order;
    for (size_t p = 0; p < count; ++p)
        if (scores_host[p]) order.push_back((uint32_t)p);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return scores_host[a] > scores_host[b]; });
    const size_t want = std::min(guesses, order.size());
    for (size_t g = 0; g < want; ++g) {
        std::memcpy(poses_out + 16 * g, poses_in + 16 * (size_t)order[g], 16 * sizeof(double));
        if (rank_out_opt) rank_out_opt[g] = rank_in_opt ? rank_in_opt[order[g]] : order[g];
    }
    *count_out = want;
    return SP_OK;
}
