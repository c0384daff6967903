// Weighted and mixed random sampling on the device: PreprocessFilter::weighted_random_sampling / mixed_random_sampling
// (filter/preprocess_operator/weighted_sampling_operator.hpp:29-95, mixed_random_sampling_operator.hpp:28-105). The reference
// walks every point on the host: one std::log, one std::mt19937 draw and one std::priority_queue step per positive weight, then
// a host pass over all flags. Only the generator is sequential; here the host draws, and everything else runs on the device:
//   sp_weight_check           one pass over the weights: the number of positive ones and the lowest index of one that is not
//                             finite or below 0 (the reference's checks, :43-61 / :57-62) — the one read-back of a sampling call.
//   sp_weighted_sample_flags  Efraimidis-Spirakis: the j-th positive weight (a prefix count gives j) takes the caller's draw
//                             u_by_rank[j]; key = log(u) / w; the m largest keys are kept. A radix SELECT, not a sort: the keys
//                             become order-preserving u32 and the m-th largest, K, is narrowed one 8-bit digit at a time; the
//                             first histogram comes from the kernel that makes the keys, three read-only passes follow, then one
//                             flag pass. 9 launches, 4 B of scratch per point (the key).
//   sp_uniform_fill_flags     the uniform part of the mixed sampler: the host runs the partial Fisher-Yates on POSITIONS in the
//                             list of points not selected so far; the device sets the flag of the p-th such point.
// Rules pinned to the reference:
//   key       std::log(u) / w in binary32 (:75 / :65). The logarithm here is the double logarithm rounded to float (correctly
//             rounded but for draws within 2^-29 of a rounding boundary), the division is IEEE (-fno-fast-math, the compiler's
//             correctly rounded sequence). glibc's logf is within 0.82 ulp, so a key differs from the reference's by at most
//             2 ulp. Keys are <= 0, may be -inf (a tiny w) and -0 (a huge w): -0 is made +0 before the mapping,
//             because the heap compares floats and -0 < +0 is false.
//   ties      the reference's min-heap of (key, index) replaces its top only when top.key < key (:81 / :71). With K the m-th
//             largest key, g = #{key > K} and c = m - g: every key above K is kept; of the points with key == K, those among the
//             first m points (index order) with key >= K are candidates, and the c candidates with the HIGHEST indices are kept
//             (until m such points have arrived everything enters the heap; afterwards ties are refused and each later key
//             above K evicts the tie with the lowest index). c == #{key == K} (no surplus tie, nearly always) needs none of
//             this: the flag pass alone decides, and the two tie launches return at once.
//   few       fewer positive weights than m (the mixed sampler, :66-69): every positive weight is kept.
#include <algorithm>
#include <cmath>

#include "sp_common.h"
#include "sp_internal.h"
#include "sp_spatial.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

constexpr int kSampBlock = 256;
constexpr int kSampPer = 4;                               // consecutive points per lane
constexpr unsigned kSampTile = kSampBlock * kSampPer;     // 1024 points per workgroup
constexpr int kScanBlock = 1024;                          // the one workgroup that scans the per-tile counts
constexpr unsigned kHistGrid = kNumCU * 4;                // grid cap of the read-only histogram passes

// workspace of sp_weighted_sample_flags: SelState | hist[4][256] | pos[T + 1] | ge[T + 1] | eq[T + 1] | keys[n]
struct SelLevel {
    unsigned prefix;  // the digits of K settled so far (right-aligned)
    unsigned r;       // K is the r-th largest of the keys that start with prefix
    unsigned all;     // 1: fewer than m keys in all — every one is kept
    unsigned count;   // keys that start with prefix
};
struct SelState {
    SelLevel level[4];  // level[3]: prefix = K, r = c, count = #{key == K}
    unsigned ties;      // 1: c < #{key == K}: the tie rule decides (sample_ties_kernel)
};
constexpr size_t kHistOffset = 256;
constexpr size_t kTilesOffset = kHistOffset + 4 * 256 * sizeof(unsigned);

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t tile_array_bytes(size_t n) { return align256(((n + kSampTile - 1) / kSampTile + 1) * sizeof(unsigned)); }

// Exclusive prefix sum over the workgroup (BLOCK lanes, all active); total = the sum. s_wave: BLOCK / 64 words of LDS.
template <int BLOCK>
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* s_wave, unsigned& total) {
    const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off *= 2) {
        const unsigned y = __shfl_up(incl, off, kWave);
        if (lane >= (unsigned)off) incl += y;
    }
    __syncthreads();  // (s_wave may still be read from the previous call)
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    unsigned base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / kWave; ++w) {
        const unsigned s = s_wave[w];
        if ((unsigned)w < wave) base += s;
        sum += s;
    }
    total = sum;
    return base + incl - v;
}

// Four consecutive values of a tile: one 16-byte load where the array allows it (tiles start at multiples of 1024 elements, so
// the alignment is the pointer's: uniform over the launch), else element by element; `fill` past n.
template <typename T>
__device__ __forceinline__ void load4(const T* __restrict__ a, size_t i, size_t n, T fill, T (&v)[4]) {
    static_assert(sizeof(T) == 4, "");
    if (i + 3 < n && (reinterpret_cast<uintptr_t>(a) & 15u) == 0) {
        const uint4 q = *reinterpret_cast<const uint4*>(a + i);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) __builtin_memcpy(&v[k], &w[k], 4);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i + k < n ? a[i + k] : fill;
    }
}

// Order-preserving u32 of a key (<= 0, never NaN); 0 is kept for "no key" (the smallest key, -inf, maps to 0x007fffff).
__device__ __forceinline__ unsigned key_bits(float key) {
    key += 0.0f;  // -0 -> +0 (the reference's heap compares floats)
    return ordered_bits(key);
}

// ------------------------------------------------------------------------------------------------------------ weight check
__global__ void weight_report_init_kernel(unsigned* __restrict__ report) {
    report[0] = 0u;
    report[1] = 0xffffffffu;
}

__global__ __launch_bounds__(kSampBlock) void weight_check_kernel(const float* __restrict__ w, size_t n, unsigned* report) {
    __shared__ unsigned s_pos[kSampBlock / kWave], s_bad[kSampBlock / kWave];
    unsigned pos = 0, bad = 0xffffffffu;
    const size_t stride = (size_t)gridDim.x * kSampTile;
    for (size_t i = ((size_t)blockIdx.x * kSampBlock + threadIdx.x) * kSampPer; i < n; i += stride) {
        float v[4];
        load4(w, i, n, 0.0f, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // !isfinite(w) || w < 0 (weighted_sampling_operator.hpp:45): NaN fails the first comparison
            if (!(fabsf(v[k]) <= 3.402823466e+38f) || v[k] < 0.0f) bad = min(bad, (unsigned)(i + k));
            pos += v[k] > 0.0f ? 1u : 0u;
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off /= 2) {
        pos += __shfl_down(pos, off, kWave);
        bad = min(bad, (unsigned)__shfl_down(bad, off, kWave));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) { s_pos[threadIdx.x / kWave] = pos; s_bad[threadIdx.x / kWave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < kSampBlock / kWave; ++v) { pos += s_pos[v]; bad = min(bad, s_bad[v]); }
        if (pos) atomicAdd(report, pos);
        if (bad != 0xffffffffu) atomicMin(report + 1, bad);
    }
}

// --------------------------------------------------------------------------------------------------------- per-tile counts
// counts[tile] = positive weights of the tile; workgroup 0 also clears the four histograms of the select.
__global__ __launch_bounds__(kSampBlock) void sample_count_pos_kernel(const float* __restrict__ w, size_t n,
                                                                      unsigned* __restrict__ counts, unsigned* __restrict__ hist) {
    __shared__ unsigned s_wave[kSampBlock / kWave];
    if (blockIdx.x == 0)
        for (int k = 0; k < 4; ++k) hist[k * 256 + threadIdx.x] = 0u;
    float v[4];
    load4(w, (size_t)blockIdx.x * kSampTile + threadIdx.x * kSampPer, n, 0.0f, v);
    unsigned c = 0, total;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += v[k] > 0.0f ? 1u : 0u;
    block_excl_scan<kSampBlock>(c, s_wave, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[tile] = points of the tile whose flag is not INCLUDE (1)
__global__ __launch_bounds__(kSampBlock) void sample_count_unflagged_kernel(const uint8_t* __restrict__ flags, size_t n,
                                                                            unsigned* __restrict__ counts) {
    __shared__ unsigned s_wave[kSampBlock / kWave];
    const size_t i = (size_t)blockIdx.x * kSampTile + threadIdx.x * kSampPer;
    unsigned c = 0, total;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += (i + k < n && flags[i + k] != 1) ? 1u : 0u;
    block_excl_scan<kSampBlock>(c, s_wave, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// In place: a[t] = a[0] + .. + a[t - 1] for t < T, a[T] = the total, for a0 and (optional) a1, by ONE workgroup: T = n / 1024
// entries (68 at 70 k points, 1024 at 1 M). Totals up to 2^32 - 1 (sp::exclusive_scan_u32's look-back words stop at 2^30 and
// cost two launches). The workgroup walks the counts 1024 at a time, one after the other: one step at 1 M points, 4096 steps
// near n = 2^32 (milliseconds, up to three times per call) — fine at the sizes in use, not meant for 10^9 points. gate
// (optional): nothing to do when *gate == 0.
__global__ __launch_bounds__(kScanBlock) void sample_tile_scan_kernel(unsigned* a0, unsigned* a1, unsigned T, const unsigned* gate) {
    __shared__ unsigned s_wave[kScanBlock / kWave];
    if (gate && *gate == 0u) return;  // (uniform)
    for (int which = 0; which < 2; ++which) {
        unsigned* const a = which ? a1 : a0;
        if (!a) continue;
        unsigned carry = 0;
        for (unsigned base = 0; base < T; base += kScanBlock) {
            const unsigned i = base + threadIdx.x;
            const unsigned v = i < T ? a[i] : 0u;
            unsigned total;
            const unsigned ex = block_excl_scan<kScanBlock>(v, s_wave, total);
            if (i < T) a[i] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) a[T] = carry;
    }
}

// ------------------------------------------------------------------------------------------------------------ radix select
// One digit of K from the histogram of that digit over the keys that start with `in.prefix`: the digit d with
// #{digit > d} < in.r <= #{digit >= d}. 256 lanes, all call it; s: 258 words of LDS. The same result in every workgroup.
__device__ __forceinline__ SelLevel select_digit(const unsigned* __restrict__ hist, SelLevel in, unsigned* s) {
    const unsigned t = threadIdx.x;
    s[t] = hist[t];
    if (t == 0) s[256] = 0xffffffffu;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < 256; off *= 2) {  // suffix sums
        const unsigned v = t + off < 256 ? s[t + off] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    const unsigned ge = s[t], gt = t < 255 ? s[t + 1] : 0u;
    if (!in.all && gt < in.r && in.r <= ge) { s[256] = t; s[257] = gt; }
    __syncthreads();
    SelLevel out;
    const unsigned d = s[256];
    if (d == 0xffffffffu) {  // fewer keys than r (level 0 only), or all already
        out.prefix = 0u; out.r = 0u; out.all = 1u; out.count = 0u;
    } else {
        out.prefix = (in.prefix << 8) | d;
        out.r = in.r - s[257];
        out.all = 0u;
        out.count = s[d] - s[257];
    }
    __syncthreads();  // (s is reused by the caller)
    return out;
}

__device__ __forceinline__ void hist_flush(const unsigned* s_hist, unsigned* __restrict__ hist) {
    __syncthreads();
    const unsigned c = s_hist[threadIdx.x];
    if (c) atomicAdd(hist + threadIdx.x, c);
}

// The keys, and the histogram of their top digit. The j-th positive weight of the cloud takes u_by_rank[j]: j = the tile's base
// (the scanned counts) + the rank within the tile.
__global__ __launch_bounds__(kSampBlock) void sample_keys_kernel(const float* __restrict__ w, const float* __restrict__ u_by_rank,
                                                                 size_t n, const unsigned* __restrict__ pos_base,
                                                                 unsigned* __restrict__ keys, unsigned* __restrict__ hist0) {
    __shared__ unsigned s_wave[kSampBlock / kWave];
    __shared__ unsigned s_hist[256];
    s_hist[threadIdx.x] = 0u;
    const size_t i = (size_t)blockIdx.x * kSampTile + threadIdx.x * kSampPer;
    float v[4];
    load4(w, i, n, 0.0f, v);
    unsigned c = 0, total;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += v[k] > 0.0f ? 1u : 0u;
    unsigned rank = pos_base[blockIdx.x] + block_excl_scan<kSampBlock>(c, s_wave, total);  // (its barriers order s_hist's zeroing)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned key = 0u;
        if (v[k] > 0.0f) {
            const float u = u_by_rank[rank++];
            key = key_bits((float)log((double)u) / v[k]);
            atomicAdd(&s_hist[key >> 24], 1u);
        }
        if (i + k < n) keys[i + k] = key;
    }
    hist_flush(s_hist, hist0);
}

// Level L = 1, 2, 3: settles digit L - 1 of K from the previous histogram, then counts digit L of the keys that start with the
// settled digits. Read-only over the keys.
__global__ __launch_bounds__(kSampBlock) void sample_hist_kernel(const unsigned* __restrict__ keys, size_t n, unsigned m, int L,
                                                                 SelState* state, unsigned* hist) {
    __shared__ unsigned s_hist[258];
    SelLevel in;
    if (L == 1) { in.prefix = 0u; in.r = m; in.all = 0u; in.count = 0u; }
    else in = state->level[L - 2];
    const SelLevel lv = select_digit(hist + (L - 1) * 256, in, s_hist);
    if (blockIdx.x == 0 && threadIdx.x == 0) state->level[L - 1] = lv;
    if (lv.all) return;  // (uniform over the launch)
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 32 - 8 * L;
    const size_t stride = (size_t)gridDim.x * kSampTile;
    for (size_t i = ((size_t)blockIdx.x * kSampBlock + threadIdx.x) * kSampPer; i < n; i += stride) {
        unsigned k4[4];
        load4(keys, i, n, 0u, k4);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((k4[k] >> shift) == lv.prefix && k4[k] != 0u) atomicAdd(&s_hist[(k4[k] >> (shift - 8)) & 255u], 1u);
    }
    hist_flush(s_hist, hist + L * 256);
}

// Settles the last digit (K, c), then flags: key > K is kept; key == K is kept when there is no surplus tie, and left to
// sample_ties_kernel (with the per-tile counts of key >= K and key == K) when there is.
__global__ __launch_bounds__(kSampBlock) void sample_flags_kernel(const unsigned* __restrict__ keys, size_t n, unsigned m,
                                                                  SelState* state, const unsigned* hist,
                                                                  const unsigned* __restrict__ pos_total, uint8_t* __restrict__ flags,
                                                                  unsigned* __restrict__ ge_cnt, unsigned* __restrict__ eq_cnt,
                                                                  unsigned* __restrict__ selected_count) {
    __shared__ unsigned s[258];
    const SelLevel lv = select_digit(hist + 3 * 256, state->level[2], s);
    const unsigned K = lv.prefix;  // (0 with lv.all: every key is above it, and "no key" equals it)
    const bool ties = !lv.all && lv.r < lv.count;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state->level[3] = lv;
        state->ties = ties ? 1u : 0u;
        if (selected_count) *selected_count = lv.all ? *pos_total : m;
    }
    const size_t i = (size_t)blockIdx.x * kSampTile + threadIdx.x * kSampPer;
    unsigned k4[4];
    load4(keys, i, n, 0u, k4);
    unsigned packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool gt = k4[k] > K, eq = k4[k] == K && !lv.all;
        if (i + k < n) flags[i + k] = (gt || (eq && !ties)) ? 1 : 0;
        packed += (gt || eq ? 1u : 0u) | (eq ? 0x10000u : 0u);
    }
    if (!ties) return;  // (uniform over the launch)
    unsigned total;
    block_excl_scan<kSampBlock>(packed, s, total);
    if (threadIdx.x == 0) { ge_cnt[blockIdx.x] = total & 0xffffu; eq_cnt[blockIdx.x] = total >> 16; }
}

// Per lane: the exclusive ranks, within the tile, of its four keys among the keys >= K (low half) and == K (high half).
__device__ __forceinline__ unsigned tile_tie_ranks(const unsigned (&k4)[4], unsigned K, unsigned* s_wave) {
    unsigned packed = 0, total;
#pragma unroll
    for (int k = 0; k < 4; ++k) packed += (k4[k] >= K ? 1u : 0u) | (k4[k] == K ? 0x10000u : 0u);
    return block_excl_scan<kSampBlock>(packed, s_wave, total);
}

// The tie rule, when it decides (state->ties). E = the ties among the first m keys >= K: the workgroup finds the tile that holds
// the m-th such key from the scanned counts, ranks that tile, and reads E off the m-th key. A tie is kept when its rank among
// the ties lies in [E - c, E).
__global__ __launch_bounds__(kSampBlock) void sample_ties_kernel(const unsigned* __restrict__ keys, size_t n, unsigned m, unsigned T,
                                                                 const SelState* __restrict__ state,
                                                                 const unsigned* __restrict__ ge_base,
                                                                 const unsigned* __restrict__ eq_base, uint8_t* __restrict__ flags) {
    __shared__ unsigned s_wave[kSampBlock / kWave];
    __shared__ unsigned s_E;
    if (state->ties == 0u) return;  // (uniform)
    const unsigned K = state->level[3].prefix, c = state->level[3].r;
    unsigned lo = 0, hi = T;  // the last tile whose base is <= m - 1 (ge_base[T] = the total >= m)
    while (hi - lo > 1) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (ge_base[mid] <= m - 1) lo = mid; else hi = mid;
    }
    unsigned k4[4];
    {
        const size_t i = (size_t)lo * kSampTile + threadIdx.x * kSampPer;
        load4(keys, i, n, 0u, k4);
        unsigned r = tile_tie_ranks(k4, K, s_wave);
        unsigned ge = ge_base[lo] + (r & 0xffffu), eq = eq_base[lo] + (r >> 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k4[k] >= K) {
                if (ge == m - 1) s_E = eq + (k4[k] == K ? 1u : 0u);
                ++ge;
                if (k4[k] == K) ++eq;
            }
        }
    }
    __syncthreads();
    const unsigned E = s_E;
    const size_t i = (size_t)blockIdx.x * kSampTile + threadIdx.x * kSampPer;
    load4(keys, i, n, 0u, k4);
    unsigned eq = eq_base[blockIdx.x] + (tile_tie_ranks(k4, K, s_wave) >> 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k4[k] == K) {
            if (i + k < n && eq + c >= E && eq < E) flags[i + k] = 1;
            ++eq;
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- uniform fill
// The p-th point not flagged so far (p in positions, ascending) becomes INCLUDE. A tile whose range of ranks holds no position
// reads two words and leaves.
__global__ __launch_bounds__(kSampBlock) void sample_uniform_fill_kernel(uint8_t* __restrict__ flags, size_t n,
                                                                         const unsigned* __restrict__ base,
                                                                         const uint32_t* __restrict__ positions, unsigned P) {
    __shared__ unsigned s_wave[kSampBlock / kWave];
    const unsigned r0 = base[blockIdx.x], r1 = base[blockIdx.x + 1];
    if (r0 == r1) return;
    unsigned lo = 0, hi = P;  // the first position >= r0
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (positions[mid] < r0) lo = mid + 1; else hi = mid;
    }
    if (lo == P || positions[lo] >= r1) return;  // (uniform over the workgroup)
    const unsigned first = lo;
    const size_t i = (size_t)blockIdx.x * kSampTile + threadIdx.x * kSampPer;
    bool open[4];
    unsigned c = 0, total;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        open[k] = i + k < n && flags[i + k] != 1;
        c += open[k] ? 1u : 0u;
    }
    unsigned rank = r0 + block_excl_scan<kSampBlock>(c, s_wave, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!open[k]) continue;
        unsigned a = first, b = P;  // is `rank` among the positions?
        while (a < b) {
            const unsigned mid = a + (b - a) / 2;
            if (positions[mid] < rank) a = mid + 1; else b = mid;
        }
        if (a < P && positions[a] == rank) flags[i + k] = 1;
        ++rank;
    }
}

void invalid(const char* msg) { sp_set_error(msg); }

}  // namespace
}  // namespace sp

extern "C" int sp_weight_check(const float* weights, size_t n, uint32_t* report_dev, void* stream) {
    if (!weights || !report_dev || n == 0 || n >= ((size_t)1 << 32)) {
        sp::invalid("[sp_weight_check] invalid argument (a null pointer, n == 0 or n >= 2^32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = sp::as_stream(stream);
    sp::weight_report_init_kernel<<<1, 1, 0, st>>>(report_dev);
    const unsigned grid = std::min<unsigned>(sp::div_up(n, sp::kSampTile), sp::kHistGrid);
    sp::weight_check_kernel<<<grid, sp::kSampBlock, 0, st>>>(weights, n, report_dev);
    return sp::launch_status();
}

extern "C" size_t sp_weighted_sample_workspace_bytes(size_t n) {
    return sp::kTilesOffset + 3 * sp::tile_array_bytes(n) + sp::align256(n * sizeof(uint32_t));
}

extern "C" int sp_weighted_sample_flags(const float* weights, const float* u_by_rank, size_t n, size_t m, uint8_t* flags_out,
                                        uint32_t* selected_count_dev_opt, void* workspace, size_t workspace_bytes, void* stream) {
    if (!weights || !u_by_rank || !flags_out || !workspace || n == 0 || n >= ((size_t)1 << 32) || m == 0 || m > n ||
        workspace_bytes < sp_weighted_sample_workspace_bytes(n)) {
        sp::invalid("[sp_weighted_sample_flags] invalid argument (a null pointer, n == 0 or >= 2^32, m == 0 or > n, or a workspace "
                    "smaller than sp_weighted_sample_workspace_bytes)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    using namespace sp;
    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    SelState* state = reinterpret_cast<SelState*>(ws);
    unsigned* hist = reinterpret_cast<unsigned*>(ws + kHistOffset);
    const size_t tb = tile_array_bytes(n);
    unsigned* pos = reinterpret_cast<unsigned*>(ws + kTilesOffset);
    unsigned* ge = reinterpret_cast<unsigned*>(ws + kTilesOffset + tb);
    unsigned* eq = reinterpret_cast<unsigned*>(ws + kTilesOffset + 2 * tb);
    unsigned* keys = reinterpret_cast<unsigned*>(ws + kTilesOffset + 3 * tb);
    const unsigned T = div_up(n, kSampTile), M = (unsigned)m;
    const unsigned hgrid = std::min<unsigned>(T, kHistGrid);
    sample_count_pos_kernel<<<T, kSampBlock, 0, st>>>(weights, n, pos, hist);
    sample_tile_scan_kernel<<<1, kScanBlock, 0, st>>>(pos, nullptr, T, nullptr);
    sample_keys_kernel<<<T, kSampBlock, 0, st>>>(weights, u_by_rank, n, pos, keys, hist);
    for (int L = 1; L <= 3; ++L) sample_hist_kernel<<<hgrid, kSampBlock, 0, st>>>(keys, n, M, L, state, hist);
    sample_flags_kernel<<<T, kSampBlock, 0, st>>>(keys, n, M, state, hist, pos + T, flags_out, ge, eq, selected_count_dev_opt);
    sample_tile_scan_kernel<<<1, kScanBlock, 0, st>>>(ge, eq, T, &state->ties);
    sample_ties_kernel<<<T, kSampBlock, 0, st>>>(keys, n, M, T, state, ge, eq, flags_out);
    return launch_status();
}

extern "C" size_t sp_uniform_fill_workspace_bytes(size_t n) { return sp::tile_array_bytes(n); }

extern "C" int sp_uniform_fill_flags(uint8_t* flags, size_t n, const uint32_t* positions_sorted, size_t n_positions, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (!flags || !positions_sorted || !workspace || n == 0 || n >= ((size_t)1 << 32) || n_positions == 0 || n_positions > n ||
        workspace_bytes < sp_uniform_fill_workspace_bytes(n)) {
        sp::invalid("[sp_uniform_fill_flags] invalid argument (a null pointer, n == 0 or >= 2^32, n_positions == 0 or > n, or a "
                    "workspace smaller than sp_uniform_fill_workspace_bytes)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    using namespace sp;
    hipStream_t st = as_stream(stream);
    unsigned* base = static_cast<unsigned*>(workspace);
    const unsigned T = div_up(n, kSampTile);
    sample_count_unflagged_kernel<<<T, kSampBlock, 0, st>>>(flags, n, base);
    sample_tile_scan_kernel<<<1, kScanBlock, 0, st>>>(base, nullptr, T, nullptr);
    sample_uniform_fill_kernel<<<T, kSampBlock, 0, st>>>(flags, n, base, positions_sorted, (unsigned)n_positions);
    return launch_status();
}
