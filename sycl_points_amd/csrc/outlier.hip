// The two outlier filters and the intensity z-score, for gfx950: what is left of the reference's algorithms/filter/ after
// scan_refine.hip.
//   sp_outlier_statistical_flags  OutlierRemoval::statistical's three kernels (filter/outlier_removal_filter.hpp:38-145)
//   sp_outlier_radius_flags       OutlierRemoval::radius's kernel             (filter/outlier_removal_filter.hpp:155-199)
//   sp_intensity_zscore           intensity_zscore::kernel::compute           (filter/intensity_zscore.hpp:17-32)
// All read a KNNResult that is already on the device: rows of k_stride entries, ascending SQUARED distances padded with FLT_MAX,
// indices padded with -1. The reference sums and compares the squared distances as they are, and so does this file.
//
// Statistical filter: three plain launches on one stream, no host round trip (the reference waits after each of its three and
// reads a USM word in between), no persistent kernel, no arrival counter, no float atomic.
//   A  mean_kernel      m[i] = (d2[i][0] + ... + d2[i][k_use-1]) / float(k_use), summed in index order (:78-84). A workgroup takes a
//                       tile of `rows` consecutive rows (256, or fewer when 256 rows do not fit 32 KB of LDS), i.e. rows * k_stride
//                       CONSECUTIVE floats: they are fetched as contiguous 16-byte loads (4-byte ones when the array is not 16-byte
//                       aligned) into LDS, and lane t then sums row t out of LDS. No lane walks a strided row in HBM. A row with
//                       FLT_MAX padding sums to inf or to a huge finite value, exactly as the reference's would: kept literal.
//                       Each workgroup leaves ONE partial sum of its m[i]: per lane in tile order, then DPP inside the wave, then
//                       the four wave totals in wave order.
//   B  variance_kernel  every workgroup sums A's partials in one fixed order (lane t takes partials t, t+256, ...; DPP; wave
//                       order), g = sum / float(n) (:102), and leaves its partial of (g - m[i])^2 (:110-111) the same way.
//   C  flags_kernel     every workgroup sums B's partials in that order, thr = g + mul * sqrt(var_sum / float(n)) (:126-128),
//                       flags[i] = m[i] > thr ? 0 : 1 (:134). Workgroup 0 stores stats_out = {g, var_sum / n, thr, float(n)}.
// At most kMaxParts = 1024 workgroups per launch (grid-stride loops), so that the next launch reads all partials in one batch of
// four loads per lane. The order of every sum depends on n and k_stride only: two calls on the same input give the same bits in
// m, stats_out and flags. (The reference's two sycl::reduction sums have no specified order.)
// Algorithmic bytes per point: A reads 4 k_stride and writes 4 (+ 4 per 256 points of partials), B reads 4, C reads 4 and writes
// 1: 4 k_stride + 13 in all, 53 at k = 10 (8.4 us per 1M points at the 6.29 TB/s copy rate), 93 at k = 20.
//
// Radius filter: one launch, flags[i] = d2[i][column] > radius ? 0 : 1 — the SQUARED distance against the radius itself, as the
// reference compares them (:178-188). One 4-byte read per lane at a stride of 4 k_stride bytes: with
// 4 k_stride <= 128 every 128-byte line of the array is touched, so the bound is the whole array, 4 k_stride + 1 bytes per point.
//
// Intensity z-score: one launch, one lane per point, scan_refine.hip's gather: the index row is contiguous per lane (16-byte words
// when k_stride is a multiple of 4), the k_use neighbour intensities are random 4-byte reads out of L2 / Infinity Cache.
// sum I and sum I^2 in index order, mean = sum I / kf, var = fmax(sum I^2 / kf - mean * mean, 0), sigma = sqrt(var), result 0 when
// sigma < sigma_min, else (I[i] - mean) / sigma. A neighbour index outside [0, n) contributes nothing and the divisor stays k_use
// (sp_intensity_gaussian's precedent, DESIGN.md section 7: one unsigned compare, never a wild read). Bytes per point:
// 4 k_stride (index row) + 4 k_use (gathered) + 4 (own) + 4 (store): 88 at k = 10.
//
// Compiled with -ffp-contract=off: every product and sum here is one rounding; sqrt and division are correctly rounded.
#include <cmath>
#include <cstdio>

#include "sp_common.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

constexpr unsigned kMaxParts = 1024;        // workgroups per launch of the statistical filter = partial sums the next one reads
constexpr unsigned kTileFloats = 8192;      // LDS of mean_kernel: 32 KB
constexpr size_t kMaxStride = kTileFloats / 4;  // a tile holds at least 4 rows
// workspace: A's partials, B's partials, g
constexpr size_t kWsFloats = 2 * kMaxParts + 4;
constexpr size_t kMaxPoints = (size_t)1 << 31;  // the grid-stride loops count in 32 bits, neighbour indices are int32

// The workgroup's sum of v, in every lane: DPP inside each wave, then the four wave totals added in wave order.
__device__ __forceinline__ float block_sum(float v, float* wave_totals /* kBlock / kWave floats of LDS */) {
    const float w = wave_sum_to_lane63(v);
    __syncthreads();  // (the caller may have read wave_totals of an earlier sum)
    if ((threadIdx.x & (kWave - 1)) == kWave - 1) wave_totals[threadIdx.x / kWave] = w;
    __syncthreads();
    float s = wave_totals[0];
#pragma unroll
    for (int i = 1; i < kBlock / kWave; ++i) s += wave_totals[i];
    return s;
}

// The sum of parts[0 .. count), count <= kMaxParts, in one order for every workgroup: lane t adds parts t, t + 256, t + 512,
// t + 768, then block_sum.
__device__ __forceinline__ float sum_parts(const float* __restrict__ parts, unsigned count, float* wave_totals) {
    float v = 0.0f;
#pragma unroll
    for (unsigned j = 0; j < kMaxParts / kBlock; ++j) {
        const unsigned p = j * kBlock + threadIdx.x;
        v += p < count ? parts[p] : 0.0f;
    }
    return block_sum(v, wave_totals);
}

template <bool VEC16>  // the array is 16-byte aligned (every tile then starts on a 16-byte boundary: rows is a multiple of 4)
__global__ __launch_bounds__(kBlock) void mean_kernel(const float* __restrict__ d2, unsigned n, unsigned k_stride, unsigned k_use,
                                                      unsigned rows, float* __restrict__ mean_out, float* __restrict__ parts) {
    __shared__ __attribute__((aligned(16))) float tile[kTileFloats];
    __shared__ float wave_totals[kBlock / kWave];
    const float kf = (float)k_use;
    float acc = 0.0f;
    const unsigned tiles = (n + rows - 1) / rows;
    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        const unsigned row0 = t * rows;
        const unsigned here = min(rows, n - row0);
        const unsigned count = here * k_stride;  // <= kTileFloats
        const float* __restrict__ src = d2 + (size_t)row0 * k_stride;
        __syncthreads();  // (the sums of the tile before are done)
        if (VEC16) {
            const unsigned quads = count >> 2;
            for (unsigned q = threadIdx.x; q < quads; q += kBlock)
                reinterpret_cast<float4*>(tile)[q] = reinterpret_cast<const float4*>(src)[q];
            for (unsigned e = (quads << 2) + threadIdx.x; e < count; e += kBlock) tile[e] = src[e];  // (the cloud's last tile)
        } else {
            for (unsigned e = threadIdx.x; e < count; e += kBlock) tile[e] = src[e];
        }
        __syncthreads();
        if (threadIdx.x < here) {
            const float* row = tile + threadIdx.x * k_stride;
            float sum = 0.0f;
            for (unsigned j = 0; j < k_use; ++j) sum += row[j];
            const float m = sum / kf;
            mean_out[row0 + threadIdx.x] = m;
            acc += m;
        }
    }
    const float total = block_sum(acc, wave_totals);
    if (threadIdx.x == 0) parts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void variance_kernel(const float* __restrict__ mean, unsigned n, const float* __restrict__ sum_parts_in,
                                                          unsigned n_sum_parts, float* __restrict__ var_parts, float* __restrict__ g_out) {
    __shared__ float wave_totals[kBlock / kWave];
    const float g = sum_parts(sum_parts_in, n_sum_parts, wave_totals) / (float)n;
    float acc = 0.0f;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float sub = g - mean[i];
        acc += sub * sub;
    }
    const float total = block_sum(acc, wave_totals);
    if (threadIdx.x == 0) {
        var_parts[blockIdx.x] = total;
        if (blockIdx.x == 0) *g_out = g;
    }
}

__global__ __launch_bounds__(kBlock) void flags_kernel(const float* __restrict__ mean, unsigned n, const float* __restrict__ var_parts,
                                                       unsigned n_var_parts, const float* __restrict__ g_in, float mul,
                                                       uint8_t* __restrict__ flags, float* __restrict__ stats) {
    __shared__ float wave_totals[kBlock / kWave];
    const float var = sum_parts(var_parts, n_var_parts, wave_totals) / (float)n;
    const float g = *g_in;
    const float thr = g + mul * sqrtf(var);
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) flags[i] = mean[i] > thr ? 0 : 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[0] = g;
        stats[1] = var;
        stats[2] = thr;
        stats[3] = (float)n;
    }
}

__global__ __launch_bounds__(kBlock) void radius_flags_kernel(const float* __restrict__ d2, unsigned n, unsigned k_stride, unsigned column,
                                                              float radius, uint8_t* __restrict__ flags) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
        flags[i] = d2[(size_t)i * k_stride + column] > radius ? 0 : 1;  // (:187-188: squared distance against the radius)
}

struct ZAcc {
    float sum = 0.0f, sum2 = 0.0f;
    // one neighbour (:22-24). An index outside [0, n) contributes nothing.
    __device__ __forceinline__ void add(int32_t idx, const float* __restrict__ intensities, unsigned n) {
        if ((unsigned)idx >= n) return;
        const float v = intensities[idx];
        sum += v;
        sum2 += v * v;
    }
};

template <bool ROW16>  // k_stride % 4 == 0 and a 16-byte aligned index array
__global__ __launch_bounds__(kBlock) void zscore_kernel(const float* __restrict__ intensities, const int32_t* __restrict__ knn, unsigned n,
                                                        unsigned k_stride, unsigned k_use, float sigma_min, float* __restrict__ out) {
    const float kf = (float)k_use;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        ZAcc z;
        const int32_t* __restrict__ row = knn + (size_t)i * k_stride;
        if (ROW16) {
            const int4* __restrict__ row4 = reinterpret_cast<const int4*>(row);
            for (unsigned j = 0; j < k_use; j += 4) {  // (j + 3 < k_stride: the stride is a multiple of 4)
                const int4 q = row4[j >> 2];
                z.add(q.x, intensities, n);
                if (j + 1 < k_use) z.add(q.y, intensities, n);
                if (j + 2 < k_use) z.add(q.z, intensities, n);
                if (j + 3 < k_use) z.add(q.w, intensities, n);
            }
        } else {
            for (unsigned j = 0; j < k_use; ++j) z.add(row[j], intensities, n);
        }
        const float mean = z.sum / kf;
        const float var = fmaxf(z.sum2 / kf - mean * mean, 0.0f);
        const float sigma = sqrtf(var);
        out[i] = sigma < sigma_min ? 0.0f : (intensities[i] - mean) / sigma;
    }
}

// rows of a tile of mean_kernel: 256, or the largest multiple of 4 that fits the LDS tile
inline unsigned tile_rows(size_t k_stride) {
    const size_t fit = (kTileFloats / k_stride) & ~(size_t)3;
    return (unsigned)(fit < (size_t)kBlock ? fit : (size_t)kBlock);
}

}  // namespace
}  // namespace sp

extern "C" size_t sp_outlier_workspace_bytes(size_t) { return sp::kWsFloats * sizeof(float); }

extern "C" int sp_outlier_statistical_flags(const float* knn_d2, size_t n, size_t k_stride, size_t k_use, float stddev_mul,
                                            uint8_t* flags_out, float* mean_dist_out, float* stats_out, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (n == 0) return SP_OK;
    if (!knn_d2 || !flags_out || !mean_dist_out || !stats_out || !workspace || workspace_bytes < kWsFloats * sizeof(float) ||
        k_use < 1 || k_use > k_stride || k_stride > kMaxStride || n >= kMaxPoints) {
        sp_set_error("[sp_outlier_statistical_flags] invalid argument (a null knn_d2 / flags_out / mean_dist_out / stats_out / "
                     "workspace, a workspace below sp_outlier_workspace_bytes, k_use outside [1, k_stride], k_stride > 2048, or "
                     "n >= 2^31)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    float* const sum_parts_ws = static_cast<float*>(workspace);
    float* const var_parts_ws = sum_parts_ws + kMaxParts;
    float* const g_ws = var_parts_ws + kMaxParts;
    const unsigned rows = tile_rows(k_stride);
    const size_t tiles = (n + rows - 1) / rows;
    const unsigned grid_a = (unsigned)(tiles < kMaxParts ? tiles : kMaxParts);
    const size_t blocks = (n + kBlock - 1) / kBlock;
    const unsigned grid_bc = (unsigned)(blocks < kMaxParts ? blocks : kMaxParts);
    if (reinterpret_cast<uintptr_t>(knn_d2) % 16 == 0)
        mean_kernel<true><<<grid_a, kBlock, 0, st>>>(knn_d2, (unsigned)n, (unsigned)k_stride, (unsigned)k_use, rows, mean_dist_out,
                                                     sum_parts_ws);
    else
        mean_kernel<false><<<grid_a, kBlock, 0, st>>>(knn_d2, (unsigned)n, (unsigned)k_stride, (unsigned)k_use, rows, mean_dist_out,
                                                      sum_parts_ws);
    variance_kernel<<<grid_bc, kBlock, 0, st>>>(mean_dist_out, (unsigned)n, sum_parts_ws, grid_a, var_parts_ws, g_ws);
    flags_kernel<<<grid_bc, kBlock, 0, st>>>(mean_dist_out, (unsigned)n, var_parts_ws, grid_bc, g_ws, stddev_mul, flags_out, stats_out);
    return launch_status();
}

extern "C" int sp_outlier_radius_flags(const float* knn_d2, size_t n, size_t k_stride, size_t column, float radius,
                                       uint8_t* flags_out, void* stream) {
    using namespace sp;
    if (n == 0) return SP_OK;
    if (!knn_d2 || !flags_out || column >= k_stride || k_stride >= ((size_t)1 << 31) || n >= kMaxPoints) {
        sp_set_error("[sp_outlier_radius_flags] invalid argument (a null knn_d2 / flags_out, column >= k_stride, or n >= 2^31)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    radius_flags_kernel<<<stream_grid(n), kBlock, 0, as_stream(stream)>>>(knn_d2, (unsigned)n, (unsigned)k_stride, (unsigned)column,
                                                                         radius, flags_out);
    return launch_status();
}

extern "C" int sp_intensity_zscore(const float* intensities_in, const int32_t* knn_indices, size_t n, size_t k_stride, size_t k_use,
                                   float sigma_min, float* intensities_out, void* stream) {
    using namespace sp;
    if (n == 0) return SP_OK;  // (:42: before any check)
    if (!intensities_in) {
        sp_set_error("[intensity_zscore::compute] Intensity field not found");
        return SP_ERR_RUNTIME;
    }
    if (k_use < 3) {
        sp_set_error("[intensity_zscore::compute] neighbors.k must be >= 3");
        return SP_ERR_RUNTIME;
    }
    if (intensities_out == intensities_in) {
        sp_set_error("[sp_intensity_zscore] intensities_out must not be intensities_in (the kernel reads the neighbours' intensities)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (!knn_indices || !intensities_out || k_use > k_stride || k_stride >= ((size_t)1 << 31) || n >= kMaxPoints) {
        sp_set_error("[sp_intensity_zscore] invalid argument (a null knn_indices / intensities_out, k_use > k_stride, or n >= 2^31)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    if (k_stride % 4 == 0 && reinterpret_cast<uintptr_t>(knn_indices) % 16 == 0)
        zscore_kernel<true><<<stream_grid(n), kBlock, 0, st>>>(intensities_in, knn_indices, (unsigned)n, (unsigned)k_stride,
                                                               (unsigned)k_use, sigma_min, intensities_out);
    else
        zscore_kernel<false><<<stream_grid(n), kBlock, 0, st>>>(intensities_in, knn_indices, (unsigned)n, (unsigned)k_stride,
                                                                (unsigned)k_use, sigma_min, intensities_out);
    return launch_status();
}
