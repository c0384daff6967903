// The building blocks the search structures share — GridKNN (grid.hip), the BVH (bvh.hip), the octree (octree.hip), the device
// KD-tree search (kdtree.hip) and brute force (knn_bruteforce.hip); voxel.hip and sampling.hip borrow one piece each — held once:
// the order-preserving float encoding, the bounding box of the finite points, the Morton key of a point in a box, the sorted
// insertion into a register-resident list, and two one-line kernels — and, on the query side, the pose an external search is asked
// at and the one way a kernel reads a query through it (QueryPose, query_pose, load_pose, load_query: a changed query argument
// has one place to change; the cell key of a query lives with the grid, grid_device.h). The kernels are templates (of nothing: launch them as
// `bbox_kernel<><<<...>>>`) so that a translation unit that launches one instantiates its own copy, with a row in its resource
// report, and one that does not gets nothing.
// Probed on their own by sp_internal_bbox / sp_internal_morton_keys / sp_internal_sorted_insert (spatial_probes.hip,
// tests/test_gpu_spatial_primitives.py).
#pragma once
#include <cfloat>

#include "sp_common.h"
#include "sp_math.h"

namespace sp {

// The pose an external search is asked at: a query q is searched at T * q, T column-major. `dev` names 16 floats resident on the
// device, or is null and the matrix travels by value in `m` (the identity when the caller gave none). One kernel argument; a caller
// that only wants the matrix by value takes the Mat4Arg it begins with.
struct QueryPose : Mat4Arg {
    const float* dev;
};
inline QueryPose query_pose(const float* transT, int transT_on_device) {
    QueryPose P;
    for (int i = 0; i < 16; ++i) P.m[i] = (transT && !transT_on_device) ? transT[i] : (i % 5 == 0 ? 1.0f : 0.0f);
    P.dev = transT_on_device ? transT : nullptr;
    return P;
}
__device__ __forceinline__ Rigid load_pose(const QueryPose& P) { return load_rigid_colmajor(P.dev ? P.dev : P.m); }
// Query qi where it is searched: T * queries[qi] by transform_point's fma chain (the reference's, sp_math.h) and no other.
__device__ __forceinline__ void load_query(const float4* __restrict__ queries, unsigned qi, const Rigid& T, float& x, float& y, float& z) {
    const float4 q4 = queries[qi];
    transform_point(T, q4.x, q4.y, q4.z, x, y, z);
}
// ... as a float4 whose .w the caller sets
__device__ __forceinline__ float4 load_query(const float4* __restrict__ queries, unsigned qi, const Rigid& T, float w) {
    float4 q;
    load_query(queries, qi, T, q.x, q.y, q.z);
    q.w = w;
    return q;
}

// Order-preserving float -> u32 and back: a < b as floats <=> ordered_bits(a) < ordered_bits(b) as unsigned (-0 below +0).
__host__ __device__ inline unsigned ordered_bits(float f) {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ordered_float(unsigned u) {
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// Three minima and three maxima over a workgroup of kBlock lanes (every lane calls): wave butterfly, then LDS across the
// waves. Thread t < 6 returns value t of (mn[0..2], mx[0..2]); the others return nothing of use.
template <class W>
__device__ __forceinline__ W block_minmax3(W (&mn)[3], W (&mx)[3]) {
    __shared__ W red[kBlock / kWave][6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            mn[a] = min(mn[a], (W)__shfl_xor((int)mn[a], o, kWave));
            mx[a] = max(mx[a], (W)__shfl_xor((int)mx[a], o, kWave));
        }
    }
    const unsigned wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[wave][a] = mn[a]; red[wave][3 + a] = mx[a]; }
    }
    __syncthreads();
    W v = 0;
    if (threadIdx.x < 6) {
        v = red[0][threadIdx.x];
        for (int w = 1; w < kBlock / kWave; ++w) v = threadIdx.x < 3 ? min(v, red[w][threadIdx.x]) : max(v, red[w][threadIdx.x]);
    }
    return v;
}
// ... and into box[0..5] = {min x y z, max x y z} with six integer atomics per workgroup (exact, order independent).
template <class W>
__device__ __forceinline__ void block_minmax3_atomic(W (&mn)[3], W (&mx)[3], W* box) {
    const W v = block_minmax3(mn, mx);
    if (threadIdx.x < 3) atomicMin(&box[threadIdx.x], v);
    else if (threadIdx.x < 6) atomicMax(&box[threadIdx.x], v);
}

// The box before any point: bbox[0..2] = min xyz, bbox[3..5] = max xyz as ordered_bits. A cloud without a finite point leaves it so.
__device__ __forceinline__ void bbox_sentinel(unsigned* bbox) {
    if (threadIdx.x < 6) bbox[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}
template <int = 0>
__global__ void bbox_init_kernel(unsigned* bbox) { bbox_sentinel(bbox); }

// Bounding box of the finite points into a box that holds the sentinel. Grid-stride, the caller chooses the workgroups (up to
// 256 are in use; 1024 workgroups: 26 us per 1M points — their 6 atomics each share one cache line).
// Precondition: n >= 1 (the tail load reads pts[n - 1]) and n + 3 * gridDim.x * 256 fits 32 bits.
template <int = 0>
__global__ __launch_bounds__(kBlock) void bbox_kernel(const float4* __restrict__ pts, unsigned n, unsigned* bbox) {
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    // (four loads in flight per lane: one at a time, 16 dependent trips made this the longest kernel of the grid build, 18 us)
    const unsigned stride = gridDim.x * kBlock;
    for (unsigned i0 = blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += 4 * stride) {
        float4 p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = pts[min(i0 + u * stride, n - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * stride < n && isfinite(p[u].x) && isfinite(p[u].y) && isfinite(p[u].z)) {
                const unsigned e[3] = {ordered_bits(p[u].x), ordered_bits(p[u].y), ordered_bits(p[u].z)};
#pragma unroll
                for (int a = 0; a < 3; ++a) { mn[a] = min(mn[a], e[a]); mx[a] = max(mx[a], e[a]); }
            }
    }
    block_minmax3_atomic(mn, mx, bbox);
}

__device__ __forceinline__ uint64_t spread21(uint64_t x) {  // up to 21 bits -> every third bit
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
__device__ __forceinline__ uint64_t morton3(uint64_t c0, uint64_t c1, uint64_t c2) {
    return spread21(c0) | (spread21(c1) << 1) | (spread21(c2) << 2);
}
// Cells per axis of a structure's curve: a coordinate becomes clamp((v - lo) / ext * scale, 0, cmax), 0 on an axis without extent.
struct MortonCells {
    float scale, cmax;
};
constexpr MortonCells kBvhCells{65535.0f, 65534.0f};       // 16 bits per axis; cell 65535 is left to the invalid key
constexpr MortonCells kOctCells{2097152.0f, 2097151.0f};   // 21 bits per axis
// Morton key of the finite point (x, y, z) in box = {lo x y z, hi x y z}: each axis scaled by its own extent, points outside clamped.
__device__ __forceinline__ uint64_t morton_key_in_box(float x, float y, float z, const float (&box)[6], MortonCells cells) {
    const float v[3] = {x, y, z};
    uint64_t c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = box[a], ext = box[3 + a] - lo;
        const float t = ext > 0.0f ? (v[a] - lo) / ext * cells.scale : 0.0f;
        c[a] = (uint64_t)fminf(fmaxf(t, 0.0f), cells.cmax);
    }
    return morton3(c[0], c[1], c[2]);
}

// Sorted insertion of (d, idx) into the first k slots of a register-resident list, written as a fully unrolled carry chain so
// the arrays stay in registers; kth = the k-th distance afterwards. Two orders:
//   kByDistance       strict '<' on the distance: a later arrival goes behind equal distances, the first one wins ties (the
//                     reference's rule, bruteforce.hpp / kdtree.hpp:119-137);
//   kByDistanceIndex  (distance, index) lexicographic; kth_idx = the k-th index afterwards, and with `bp` the positions of the
//                     entries ride along (the grid's fused covariance reads the neighbours by position).
// Empty slots hold (FLT_MAX, -1). A NaN distance compares false and is never taken; FLT_MAX and +inf never replace an empty slot.
enum class InsertOrder { kByDistance, kByDistanceIndex };
template <int KCAP, InsertOrder ORDER>
__device__ __forceinline__ void sorted_insert(float (&bd)[KCAP], int (&bi)[KCAP], int k, float d, int idx, float& kth,
                                              int* kth_idx = nullptr, int* bp = nullptr, int pos = 0) {
    constexpr bool kLex = ORDER == InsertOrder::kByDistanceIndex;
    if (KCAP == 1) {
        const bool better = d < bd[0] || (kLex && d == bd[0] && idx < bi[0]);
        bi[0] = better ? idx : bi[0];
        bd[0] = better ? d : bd[0];
        if (bp) bp[0] = better ? pos : bp[0];
        kth = bd[0];
        if (kth_idx) *kth_idx = bi[0];
        return;
    }
    float cd = d;
    int ci = idx, cp = pos;
    bool shifting = false;
#pragma unroll
    for (int i = 0; i < KCAP; ++i) {
        if (i < k) {
            // (two statements, not `... || (kLex && ...)`: with the constant inside the chain the brute-force kernels allocate
            // up to 30 VGPRs more — knn_bf_kernel<20, 1> 86 against 56, five waves a SIMD against eight)
            bool sw;
            if constexpr (kLex) sw = shifting || cd < bd[i] || (cd == bd[i] && ci < bi[i]);
            else sw = shifting || (cd < bd[i]);
            const float td = bd[i];
            const int ti = bi[i];
            const float nd = sw ? cd : td;
            const int ni = sw ? ci : ti;
            bd[i] = nd;
            bi[i] = ni;
            cd = sw ? td : cd;
            ci = sw ? ti : ci;
            if (bp) {  // (known when the call is inlined: no test remains)
                const int tp = bp[i];
                bp[i] = sw ? cp : tp;
                cp = sw ? tp : cp;
            }
            shifting = sw;
            kth = nd;  // after the last executed iteration (i == k - 1) this is bestK[k-1].dist_sq
            if (kth_idx) *kth_idx = ni;
        }
    }
}

// A result without neighbours: every slot keeps its initial -1 / FLT_MAX (knn/result.hpp:21-27).
template <int = 0>
__global__ void fill_empty_kernel(int32_t* idx, float* d2, size_t n) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) { idx[i] = -1; d2[i] = FLT_MAX; }
}

// out[i] = pts[order[i]] with the original index in .w, for i < n — or i < *n_dev when the count is a device word.
template <int = 0>
__global__ __launch_bounds__(kBlock) void gather_by_order_kernel(const float4* __restrict__ pts, const unsigned* __restrict__ order,
                                                                 unsigned n, float4* __restrict__ out,
                                                                 const unsigned* __restrict__ n_dev = nullptr) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (n_dev ? *n_dev : n)) return;
    const unsigned src = order[i];
    float4 p = pts[src];
    p.w = __uint_as_float(src);
    out[i] = p;
}

}  // namespace sp
