// sp_internal_bbox / sp_internal_morton_keys / sp_internal_sorted_insert (sp_internal.h): the pieces of sp_spatial.h on their own,
// for tests/test_gpu_spatial_primitives.py. Each entry wraps exactly what the search structures call and does nothing more.
#include "sp_internal.h"
#include "sp_spatial.h"

namespace sp {
namespace {

__global__ __launch_bounds__(kBlock) void probe_morton_kernel(const float4* __restrict__ pts, unsigned n, const float* __restrict__ lo3,
                                                              const float* __restrict__ hi3, MortonCells cells,
                                                              uint64_t* __restrict__ keys) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    const float box[6] = {lo3[0], lo3[1], lo3[2], hi3[0], hi3[1], hi3[2]};
    keys[i] = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) ? morton_key_in_box(p.x, p.y, p.z, box, cells) : ~0ull;
}

// One lane per row: the row's m candidates, in sequence, into an empty list; the first k slots go out.
template <int KCAP, InsertOrder ORDER>
__global__ __launch_bounds__(kBlock) void probe_insert_kernel(int k, const float* __restrict__ d, const int32_t* __restrict__ idx,
                                                              unsigned rows, unsigned m, float* __restrict__ d_out,
                                                              int32_t* __restrict__ idx_out) {
    const unsigned r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= rows) return;
    float bd[KCAP];
    int bi[KCAP];
#pragma unroll
    for (int i = 0; i < KCAP; ++i) { bd[i] = FLT_MAX; bi[i] = -1; }
    float kth = FLT_MAX;
    int kth_idx = -1;
    for (unsigned j = 0; j < m; ++j)
        sorted_insert<KCAP, ORDER>(bd, bi, k, d[(size_t)r * m + j], idx[(size_t)r * m + j], kth, &kth_idx);
#pragma unroll
    for (int i = 0; i < KCAP; ++i)
        if (i < k) { d_out[(size_t)r * k + i] = bd[i]; idx_out[(size_t)r * k + i] = bi[i]; }
}

template <int KCAP>
void launch_insert(int order, int k, const float* d, const int32_t* idx, unsigned rows, unsigned m, float* d_out, int32_t* idx_out,
                   hipStream_t st) {
    if (order == 0)
        probe_insert_kernel<KCAP, InsertOrder::kByDistance><<<div_up(rows, kBlock), kBlock, 0, st>>>(k, d, idx, rows, m, d_out, idx_out);
    else
        probe_insert_kernel<KCAP, InsertOrder::kByDistanceIndex><<<div_up(rows, kBlock), kBlock, 0, st>>>(k, d, idx, rows, m, d_out, idx_out);
}

}  // namespace
}  // namespace sp

extern "C" int sp_internal_bbox(const float* points, size_t n, unsigned workgroups, uint32_t* box6_words_out, void* stream) {
    using namespace sp;
    // (bbox_kernel's precondition: n + 3 * workgroups * 256 in 32 bits)
    if (!box6_words_out || workgroups < 1 || workgroups > 256 || n >= (1ull << 31)) return SP_ERR_INVALID_ARGUMENT;
    hipStream_t st = as_stream(stream);
    bbox_init_kernel<><<<1, 64, 0, st>>>(box6_words_out);
    if (n) bbox_kernel<><<<workgroups, kBlock, 0, st>>>(reinterpret_cast<const float4*>(points), (unsigned)n, box6_words_out);
    return launch_status();
}

extern "C" int sp_internal_morton_keys(const float* points, size_t n, const float* lo3, const float* hi3, int mode,
                                       uint64_t* keys_out, void* stream) {
    using namespace sp;
    if ((mode != 0 && mode != 1) || n >= (1ull << 31)) return SP_ERR_INVALID_ARGUMENT;
    if (n == 0) return SP_OK;
    probe_morton_kernel<<<div_up(n, kBlock), kBlock, 0, as_stream(stream)>>>(reinterpret_cast<const float4*>(points), (unsigned)n, lo3, hi3,
                                                                             mode == 0 ? kBvhCells : kOctCells, keys_out);
    return launch_status();
}

extern "C" int sp_internal_sorted_insert(int order, int kcap, int k, const float* d, const int32_t* idx, size_t rows, size_t m,
                                         float* d_out, int32_t* idx_out, void* stream) {
    using namespace sp;
    // the largest lists the library keeps: 100 by distance (kdtree.hip), 32 by (distance, index) (bvh.hip)
    const bool cap_ok = kcap == 1 || kcap == 10 || kcap == (order == 0 ? 100 : 32);
    if ((order != 0 && order != 1) || !cap_ok || k < 1 || k > kcap || rows >= (1ull << 31) || m >= (1ull << 31))
        return SP_ERR_INVALID_ARGUMENT;
    if (rows == 0) return SP_OK;
    hipStream_t st = as_stream(stream);
    const unsigned r = (unsigned)rows, mm = (unsigned)m;
    if (kcap == 1) launch_insert<1>(order, k, d, idx, r, mm, d_out, idx_out, st);
    else if (kcap == 10) launch_insert<10>(order, k, d, idx, r, mm, d_out, idx_out, st);
    else if (order == 0) probe_insert_kernel<100, InsertOrder::kByDistance><<<div_up(r, kBlock), kBlock, 0, st>>>(k, d, idx, r, mm, d_out, idx_out);
    else probe_insert_kernel<32, InsertOrder::kByDistanceIndex><<<div_up(r, kBlock), kBlock, 0, st>>>(k, d, idx, r, mm, d_out, idx_out);
    return launch_status();
}
