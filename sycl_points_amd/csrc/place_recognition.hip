// Scan Context place recognition for gfx950 (MI355X extension): "have I been here before, and at what heading?"
//   sp_scan_context_compute(_host)   the polar height image of a scan: rings x sectors maxima of z + sensor_height
//   sp_scan_context_db_*             the keyframe database: every descriptor as normalised columns in the matrix cores' operand order
//   sp_scan_context_db_search        the query against EVERY entry of a range under every column shift, the k best
//   sp_scan_context_guesses_host     initial guesses for sp_gicp_align_batch around a candidate's shift
// The definitions are include/sycl_points_amd.h's. No float atomic anywhere: every result is the same bits on every call.
//
// Descriptor (descriptor_kernel): a lane per point. The sector is a count of half-plane tests against the boundary table, which
// arrives in the kernel arguments (uniform loads; no atan2, so host and device agree at every boundary); ring and value are plain
// f32. The bin takes an integer atomicMax on the value's bits (v >= 0: the order of the bits is the order of the floats) in LDS,
// and a workgroup issues one global atomicMax per bin it touched. A maximum does not depend on the order: the device's bits are
// the host twin's.
//
// Database entry (normalise_kernel, one wave, a lane per column): K_pad = rings rounded up to a multiple of 4, KS = K_pad / 2,
// TILES = 1 (sectors <= 32) or 2. The entry is TILES x 2 x KS x 32 floats laid out [tile][half][pair][column & 31][2]: lane
// (column & 31, half) of a wave reads the KS rings half * KS .. + KS - 1 of its column as KS / 2 float2s, each load of the wave
// 512 contiguous bytes, and has them as the KS k-steps of v_mfma_f32_32x32x2_f32 — step w multiplies ring w (lanes 0 .. 31) and
// ring KS + w (lanes 32 .. 63); query and candidate use the same assignment, so the sum runs over all rings. Rings and columns
// beyond the descriptor's are zeros. The 64-bit mask of non-empty columns lies in an array of its own.
//
// Search (search_kernel<KS, TILES>): a wave per candidate, striding over the range; the query's operands stay in registers, the
// next candidate's are requested before this one's products start. G = Q^T C as TILES x TILES tiles of 32 x 32; the tiles go to
// the wave's own LDS (row a at a * R + ((a + b) & (R - 1)), R = 32 TILES: both the store and the diagonal walk are spread over
// the banks without padding), lane s sums diagonal s in ascending column, N_s is a rotate-and-popcount of the two masks, and the
// wave takes the minimum of (bits of d_s) << 32 | s. A second kernel (select_kernel) selects the k smallest
// (bits of d) << 32 | index per 4096 keys, repeatedly, until one workgroup holds the answer.
//
// Compiled with -ffp-contract=off; sqrt and division are correctly rounded.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "sp_common.h"
#include "sp_internal.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

constexpr unsigned kMaxRings = SP_SCAN_CONTEXT_MAX_RINGS, kMaxSectors = SP_SCAN_CONTEXT_MAX_SECTORS;
constexpr size_t kMaxCloud = (size_t)1 << 32;

struct SectorTable {  // c_k = (float)cos(phi_k), s_k = (float)sin(phi_k), phi_k = -pi + 2 pi k / sectors (double)
    float c[kMaxSectors], s[kMaxSectors];
};
SectorTable sector_table(unsigned sectors) {
    SectorTable t{};
    for (unsigned k = 0; k < sectors; ++k) {
        const double phi = -M_PI + 2.0 * M_PI * (double)k / (double)sectors;
        t.c[k] = (float)cos(phi);
        t.s[k] = (float)sin(phi);
    }
    return t;
}

bool params_ok(const sp_scan_context_params* p, const char* who) {
    char msg[256];
    if (!p) {
        snprintf(msg, sizeof msg, "[%s] null params", who);
    } else if (p->rings < 1 || p->rings > kMaxRings) {
        snprintf(msg, sizeof msg, "[%s] rings must be in 1..SP_SCAN_CONTEXT_MAX_RINGS (32)", who);
    } else if (p->sectors < 4 || p->sectors > kMaxSectors || (p->sectors & 1u)) {
        snprintf(msg, sizeof msg, "[%s] sectors must be even and in 4..SP_SCAN_CONTEXT_MAX_SECTORS (64)", who);
    } else if (!(p->max_range > 0.0f) || !(p->max_range < INFINITY)) {
        snprintf(msg, sizeof msg, "[%s] max_range must be positive and finite", who);
    } else {
        return true;
    }
    sp_set_error(msg);
    return false;
}
inline float ring_scale(const sp_scan_context_params& p) { return (float)((double)p.rings / (double)p.max_range); }

// The bin and value of one point (the header's definition, in its order); false: the point is skipped.
__host__ __device__ inline bool bin_of(float x, float y, float z, const SectorTable& t, unsigned rings, unsigned sectors, float scale,
                                       float max_range, float sensor_height, unsigned* bin, float* value) {
    if (!(fabsf(x) < INFINITY) || !(fabsf(y) < INFINITY) || !(fabsf(z) < INFINITY)) return false;
    const float r2 = x * x + y * y;
    if (r2 == 0.0f) return false;
    const float r = sqrtf(r2);
    if (!(r < max_range)) return false;
    int ring = (int)floorf(r * scale);
    ring = ring < (int)rings - 1 ? ring : (int)rings - 1;
    const unsigned h = sectors / 2;
    const bool upper = y >= 0.0f;  // (-0.0 too)
    unsigned count = 0;
    for (unsigned k = 1; k < h; ++k) {  // (uniform: both halves are evaluated, the lane's own is counted)
        const bool lo = t.c[k] * y >= t.s[k] * x;
        const bool hi = t.c[k + h] * y >= t.s[k + h] * x;
        count += (upper ? hi : lo) ? 1u : 0u;
    }
    const unsigned sector = upper ? h + count : count;
    const float v = z + sensor_height;
    *bin = (unsigned)ring * sectors + sector;
    *value = v > 0.0f ? v : 0.0f;
    return true;
}

__global__ __launch_bounds__(kBlock) void descriptor_kernel(const float4* __restrict__ points, unsigned n, SectorTable table,
                                                            unsigned rings, unsigned sectors, float scale, float max_range,
                                                            float sensor_height, unsigned* __restrict__ desc_bits) {
    __shared__ unsigned s_bins[kMaxRings * kMaxSectors];
    const unsigned bins = rings * sectors;
    for (unsigned b = threadIdx.x; b < bins; b += kBlock) s_bins[b] = 0u;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {  // (n may be close to 2^32)
        const float4 p = points[i];
        unsigned bin;
        float v;
        if (bin_of(p.x, p.y, p.z, table, rings, sectors, scale, max_range, sensor_height, &bin, &v) && v > 0.0f)
            atomicMax(&s_bins[bin], __float_as_uint(v));  // (bin < rings * sectors by construction)
    }
    __syncthreads();
    for (unsigned b = threadIdx.x; b < bins; b += kBlock) {
        const unsigned v = s_bins[b];
        if (v) atomicMax(&desc_bits[b], v);
    }
}

// ------------------------------------------------------------------------------------------------------------- the entries
struct Layout {
    unsigned rings, sectors, ks, tiles;
    unsigned entry_floats() const { return tiles * 2u * ks * 32u; }
};
Layout layout_of(const sp_scan_context_params& p) {
    const unsigned k_pad = (p.rings + 3u) & ~3u;
    return Layout{p.rings, p.sectors, k_pad / 2u, p.sectors > 32u ? 2u : 1u};
}
__host__ __device__ inline unsigned entry_offset(unsigned ring, unsigned column, unsigned ks) {
    const unsigned t = column >> 5, col = column & 31u, h = ring / ks, w = ring % ks;
    return ((((t * 2u + h) * (ks / 2u) + (w >> 1)) * 32u + col) << 1) + (w & 1u);
}

// One wave: lane j normalises column j of desc (rings x sectors, ring-major) into `entry` and the wave stores the column mask.
__global__ __launch_bounds__(kWave) void normalise_kernel(const float* __restrict__ desc, Layout L, float* __restrict__ entry,
                                                          unsigned long long* __restrict__ mask) {
    const unsigned j = threadIdx.x;
    const bool column = j < L.sectors;
    double sum = 0.0;
    if (column)
        for (unsigned i = 0; i < L.rings; ++i) {
            const double v = (double)desc[i * L.sectors + j];
            sum += v * v;
        }
    const float norm = (float)sqrt(sum);
    const bool filled = column && norm != 0.0f;
    if (j < 32u * L.tiles)
        for (unsigned i = 0; i < 2u * L.ks; ++i)
            entry[entry_offset(i, j, L.ks)] = filled && i < L.rings ? desc[i * L.sectors + j] / norm : 0.0f;
    const unsigned long long m = __ballot(filled);
    if (j == 0) *mask = m;
}

// -------------------------------------------------------------------------------------------------------------- the search
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr unsigned long long kNoKey = ~0ull;

template <int KS, int TILES>
__device__ __forceinline__ void load_operands(const float* __restrict__ entry, unsigned col, unsigned h, float (&x)[TILES][KS]) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const float2* p = reinterpret_cast<const float2*>(entry) + (size_t)((t * 2 + (int)h) * (KS / 2)) * 32u + col;
#pragma unroll
        for (int c = 0; c < KS / 2; ++c) {
            const float2 v = p[c * 32];
            x[t][2 * c] = v.x, x[t][2 * c + 1] = v.y;
        }
    }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o, 64);
        v = other < v ? other : v;
    }
    return v;
}

// entries: the first candidate's entry; masks: its mask. keys[c] = (bits of distance) << 32 | (index_base + c), shifts[c] its shift.
template <int KS, int TILES>
__global__ __launch_bounds__(kBlock) void search_kernel(const float* __restrict__ entries, const unsigned long long* __restrict__ masks,
                                                        const float* __restrict__ query, const unsigned long long* __restrict__ query_mask,
                                                        unsigned index_base, unsigned count, unsigned sectors,
                                                        unsigned long long* __restrict__ keys, uint8_t* __restrict__ shifts) {
    constexpr unsigned R = 32u * TILES, kEntry = TILES * 2u * KS * 32u, kWaves = kBlock / kWave;
    __shared__ float s_g[kWaves][R * R];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, col = lane & 31u, h = lane >> 5;
    float* g = s_g[wave];
    const unsigned stride = gridDim.x * kWaves;
    unsigned c = blockIdx.x * kWaves + wave;
    if (c >= count) return;  // (uniform across the wave; no workgroup barrier below)

    float q[TILES][KS], cur[TILES][KS], nxt[TILES][KS];
    load_operands<KS, TILES>(query, col, h, q);
    const unsigned long long qm = *query_mask;
    const unsigned long long all = sectors == 64u ? ~0ull : (1ull << sectors) - 1ull;
    // column (j + s) mod sectors of the query on bit j
    const unsigned long long qrot = lane == 0u || lane >= sectors ? qm : ((qm >> lane) | (qm << (sectors - lane))) & all;
    load_operands<KS, TILES>(entries + (size_t)c * kEntry, col, h, cur);
    for (; c < count; c += stride) {
        const unsigned next = c + stride;
        if (next < count) load_operands<KS, TILES>(entries + (size_t)next * kEntry, col, h, nxt);
        const unsigned long long cm = masks[c];
        f32x16 acc[TILES][TILES];
#pragma unroll
        for (int ta = 0; ta < TILES; ++ta)
#pragma unroll
            for (int tb = 0; tb < TILES; ++tb) {
                f32x16 a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int w = 0; w < KS; ++w) a = __builtin_amdgcn_mfma_f32_32x32x2f32(q[ta][w], cur[tb][w], a, 0, 0, 0);
                acc[ta][tb] = a;
            }
        // G[a][b], a the query's column (the rows of the tile), b the candidate's (the lane's)
#pragma unroll
        for (int ta = 0; ta < TILES; ++ta)
#pragma unroll
            for (int tb = 0; tb < TILES; ++tb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned a = 32u * ta + (r & 3) + 8u * (r >> 2) + 4u * h, b = 32u * tb + col;
                    g[a * R + ((a + b) & (R - 1u))] = acc[ta][tb][r];
                }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        unsigned long long key = kNoKey;
        if (lane < sectors) {
            // ascending j; a = (j + s) mod sectors. (Unrolled over the tile's columns, every read in flight before the first add,
            // the kernel takes 255 VGPRs and the search at 10^5 entries 454 us against 305: not kept.)
            float sum = 0.0f;
            unsigned a = lane;
            for (unsigned j = 0; j < sectors; ++j) {
                sum += g[a * R + ((a + j) & (R - 1u))];
                a = a + 1u == sectors ? 0u : a + 1u;
            }
            const unsigned n = (unsigned)__popcll(qrot & cm);
            float d = n ? 1.0f - sum / (float)n : 1.0f;
            d = d < 0.0f ? 0.0f : d;
            key = ((unsigned long long)__float_as_uint(d) << 32) | lane;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (the next candidate's stores come after every lane's reads)
        key = wave_min_u64(key);
        if (lane == 0u) {
            keys[c] = (key & 0xffffffff00000000ull) | (unsigned long long)(index_base + c);
            shifts[c] = (uint8_t)(key & 0xffu);
        }
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int w = 0; w < KS; ++w) cur[t][w] = nxt[t][w];
    }
}

// The same search on the vector unit, for the A/B measurement of DESIGN.md 4.21 (sp_internal_scan_context_search_form(1)): lane b
// holds the candidate's column b in registers; step a takes the query's column a as scalar operands (uniform loads), so
// G[a][b] is 2 KS fmafs a lane, and adds it to the running sum of shift (a - b) mod sectors, which moves one lane up per step
// (a ds_bpermute). No LDS tile, no prefetch: a workgroup needs no LDS and 8 waves a SIMD hide the loads. A shift's columns are
// summed in cyclic order from column sectors - s, not from 0: the same value in exact arithmetic, not always the same bits.
template <int KS>
__global__ __launch_bounds__(kBlock) void search_valu_kernel(const float* __restrict__ entries, const unsigned long long* __restrict__ masks,
                                                             const float* __restrict__ query, const unsigned long long* __restrict__ query_mask,
                                                             unsigned index_base, unsigned count, unsigned sectors, unsigned tiles,
                                                             unsigned long long* __restrict__ keys, uint8_t* __restrict__ shifts) {
    constexpr unsigned kWaves = kBlock / kWave;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned entry_floats = tiles * 2u * KS * 32u;
    const bool column = lane < sectors;
    const unsigned b = column ? lane : 0u;  // (lanes beyond the columns ride along on column 0; their sums are not used)
    const unsigned t = b >> 5, col = b & 31u;
    const unsigned s_mine = sectors - 1u - b;  // the shift whose sum ends in this lane
    const unsigned long long qm = *query_mask;
    const unsigned long long all = sectors == 64u ? ~0ull : (1ull << sectors) - 1ull;
    const unsigned long long qrot = s_mine == 0u ? qm : ((qm >> s_mine) | (qm << (sectors - s_mine))) & all;
    const int from = column ? (int)(lane == 0u ? sectors - 1u : lane - 1u) : (int)lane;
    const float2* q2 = reinterpret_cast<const float2*>(query);
    for (unsigned c = blockIdx.x * kWaves + wave; c < count; c += gridDim.x * kWaves) {  // uniform across the wave
        const float2* e2 = reinterpret_cast<const float2*>(entries + (size_t)c * entry_floats);
        float cand[2 * KS];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int p = 0; p < KS / 2; ++p) {
                const float2 v = e2[((t * 2u + h) * (KS / 2) + p) * 32u + col];
                cand[h * KS + 2 * p] = v.x, cand[h * KS + 2 * p + 1] = v.y;
            }
        const unsigned long long cm = masks[c];
        float acc = 0.0f;
        for (unsigned a = 0; a < sectors; ++a) {
            if (a) acc = __shfl(acc, from, 64);
            const unsigned ta = a >> 5, ca = a & 31u;
            float g = 0.0f;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int p = 0; p < KS / 2; ++p) {
                    const float2 qv = q2[((ta * 2u + h) * (KS / 2) + p) * 32u + ca];  // (uniform)
                    g = fmaf(qv.x, cand[h * KS + 2 * p], g);
                    g = fmaf(qv.y, cand[h * KS + 2 * p + 1], g);
                }
            acc += g;
        }
        unsigned long long key = kNoKey;
        if (column) {
            const unsigned n = (unsigned)__popcll(qrot & cm);
            float d = n ? 1.0f - acc / (float)n : 1.0f;
            d = d < 0.0f ? 0.0f : d;
            key = ((unsigned long long)__float_as_uint(d) << 32) | s_mine;
        }
        key = wave_min_u64(key);
        if (lane == 0u) {
            keys[c] = (key & 0xffffffff00000000ull) | (unsigned long long)(index_base + c);
            shifts[c] = (uint8_t)(key & 0xffu);
        }
    }
}

// The k smallest of each chunk of kSelectChunk keys, ascending (keys are distinct: the index is part of them). unpack == 0:
// out_keys[block * k + r]; else (one workgroup) the answer's rows, kNoKey as -1 / FLT_MAX / 0.
constexpr unsigned kSelectPerLane = 16, kSelectChunk = kBlock * kSelectPerLane;
__global__ __launch_bounds__(kBlock) void select_kernel(const unsigned long long* __restrict__ in, unsigned n, unsigned k,
                                                        unsigned long long* __restrict__ out_keys, int unpack,
                                                        const uint8_t* __restrict__ shifts, unsigned index_base,
                                                        int32_t* __restrict__ idx_out, float* __restrict__ dist_out,
                                                        int32_t* __restrict__ shift_out) {
    __shared__ unsigned long long s_min[kBlock / kWave];
    const unsigned tid = threadIdx.x, base = blockIdx.x * kSelectChunk;
    unsigned long long v[kSelectPerLane];
#pragma unroll
    for (unsigned u = 0; u < kSelectPerLane; ++u) {
        const unsigned i = base + u * kBlock + tid;
        v[u] = i < n ? in[i] : kNoKey;
    }
    unsigned long long prev = 0;
    for (unsigned r = 0; r < k; ++r) {
        unsigned long long m = kNoKey;
#pragma unroll
        for (unsigned u = 0; u < kSelectPerLane; ++u) {
            const bool open = r == 0u || v[u] > prev;
            m = open && v[u] < m ? v[u] : m;
        }
        m = wave_min_u64(m);
        __syncthreads();  // (the previous round's reads of s_min)
        if ((tid & 63u) == 0u) s_min[tid >> 6] = m;
        __syncthreads();
        m = s_min[0];
#pragma unroll
        for (unsigned w = 1; w < kBlock / kWave; ++w) m = s_min[w] < m ? s_min[w] : m;
        prev = m;  // (kNoKey once the chunk is exhausted: nothing is above it, the later rounds give kNoKey too)
        if (tid == 0u) {
            if (!unpack) {
                out_keys[(size_t)blockIdx.x * k + r] = m;
            } else {
                const bool none = m == kNoKey;
                const unsigned idx = (unsigned)(m & 0xffffffffull);
                idx_out[r] = none ? -1 : (int32_t)idx;
                dist_out[r] = none ? FLT_MAX : __uint_as_float((unsigned)(m >> 32));
                shift_out[r] = none ? 0 : (int32_t)shifts[idx - index_base];
            }
        }
    }
}

struct Db {
    sp_scan_context_params params;
    Layout layout;
    size_t size = 0, capacity = 0, capacity_hint = 0;
    float* entries = nullptr;
    unsigned long long* masks = nullptr;
    StreamSet streams;
};

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
struct SearchPlan {
    size_t query_off, mask_off, keys_off, shifts_off, tmp_off[2], tmp_keys, bytes;
};
SearchPlan search_plan(const Layout& L, size_t count) {
    SearchPlan p{};
    p.query_off = 0;
    p.mask_off = align16((size_t)L.entry_floats() * 4);
    p.keys_off = p.mask_off + 16;
    p.shifts_off = p.keys_off + align16(8 * count);
    p.tmp_keys = (size_t)div_up(count, kSelectChunk) * SP_SCAN_CONTEXT_MAX_K;
    p.tmp_off[0] = p.shifts_off + align16(count);
    p.tmp_off[1] = p.tmp_off[0] + align16(8 * p.tmp_keys);
    p.bytes = p.tmp_off[1] + align16(8 * p.tmp_keys);
    return p;
}

int g_search_form = 0;  // sp_internal_scan_context_search_form

template <int KS>
void launch_search(const Layout& L, hipStream_t st, const float* entries, const unsigned long long* masks, const float* query,
                   const unsigned long long* qmask, unsigned first, unsigned count, unsigned long long* keys, uint8_t* shifts) {
    // workgroups a compute unit: two with the 64 KB tile of the two-tile kernels, eight otherwise
    auto grid = [&](unsigned per_cu) { return (unsigned)std::min<size_t>(div_up(count, kBlock / kWave), (size_t)kNumCU * per_cu); };
    if (g_search_form == 1)
        search_valu_kernel<KS><<<grid(8), kBlock, 0, st>>>(entries, masks, query, qmask, first, count, L.sectors, L.tiles, keys, shifts);
    else if (L.tiles == 1)
        search_kernel<KS, 1><<<grid(8), kBlock, 0, st>>>(entries, masks, query, qmask, first, count, L.sectors, keys, shifts);
    else
        search_kernel<KS, 2><<<grid(2), kBlock, 0, st>>>(entries, masks, query, qmask, first, count, L.sectors, keys, shifts);
}

int ensure_capacity(Db& db, hipStream_t st) {
    if (db.size < db.capacity) return SP_OK;
    size_t cap = db.capacity ? 2 * db.capacity : (db.capacity_hint ? db.capacity_hint : 64);
    if (cap > SP_SCAN_CONTEXT_DB_MAX) cap = SP_SCAN_CONTEXT_DB_MAX;
    const size_t entry_bytes = (size_t)db.layout.entry_floats() * 4;
    float* entries = nullptr;
    unsigned long long* masks = nullptr;
    hipError_t e = pooled_alloc(&entries, cap * entry_bytes, st);
    if (e == hipSuccess) e = pooled_alloc(&masks, cap * 8, st);
    if (e == hipSuccess && db.size) {
        e = hipMemcpyAsync(entries, db.entries, db.size * entry_bytes, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(masks, db.masks, db.size * 8, hipMemcpyDeviceToDevice, st);
    }
    if (e != hipSuccess) {
        sp_set_error(hipGetErrorString(e));
        pooled_free(entries);
        pooled_free(masks);
        return SP_ERR_HIP;
    }
    db.streams.note(st);
    pooled_free_after(db.entries, db.streams);  // (earlier searches may still read them)
    pooled_free_after(db.masks, db.streams);
    db.entries = entries, db.masks = masks, db.capacity = cap;
    return SP_OK;
}

}  // namespace
}  // namespace sp

extern "C" int sp_scan_context_boundaries_host(uint32_t sectors, float* cos_out, float* sin_out) {
    if (sectors < 4 || sectors > sp::kMaxSectors || (sectors & 1u) || !cos_out || !sin_out) {
        sp_set_error("[sp_scan_context_boundaries_host] sectors must be even and in 4..64; the outputs must not be null");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const sp::SectorTable t = sp::sector_table(sectors);
    memcpy(cos_out, t.c, sectors * sizeof(float));
    memcpy(sin_out, t.s, sectors * sizeof(float));
    return SP_OK;
}

extern "C" int sp_scan_context_compute_host(const sp_scan_context_params* params, const float* points_host, size_t n,
                                            float* desc_out_host) {
    using namespace sp;
    if (!params_ok(params, "sp_scan_context_compute_host")) return SP_ERR_INVALID_ARGUMENT;
    if (!desc_out_host || (n && !points_host)) {
        sp_set_error("[sp_scan_context_compute_host] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const SectorTable t = sector_table(params->sectors);
    const float scale = ring_scale(*params);
    const unsigned bins = params->rings * params->sectors;
    for (unsigned b = 0; b < bins; ++b) desc_out_host[b] = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float* p = points_host + 4 * i;
        unsigned bin;
        float v;
        if (bin_of(p[0], p[1], p[2], t, params->rings, params->sectors, scale, params->max_range, params->sensor_height, &bin, &v) &&
            v > desc_out_host[bin])
            desc_out_host[bin] = v;
    }
    return SP_OK;
}

extern "C" int sp_scan_context_compute(const sp_scan_context_params* params, const float* points, size_t n, float* desc_out,
                                       void* stream) {
    using namespace sp;
    if (!params_ok(params, "sp_scan_context_compute")) return SP_ERR_INVALID_ARGUMENT;
    if (!desc_out || (n && !points) || n >= kMaxCloud) {
        sp_set_error("[sp_scan_context_compute] null argument or n >= 2^32");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    const unsigned bins = params->rings * params->sectors;
    if (const int rc = zero_async(desc_out, (size_t)bins * 4, st); rc != SP_OK) return rc;
    if (n == 0) return SP_OK;
    descriptor_kernel<<<stream_grid(n, kBlock, 4), kBlock, 0, st>>>(reinterpret_cast<const float4*>(points), (unsigned)n,
                                                                    sector_table(params->sectors), params->rings, params->sectors,
                                                                    ring_scale(*params), params->max_range, params->sensor_height,
                                                                    reinterpret_cast<unsigned*>(desc_out));
    return launch_status();
}

extern "C" int sp_scan_context_db_create(const sp_scan_context_params* params, size_t capacity_hint, sp_scan_context_db** out) {
    using namespace sp;
    if (!out) {
        sp_set_error("[sp_scan_context_db_create] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    *out = nullptr;
    if (!params_ok(params, "sp_scan_context_db_create")) return SP_ERR_INVALID_ARGUMENT;
    if (capacity_hint > SP_SCAN_CONTEXT_DB_MAX) {
        sp_set_error("[sp_scan_context_db_create] capacity_hint exceeds SP_SCAN_CONTEXT_DB_MAX (2^20)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    Db* db = new (std::nothrow) Db();
    if (!db) {
        sp_set_error("[sp_scan_context_db_create] out of memory");
        return SP_ERR_RUNTIME;
    }
    db->params = *params;
    db->layout = layout_of(*params);
    db->capacity_hint = capacity_hint;  // (the arrays are taken at the first add: creating a database needs no device)
    *out = reinterpret_cast<sp_scan_context_db*>(db);
    return SP_OK;
}

extern "C" void sp_scan_context_db_destroy(sp_scan_context_db* handle) {
    using namespace sp;
    Db* db = reinterpret_cast<Db*>(handle);
    if (!db) return;
    pooled_free_after(db->entries, db->streams);
    pooled_free_after(db->masks, db->streams);
    delete db;
}

extern "C" size_t sp_scan_context_db_size(const sp_scan_context_db* handle) {
    return handle ? reinterpret_cast<const sp::Db*>(handle)->size : 0;
}

extern "C" int sp_scan_context_db_clear(sp_scan_context_db* handle) {
    if (!handle) {
        sp_set_error("[sp_scan_context_db_clear] null handle");
        return SP_ERR_INVALID_ARGUMENT;
    }
    reinterpret_cast<sp::Db*>(handle)->size = 0;  // (the storage is kept; work already enqueued on the old entries is ordered before later adds on the same stream)
    return SP_OK;
}

extern "C" int sp_scan_context_db_add(sp_scan_context_db* handle, const float* desc_device, void* stream) {
    using namespace sp;
    Db* db = reinterpret_cast<Db*>(handle);
    if (!db || !desc_device) {
        sp_set_error("[sp_scan_context_db_add] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (db->size >= SP_SCAN_CONTEXT_DB_MAX) {
        sp_set_error("[sp_scan_context_db_add] the database holds SP_SCAN_CONTEXT_DB_MAX (2^20) entries");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    if (const int rc = ensure_capacity(*db, st); rc != SP_OK) return rc;
    db->streams.note(st);
    normalise_kernel<<<1, kWave, 0, st>>>(desc_device, db->layout, db->entries + db->size * db->layout.entry_floats(),
                                          db->masks + db->size);
    if (const int rc = launch_status(); rc != SP_OK) return rc;
    ++db->size;
    return SP_OK;
}

extern "C" size_t sp_scan_context_db_search_workspace_bytes(const sp_scan_context_db* handle, size_t count) {
    if (!handle || count > SP_SCAN_CONTEXT_DB_MAX) return 0;
    return sp::search_plan(reinterpret_cast<const sp::Db*>(handle)->layout, count).bytes;
}

extern "C" int sp_scan_context_db_search(sp_scan_context_db* handle, const float* desc_device, size_t first, size_t count, size_t k,
                                         int32_t* idx_out, float* dist_out, int32_t* shift_out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    using namespace sp;
    Db* db = reinterpret_cast<Db*>(handle);
    if (!db) {
        sp_set_error("[sp_scan_context_db_search] null handle");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (k > SP_SCAN_CONTEXT_MAX_K) {
        sp_set_error("[sp_scan_context_db_search] k exceeds SP_SCAN_CONTEXT_MAX_K (32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (first > db->size || count > db->size - first) {
        sp_set_error("[sp_scan_context_db_search] [first, first + count) is not a range of the database's entries");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (k == 0) return SP_OK;
    if (!desc_device || !idx_out || !dist_out || !shift_out || !workspace) {
        sp_set_error("[sp_scan_context_db_search] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const Layout& L = db->layout;
    const SearchPlan p = search_plan(L, count);
    if (workspace_bytes < p.bytes || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
        sp_set_error("[sp_scan_context_db_search] the workspace is smaller than sp_scan_context_db_search_workspace_bytes(db, count) "
                     "or not 16-byte aligned");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    db->streams.note(st);
    char* ws = static_cast<char*>(workspace);
    float* query = reinterpret_cast<float*>(ws + p.query_off);
    auto* qmask = reinterpret_cast<unsigned long long*>(ws + p.mask_off);
    auto* keys = reinterpret_cast<unsigned long long*>(ws + p.keys_off);
    auto* shifts = reinterpret_cast<uint8_t*>(ws + p.shifts_off);
    unsigned long long* tmp[2] = {reinterpret_cast<unsigned long long*>(ws + p.tmp_off[0]),
                                  reinterpret_cast<unsigned long long*>(ws + p.tmp_off[1])};
    if (count) {
        normalise_kernel<<<1, kWave, 0, st>>>(desc_device, L, query, qmask);
        const float* entries = db->entries + first * L.entry_floats();
        const unsigned long long* masks = db->masks + first;
        const unsigned n = (unsigned)count, base = (unsigned)first;
        switch (L.ks) {
            case 2: launch_search<2>(L, st, entries, masks, query, qmask, base, n, keys, shifts); break;
            case 4: launch_search<4>(L, st, entries, masks, query, qmask, base, n, keys, shifts); break;
            case 6: launch_search<6>(L, st, entries, masks, query, qmask, base, n, keys, shifts); break;
            case 8: launch_search<8>(L, st, entries, masks, query, qmask, base, n, keys, shifts); break;
            case 10: launch_search<10>(L, st, entries, masks, query, qmask, base, n, keys, shifts); break;
            case 12: launch_search<12>(L, st, entries, masks, query, qmask, base, n, keys, shifts); break;
            case 14: launch_search<14>(L, st, entries, masks, query, qmask, base, n, keys, shifts); break;
            default: launch_search<16>(L, st, entries, masks, query, qmask, base, n, keys, shifts); break;
        }
    }
    // the k smallest keys: every pass leaves k per 4096, the last one (a single workgroup) writes the rows
    const unsigned long long* in = keys;
    size_t n = count;
    int flip = 0;
    while (n > kSelectChunk) {
        const unsigned blocks = div_up(n, kSelectChunk);
        select_kernel<<<blocks, kBlock, 0, st>>>(in, (unsigned)n, (unsigned)k, tmp[flip], 0, nullptr, 0u, nullptr, nullptr, nullptr);
        in = tmp[flip];
        n = (size_t)blocks * k;
        flip ^= 1;
    }
    select_kernel<<<1, kBlock, 0, st>>>(in, (unsigned)n, (unsigned)k, nullptr, 1, shifts, (unsigned)first, idx_out, dist_out, shift_out);
    return launch_status();
}

extern "C" int sp_scan_context_guesses_host(const sp_scan_context_params* params, uint32_t shift, size_t steps, double* poses_out) {
    using namespace sp;
    if (!params_ok(params, "sp_scan_context_guesses_host")) return SP_ERR_INVALID_ARGUMENT;
    if (shift >= params->sectors || (steps && !poses_out)) {
        sp_set_error("[sp_scan_context_guesses_host] shift must be below sectors; poses_out must not be null");
        return SP_ERR_INVALID_ARGUMENT;
    }
    for (size_t i = 0; i < steps; ++i) {
        const double delta = steps > 1 ? -0.5 + (double)i / (double)(steps - 1) : 0.0;
        const double angle = -((double)shift + delta) * (2.0 * M_PI) / (double)params->sectors;
        const double c = cos(angle), s = sin(angle);
        double* T = poses_out + 16 * i;
        for (int e = 0; e < 16; ++e) T[e] = 0.0;
        T[0] = c, T[1] = s, T[4] = -s, T[5] = c, T[10] = 1.0, T[15] = 1.0;
    }
    return SP_OK;
}

extern "C" int sp_internal_scan_context_search_form(int form) {
    if (form != 0 && form != 1) return -1;
    const int before = sp::g_search_form;
    sp::g_search_form = form;
    return before;
}
