// sensor_msgs/PointCloud2 ingestion for gfx950: the conversion kernel of ros2::fromROS2msg (ros2/convert.hpp:192-248) with its host
// loop over the time stamps (:144-190), the packing loop of ros2::toROS2msg (:394-426), and
// ros2::EnhancedReflectivityCorrector::apply (ros2/enhanced_reflectivity.hpp:45-140), all on the device.
//
// Records have any point_step (22, 26, 33 ... bytes), so their fields are unaligned. No lane loads bytes from global memory: a
// workgroup owns SP_PC2_BLOCK_POINTS = 256 consecutive records, whose byte span starts at a multiple of 256 * point_step (16-byte
// aligned, as data_dev is), copies the span into LDS with aligned 16-byte loads, and every lane assembles the fields of its record
// from aligned LDS words. The packing goes the other way: words into LDS, 16-byte stores out.
// Everything is bound by memory bandwidth: point_step bytes in, 16 (+ 16 + 4 + 4) out per point.
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string_view>

#include "sp_common.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

constexpr unsigned kPc2Points = SP_PC2_BLOCK_POINTS;
static_assert(kPc2Points == (unsigned)kBlock, "one lane per record of the workgroup's span");
constexpr unsigned kRings = SP_ER_MAX_RINGS;
static_assert(kRings == (unsigned)kBlock, "one lane per ring in the reflectivity sums");

/// LDS bytes for `records` records of `step` bytes: whole 16-byte slots plus one so that lds_u32's second word exists
inline size_t stage_bytes(unsigned step) { return ((size_t)kPc2Points * step + 15) / 16 * 16 + 16; }

/// bytes [0, bytes) of src (16-byte aligned; readable up to the next multiple of 16) -> lds; the caller synchronises
__device__ __forceinline__ void stage_records(const uint8_t* __restrict__ src, unsigned bytes, uint32_t* lds) {
    const uint4* g = reinterpret_cast<const uint4*>(src);
    uint4* s = reinterpret_cast<uint4*>(lds);
    const unsigned slots = (bytes + 15u) / 16u;
    for (unsigned v = threadIdx.x; v < slots; v += kBlock) s[v] = g[v];
}
/// the four bytes at byte offset `off` of the staged span, little endian, from the two aligned words that hold them
__device__ __forceinline__ uint32_t lds_u32(const uint32_t* lds, unsigned off) {
    const uint64_t pair = (uint64_t)lds[off >> 2] | ((uint64_t)lds[(off >> 2) + 1] << 32);
    return (uint32_t)(pair >> ((off & 3u) * 8u));
}
__device__ __forceinline__ uint32_t lds_u16(const uint32_t* lds, unsigned off) { return lds_u32(lds, off) & 0xffffu; }
__device__ __forceinline__ uint32_t lds_u8(const uint32_t* lds, unsigned off) { return (lds[off >> 2] >> ((off & 3u) * 8u)) & 0xffu; }
__device__ __forceinline__ double lds_f64(const uint32_t* lds, unsigned off) {
    return __longlong_as_double((long long)((uint64_t)lds_u32(lds, off) | ((uint64_t)lds_u32(lds, off + 4) << 32)));
}

// ------------------------------------------------------------------------------------------------------------------ unpack
__global__ __launch_bounds__(kBlock) void pc2_unpack_kernel(const uint8_t* __restrict__ data, unsigned n, sp_pc2_layout L,
                                                            float4* __restrict__ points, float4* __restrict__ rgb,
                                                            float* __restrict__ intensities, float* __restrict__ timestamps,
                                                            unsigned long long* block_max_bits) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const size_t p0 = (size_t)blockIdx.x * kPc2Points;
    const unsigned cnt = (unsigned)((size_t)n - p0 < kPc2Points ? (size_t)n - p0 : kPc2Points);
    stage_records(data + p0 * L.point_step, cnt * L.point_step, lds);
    __syncthreads();
    const unsigned t = threadIdx.x;
    const size_t i = p0 + t;
    unsigned long long max_bits = 0ull;  // of a double >= +0: their order is the order of their bits
    if (t < cnt) {
        const unsigned base = t * L.point_step;
        float4 p;
        p.w = 1.0f;
        if (L.xyz_type == SP_PC2_FLOAT32) {
            p.x = __uint_as_float(lds_u32(lds, base + L.x_offset));
            p.y = __uint_as_float(lds_u32(lds, base + L.y_offset));
            p.z = __uint_as_float(lds_u32(lds, base + L.z_offset));
        } else {
            p.x = (float)lds_f64(lds, base + L.x_offset);
            p.y = (float)lds_f64(lds, base + L.y_offset);
            p.z = (float)lds_f64(lds, base + L.z_offset);
        }
        points[i] = p;
        if (L.rgb_offset >= 0) {
            const uint32_t c = lds_u32(lds, base + L.rgb_offset);
            rgb[i] = make_float4((float)(c & 0xffu) / 255.0f, (float)((c >> 8) & 0xffu) / 255.0f, (float)((c >> 16) & 0xffu) / 255.0f,
                                 (float)(c >> 24) / 255.0f);
        }
        if (L.intensity_offset >= 0)
            intensities[i] = L.intensity_type == SP_PC2_FLOAT32 ? __uint_as_float(lds_u32(lds, base + L.intensity_offset))
                                                                : (float)lds_u16(lds, base + L.intensity_offset);
        if (L.timestamp_offset >= 0) {
            const unsigned at = base + L.timestamp_offset;
            double offset_ms = 0.0;
            float stored;
            if (L.timestamp_type == SP_PC2_UINT32) {  // nanoseconds from the start of the scan
                stored = (float)lds_u32(lds, at) * 1e-6f;
                offset_ms = (double)stored;
            } else {
                if (L.timestamp_type == SP_PC2_FLOAT32) {  // seconds from the start of the scan
                    const double raw = (double)__uint_as_float(lds_u32(lds, at));
                    if (isfinite(raw) && raw > 0.0) offset_ms = raw * 1e3;
                } else {  // seconds; beyond 1e8 an absolute Unix time
                    const double raw = lds_f64(lds, at);
                    if (isfinite(raw) && raw >= 0.0) {
                        offset_ms = raw > 1e8 ? raw * 1e3 - L.start_time_ms : raw * 1e3;
                        if (offset_ms < 0.0) offset_ms = 0.0;
                    }
                }
                stored = (float)offset_ms;
            }
            timestamps[i] = stored;
            if (offset_ms > 0.0) max_bits = (unsigned long long)__double_as_longlong(offset_ms);  // (-0.0 counts as +0, as std::max leaves it)
        }
    }
    if (L.timestamp_offset >= 0) {  // (uniform: every lane of the wave takes part)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(max_bits, o, 64);
            max_bits = other > max_bits ? other : max_bits;
        }
        // one value per workgroup, stored: 2048 waves sending an atomic to one address took 22 of this kernel's 26 us
        unsigned long long* s_max = reinterpret_cast<unsigned long long*>(lds);
        __syncthreads();  // (every lane has read its record)
        if ((t & 63u) == 0) s_max[t >> 6] = max_bits;
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (unsigned w = 1; w < kBlock / kWave; ++w) max_bits = s_max[w] > max_bits ? s_max[w] : max_bits;
            block_max_bits[blockIdx.x] = max_bits;
        }
    }
}

/// The maximum over the workgroups' values: one workgroup of 1024 lanes (an integer maximum: the same for every order)
__global__ __launch_bounds__(1024) void pc2_max_kernel(const unsigned long long* __restrict__ block_max_bits, unsigned blocks,
                                                       unsigned long long* max_offset_bits) {
    __shared__ unsigned long long s_max[1024 / kWave];
    const unsigned t = threadIdx.x;
    unsigned long long m = 0ull;
    for (unsigned b = t; b < blocks; b += 1024) m = block_max_bits[b] > m ? block_max_bits[b] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(m, o, 64);
        m = other > m ? other : m;
    }
    if ((t & 63u) == 0) s_max[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (unsigned w = 1; w < 1024 / kWave; ++w) m = s_max[w] > m ? s_max[w] : m;
        *max_offset_bits = m;
    }
}

// -------------------------------------------------------------------------------------------------------------------- pack
__global__ __launch_bounds__(kBlock) void pc2_pack_kernel(const float4* __restrict__ points, const float4* __restrict__ rgb,
                                                          const float* __restrict__ intensities, const float* __restrict__ timestamps,
                                                          unsigned n, double start_time_ms, unsigned step, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const size_t p0 = (size_t)blockIdx.x * kPc2Points;
    const unsigned cnt = (unsigned)((size_t)n - p0 < kPc2Points ? (size_t)n - p0 : kPc2Points);
    const unsigned t = threadIdx.x;
    if (t < cnt) {
        const size_t i = p0 + t;
        uint32_t* rec = lds + t * (step / 4);  // (every record length of toROS2msg is a multiple of 4)
        const float4 p = points[i];
        rec[0] = __float_as_uint(p.x); rec[1] = __float_as_uint(p.y); rec[2] = __float_as_uint(p.z); rec[3] = __float_as_uint(p.w);
        unsigned w = 4;
        if (rgb) {
            const float4 c = rgb[i];
            auto q = [](float v) { return (uint32_t)(uint8_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); };  // NaN -> fmaxf gives 0
            rec[w++] = q(c.x) | (q(c.y) << 8) | (q(c.z) << 16) | (q(c.w) << 24);
        }
        if (intensities) rec[w++] = __float_as_uint(intensities[i]);
        if (timestamps) {
            const uint64_t b = (uint64_t)__double_as_longlong((start_time_ms + (double)timestamps[i]) * 1e-3);
            rec[w++] = (uint32_t)b;
            rec[w++] = (uint32_t)(b >> 32);
        }
    }
    __syncthreads();
    // the span starts at p0 * step, a multiple of 256 * 4: whole 16-byte slots first, then the words of a short last span
    const unsigned words = cnt * (step / 4);
    uint8_t* dst = out + p0 * step;
    for (unsigned v = t; v < words / 4; v += kBlock) reinterpret_cast<uint4*>(dst)[v] = reinterpret_cast<const uint4*>(lds)[v];
    for (unsigned wd = (words & ~3u) + t; wd < words; wd += kBlock) reinterpret_cast<uint32_t*>(dst)[wd] = lds[wd];
}

// ------------------------------------------------------------------------------------------------- enhanced reflectivity
struct ErFields {  // by value in the kernarg segment
    unsigned step, ring_offset, ambient_offset;
    int ring_is_u8;
};
struct ErPoint {
    unsigned ring;
    float ref, amb;  // enhanced_reflectivity.hpp:84-95; both 0 where range_sq < 1e-6f
    bool in_range;
};
__device__ __forceinline__ ErPoint er_point(const uint32_t* lds, unsigned base, const ErFields& F, const float4 p, float intensity) {
    ErPoint e;
    e.ring = F.ring_is_u8 ? lds_u8(lds, base + F.ring_offset) : lds_u16(lds, base + F.ring_offset);
    const float range_sq = p.x * p.x + p.y * p.y + p.z * p.z;
    e.in_range = !(range_sq < 1e-6f);
    e.ref = e.in_range ? intensity * range_sq : 0.0f;
    e.amb = e.in_range ? (float)lds_u16(lds, base + F.ambient_offset) / range_sq : 0.0f;
    return e;
}

constexpr unsigned kErLaneArrays = 3 * kPc2Points * 4;  // ring, ref, amb of a tile, in front of the staged records

/// Launch 1: workgroup b sums the points [b * span, (b + 1) * span) per ring, in index order: lane r owns ring r and walks the
/// tile's 256 (ring, ref, amb) entries in LDS (every lane reads the same address: a broadcast), adding the ones that are its own.
/// partials: [b][ref | amb | count][256]
__global__ __launch_bounds__(kBlock) void er_partials_kernel(const float4* __restrict__ points, const float* __restrict__ intensities,
                                                             unsigned n, const uint8_t* __restrict__ data, ErFields F, unsigned span,
                                                             uint32_t* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    int* s_ring = reinterpret_cast<int*>(lds);
    float* s_ref = reinterpret_cast<float*>(lds) + kPc2Points;
    float* s_amb = reinterpret_cast<float*>(lds) + 2 * kPc2Points;
    const uint32_t* rec = lds + kErLaneArrays / 4;
    const unsigned t = threadIdx.x;
    const size_t begin = (size_t)blockIdx.x * span;
    const size_t end = begin + span < (size_t)n ? begin + span : (size_t)n;
    float sum_ref = 0.0f, sum_amb = 0.0f;
    unsigned count = 0;
    for (size_t p0 = begin; p0 < end; p0 += kPc2Points) {  // (span is a multiple of 256: every tile starts 16-byte aligned)
        const unsigned cnt = (unsigned)(end - p0 < kPc2Points ? end - p0 : kPc2Points);
        stage_records(data + p0 * F.step, cnt * F.step, const_cast<uint32_t*>(rec));
        __syncthreads();
        int ring = -1;
        float ref = 0.0f, amb = 0.0f;
        if (t < cnt) {
            const ErPoint e = er_point(rec, t * F.step, F, points[p0 + t], intensities[p0 + t]);
            if (e.in_range && e.ring < kRings) { ring = (int)e.ring; ref = e.ref; amb = e.amb; }
        }
        s_ring[t] = ring;
        s_ref[t] = ref;
        s_amb[t] = amb;
        __syncthreads();
#pragma unroll 2
        for (unsigned j = 0; j < kPc2Points; j += 4) {
            const int4 r4 = *reinterpret_cast<const int4*>(s_ring + j);
            const float4 a4 = *reinterpret_cast<const float4*>(s_ref + j);
            const float4 b4 = *reinterpret_cast<const float4*>(s_amb + j);
            if (r4.x == (int)t) { sum_ref += a4.x; sum_amb += b4.x; ++count; }
            if (r4.y == (int)t) { sum_ref += a4.y; sum_amb += b4.y; ++count; }
            if (r4.z == (int)t) { sum_ref += a4.z; sum_amb += b4.z; ++count; }
            if (r4.w == (int)t) { sum_ref += a4.w; sum_amb += b4.w; ++count; }
        }
        __syncthreads();  // (the next tile overwrites the arrays)
    }
    uint32_t* out = partials + (size_t)blockIdx.x * 3 * kRings;
    out[t] = __float_as_uint(sum_ref);
    out[kRings + t] = __float_as_uint(sum_amb);
    out[2 * kRings + t] = count;
}

constexpr unsigned kErSlices = 4;  // launch 2: the spans in four contiguous slices, one group of 256 lanes each

/// Launch 2: one workgroup of 4 x 256 lanes. Lane (s, r) adds ring r's partials over slice s of the spans in span order (eight
/// loads in flight: a chain of dependent L2 round trips is what this launch costs), then lane (0, r) adds the four slices in
/// slice order and updates the ring's means (:107-123). The order depends on the number of spans alone.
__global__ __launch_bounds__(kErSlices * kRings) void er_update_kernel(const uint32_t* __restrict__ partials, unsigned blocks,
                                                                       uint32_t* state, float ema_alpha) {
    __shared__ float s_ref[kErSlices][kRings], s_amb[kErSlices][kRings];
    __shared__ unsigned s_count[kErSlices][kRings];
    const unsigned r = threadIdx.x % kRings, slice = threadIdx.x / kRings;
    const unsigned per = (blocks + kErSlices - 1) / kErSlices;
    const unsigned b0 = slice * per < blocks ? slice * per : blocks, b1 = b0 + per < blocks ? b0 + per : blocks;
    float sum_ref = 0.0f, sum_amb = 0.0f;
    unsigned count = 0;
#pragma unroll 8
    for (unsigned b = b0; b < b1; ++b) {
        const uint32_t* p = partials + (size_t)b * 3 * kRings;
        sum_ref += __uint_as_float(p[r]);
        sum_amb += __uint_as_float(p[kRings + r]);
        count += p[2 * kRings + r];
    }
    s_ref[slice][r] = sum_ref;
    s_amb[slice][r] = sum_amb;
    s_count[slice][r] = count;
    __syncthreads();
    if (slice != 0) return;
#pragma unroll
    for (unsigned s = 1; s < kErSlices; ++s) {
        sum_ref += s_ref[s][r];
        sum_amb += s_amb[s][r];
        count += s_count[s][r];
    }
    if (count == 0) return;  // no point of this ring in the scan: its means stay
    const float cnt = (float)count;
    const float new_ref = sum_ref / cnt, new_amb = sum_amb / cnt;
    float* mean_ref = reinterpret_cast<float*>(state);
    float* mean_amb = mean_ref + kRings;
    uint32_t* initialised = state + 2 * kRings;
    if (!initialised[r]) {
        mean_ref[r] = new_ref;
        mean_amb[r] = new_amb;
        initialised[r] = 1u;
    } else {
        mean_ref[r] = ema_alpha * new_ref + (1.0f - ema_alpha) * mean_ref[r];
        mean_amb[r] = ema_alpha * new_amb + (1.0f - ema_alpha) * mean_amb[r];
    }
}

/// Launch 3: normalise by the ring's means, clamp, write back (:127-138)
__global__ __launch_bounds__(kBlock) void er_apply_kernel(const float4* __restrict__ points, float* intensities, unsigned n,
                                                          const uint8_t* __restrict__ data, ErFields F,
                                                          const float* __restrict__ state, float clip_max) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const size_t p0 = (size_t)blockIdx.x * kPc2Points;
    const unsigned cnt = (unsigned)((size_t)n - p0 < kPc2Points ? (size_t)n - p0 : kPc2Points);
    stage_records(data + p0 * F.step, cnt * F.step, lds);
    __syncthreads();
    const unsigned t = threadIdx.x;
    if (t >= cnt) return;
    const size_t i = p0 + t;
    const ErPoint e = er_point(lds, t * F.step, F, points[i], intensities[i]);
    float v = 0.0f;
    if (e.ring < kRings) {
        float ref = e.ref, amb = e.amb;
        const float mean_ref = state[e.ring], mean_amb = state[kRings + e.ring];
        if (mean_ref > 0.0f) ref /= mean_ref;
        if (mean_amb > 0.0f) amb /= mean_amb;
        v = ref + amb;
        v = v < 0.0f ? 0.0f : (clip_max < v ? clip_max : v);  // std::clamp
    }
    intensities[i] = v;
}

/// Points per workgroup of launch 1: 512 while that needs at most 2048 workgroups, then whatever does (a multiple of 256)
inline unsigned er_span(size_t n) {
    const size_t kMaxBlocks = 2048;
    if ((n + 511) / 512 <= kMaxBlocks) return 512;
    const size_t per = (n + kMaxBlocks - 1) / kMaxBlocks;
    return (unsigned)((per + kPc2Points - 1) / kPc2Points * kPc2Points);
}
inline unsigned er_blocks(size_t n) { return div_up(n, er_span(n)); }

int field_size(int type) {
    switch (type) {
        case SP_PC2_INT8: case SP_PC2_UINT8: return 1;
        case SP_PC2_INT16: case SP_PC2_UINT16: return 2;
        case SP_PC2_INT32: case SP_PC2_UINT32: case SP_PC2_FLOAT32: return 4;
        case SP_PC2_FLOAT64: return 8;
    }
    return 0;
}
bool field_inside(int32_t offset, int type, uint32_t point_step) {
    return offset >= 0 && field_size(type) > 0 && (uint64_t)offset + (uint64_t)field_size(type) <= (uint64_t)point_step;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace sp

extern "C" int sp_pc2_resolve_fields_host(const char* const* names, const uint32_t* offsets, const uint8_t* datatypes, size_t num_fields,
                                          uint32_t point_step, int convert_rgb, int convert_intensity,
                                          int use_reflectivity_as_intensity, sp_pc2_layout* layout_out) {
    using namespace sp;
    if (!layout_out || point_step == 0 || (num_fields && (!names || !offsets || !datatypes))) {
        sp_set_error("[sp_pc2_resolve_fields_host] invalid argument (a null pointer or point_step == 0)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    struct Slot { int32_t offset = -1; uint8_t type = 0; } x, y, z, rgb, intensity, reflectivity, timestamp;
    for (size_t f = 0; f < num_fields; ++f) {
        if (!names[f]) {
            sp_set_error("[sp_pc2_resolve_fields_host] invalid argument (a null field name)");
            return SP_ERR_INVALID_ARGUMENT;
        }
        const std::string_view name(names[f]);
        Slot* s = name == "x" ? &x : name == "y" ? &y : name == "z" ? &z : (name == "rgb" || name == "rgba") ? &rgb
                  : name == "intensity" ? &intensity : name == "reflectivity" ? &reflectivity
                  : (name == "t" || name == "time" || name == "timestamp" || name == "offset_time") ? &timestamp : nullptr;
        if (!s) continue;
        if (offsets[f] > (uint32_t)INT32_MAX) {
            sp_set_error("[sp_pc2_resolve_fields_host] invalid argument (a field offset beyond 2^31)");
            return SP_ERR_INVALID_ARGUMENT;
        }
        s->offset = (int32_t)offsets[f];
        s->type = datatypes[f];
    }
    if (x.offset < 0 || y.offset < 0 || z.offset < 0) {
        sp_set_error("Not found point cloud field");
        return SP_ERR_RUNTIME;
    }
    if ((x.type != SP_PC2_FLOAT32 && x.type != SP_PC2_FLOAT64) || x.type != y.type || x.type != z.type) {
        sp_set_error("Not supported point field type");
        return SP_ERR_RUNTIME;
    }
    auto keep = [](Slot s, bool wanted, std::initializer_list<int> types) {
        bool ok = wanted && s.offset >= 0;
        if (ok) {
            ok = false;
            for (int t : types) ok = ok || s.type == t;
        }
        return ok ? s : Slot{};
    };
    // a UINT16 reflectivity takes the intensity's place; any other type leaves the intensity field in charge (:112-121)
    if (convert_intensity && use_reflectivity_as_intensity && reflectivity.offset >= 0 && reflectivity.type == SP_PC2_UINT16)
        intensity = reflectivity;
    rgb = keep(rgb, convert_rgb != 0, {SP_PC2_FLOAT32, SP_PC2_UINT32});
    intensity = keep(intensity, convert_intensity != 0, {SP_PC2_FLOAT32, SP_PC2_UINT16});
    timestamp = keep(timestamp, true, {SP_PC2_FLOAT32, SP_PC2_FLOAT64, SP_PC2_UINT32});
    for (const Slot* s : {&x, &y, &z, &rgb, &intensity, &timestamp})
        if (s->offset >= 0 && !field_inside(s->offset, s->type, point_step)) {
            sp_set_error("[sp_pc2_resolve_fields_host] invalid argument (a field runs past point_step)");
            return SP_ERR_INVALID_ARGUMENT;
        }
    sp_pc2_layout L{};
    L.point_step = point_step;
    L.x_offset = x.offset; L.y_offset = y.offset; L.z_offset = z.offset;
    L.rgb_offset = rgb.offset; L.intensity_offset = intensity.offset; L.timestamp_offset = timestamp.offset;
    L.xyz_type = x.type; L.rgb_type = rgb.type; L.intensity_type = intensity.type; L.timestamp_type = timestamp.type;
    L.start_time_ms = 0.0;
    *layout_out = L;
    return SP_OK;
}

extern "C" size_t sp_pc2_unpack_workspace_bytes(size_t n) { return (size_t)sp::div_up(n, sp::kPc2Points) * sizeof(unsigned long long); }

extern "C" int sp_pc2_unpack(const void* data_dev, size_t data_bytes, size_t n, const sp_pc2_layout* layout, float* points_out,
                             float* rgb_out, float* intensities_out, float* timestamps_out, double* max_offset_ms_dev, void* workspace,
                             void* stream) {
    using namespace sp;
    if (!layout) {
        sp_set_error("[sp_pc2_unpack] invalid argument (null layout)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return SP_OK;
    const sp_pc2_layout& L = *layout;
    const bool has_rgb = L.rgb_offset >= 0, has_int = L.intensity_offset >= 0, has_ts = L.timestamp_offset >= 0;
    const bool ok =
        data_dev && aligned16(data_dev) && points_out && n < (size_t(1) << 32) && L.point_step >= 1 &&
        L.point_step <= SP_PC2_MAX_POINT_STEP && n * (size_t)L.point_step <= data_bytes &&
        (L.xyz_type == SP_PC2_FLOAT32 || L.xyz_type == SP_PC2_FLOAT64) && field_inside(L.x_offset, L.xyz_type, L.point_step) &&
        field_inside(L.y_offset, L.xyz_type, L.point_step) && field_inside(L.z_offset, L.xyz_type, L.point_step) &&
        (!has_rgb || (rgb_out && (L.rgb_type == SP_PC2_FLOAT32 || L.rgb_type == SP_PC2_UINT32) &&
                      field_inside(L.rgb_offset, L.rgb_type, L.point_step))) &&
        (!has_int || (intensities_out && (L.intensity_type == SP_PC2_FLOAT32 || L.intensity_type == SP_PC2_UINT16) &&
                      field_inside(L.intensity_offset, L.intensity_type, L.point_step))) &&
        (!has_ts || (timestamps_out && max_offset_ms_dev && workspace && aligned16(workspace) &&
                     (L.timestamp_type == SP_PC2_FLOAT32 || L.timestamp_type == SP_PC2_FLOAT64 || L.timestamp_type == SP_PC2_UINT32) &&
                     field_inside(L.timestamp_offset, L.timestamp_type, L.point_step))) &&
        std::isfinite(L.start_time_ms);
    if (!ok) {
        sp_set_error("[sp_pc2_unpack] invalid argument (a null or not 16-byte aligned data_dev, a null output of a present attribute, "
                     "a null or not aligned workspace with a time stamp field, point_step == 0 or > SP_PC2_MAX_POINT_STEP, n * point_step > data_bytes, n >= 2^32, an unsupported field type, a "
                     "field running past point_step, or a start_time_ms that is not finite)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    pc2_unpack_kernel<<<div_up(n, kPc2Points), kBlock, stage_bytes(L.point_step), st>>>(
        static_cast<const uint8_t*>(data_dev), (unsigned)n, L, reinterpret_cast<float4*>(points_out), reinterpret_cast<float4*>(rgb_out),
        intensities_out, timestamps_out, static_cast<unsigned long long*>(workspace));
    if (has_ts)
        pc2_max_kernel<<<1, 1024, 0, st>>>(static_cast<const unsigned long long*>(workspace), div_up(n, kPc2Points),
                                           reinterpret_cast<unsigned long long*>(max_offset_ms_dev));
    return launch_status();
}

extern "C" uint32_t sp_pc2_pack_point_step(int has_rgb, int has_intensity, int has_timestamp) {
    return 16u + (has_rgb ? 4u : 0u) + (has_intensity ? 4u : 0u) + (has_timestamp ? 8u : 0u);
}

extern "C" int sp_pc2_pack(const float* points, const float* rgb, const float* intensities, const float* timestamps, size_t n,
                           double start_time_ms, void* data_out_dev, void* stream) {
    using namespace sp;
    if (!points || !data_out_dev || !aligned16(data_out_dev) || n >= (size_t(1) << 32)) {
        sp_set_error("[sp_pc2_pack] invalid argument (a null points or data_out_dev, a data_out_dev that is not 16-byte aligned, or "
                     "n >= 2^32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return SP_OK;
    const unsigned step = sp_pc2_pack_point_step(rgb != nullptr, intensities != nullptr, timestamps != nullptr);
    pc2_pack_kernel<<<div_up(n, kPc2Points), kBlock, (size_t)kPc2Points * step, as_stream(stream)>>>(
        reinterpret_cast<const float4*>(points), reinterpret_cast<const float4*>(rgb), intensities, timestamps, (unsigned)n,
        start_time_ms, step, static_cast<uint8_t*>(data_out_dev));
    return launch_status();
}

extern "C" size_t sp_enhanced_reflectivity_workspace_bytes(size_t n) {
    return n == 0 ? 0 : (size_t)sp::er_blocks(n) * 3 * sp::kRings * sizeof(uint32_t);
}

extern "C" int sp_enhanced_reflectivity(const float* points, float* intensities_inout, size_t n, const void* data_dev,
                                        uint32_t point_step, int32_t ring_offset, int ring_is_u8, int32_t ambient_offset,
                                        void* state_dev, float ema_alpha, float clip_max, void* workspace, void* stream) {
    using namespace sp;
    if (n == 0) return SP_OK;
    if (!points || !intensities_inout || !data_dev || !aligned16(data_dev) || !state_dev || !workspace || !aligned16(workspace) ||
        n >= (size_t(1) << 32) || point_step < 1 || point_step > SP_PC2_MAX_POINT_STEP ||
        !field_inside(ring_offset, ring_is_u8 ? SP_PC2_UINT8 : SP_PC2_UINT16, point_step) ||
        !field_inside(ambient_offset, SP_PC2_UINT16, point_step)) {
        sp_set_error("[sp_enhanced_reflectivity] invalid argument (a null pointer, a data_dev or workspace that is not 16-byte aligned, "
                     "point_step == 0 or > SP_PC2_MAX_POINT_STEP, a ring or ambient field running past point_step, or n >= 2^32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    const ErFields F{point_step, (unsigned)ring_offset, (unsigned)ambient_offset, ring_is_u8 ? 1 : 0};
    const unsigned span = er_span(n), blocks = er_blocks(n);
    const uint8_t* data = static_cast<const uint8_t*>(data_dev);
    const float4* p4 = reinterpret_cast<const float4*>(points);
    uint32_t* partials = static_cast<uint32_t*>(workspace);
    er_partials_kernel<<<blocks, kBlock, kErLaneArrays + stage_bytes(point_step), st>>>(p4, intensities_inout, (unsigned)n, data, F, span,
                                                                                        partials);
    er_update_kernel<<<1, kErSlices * kRings, 0, st>>>(partials, blocks, static_cast<uint32_t*>(state_dev), ema_alpha);
    er_apply_kernel<<<div_up(n, kPc2Points), kBlock, stage_bytes(point_step), st>>>(p4, intensities_inout, (unsigned)n, data, F,
                                                                                   static_cast<const float*>(state_dev), clip_max);
    return launch_status();
}
