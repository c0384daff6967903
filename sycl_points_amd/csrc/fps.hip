// Farthest point sampling on the device: PreprocessFilter::farthest_point_sampling
// (filter/preprocess_operator/farthest_point_sampling_operator.hpp:27-91). The reference runs one parallel_for per sample,
// waits for it and takes std::max_element over all N distances on the host: sampling_num host round trips, each moving N
// floats. Here the whole chain of argmax decisions stays on the device, in one of three forms that give the same bits:
//   one workgroup  n <= 16384: 1024 lanes keep up to 16 points each and their minimum distances in VGPRs; a sample is an
//                  update, a wave argmax by DPP, one LDS slot per wave and ONE barrier. One launch for the whole sample.
//   persistent     n <= 256 CUs x 8192: the one-workgroup step in every workgroup of a grid of at most one workgroup per CU,
//                  points register-resident; each workgroup publishes its winner as six tagged 8-byte granules, every
//                  workgroup polls all records and reduces them the same way, so all take the same decision with no
//                  broadcast. One launch. Every wait is bounded by wall_clock64: a wait that runs out sets the status word
//                  (sp_fps_status), never a silent wrong selection. Taken under the persistent-launch guard only.
//   per sample     any n: the minimum distances live in HBM; a launch per sample updates them and finds its argmax, the
//                  last-arriving workgroup reduces the per-workgroup keys and stores the next index, which the next launch
//                  reads. No host round trip, no wait between workgroups (a ticket, not a barrier): graph-capturable. Used
//                  under stream capture, when the guard is held by another stream, after a timed-out persistent launch and
//                  above the persistent form's capacity.
// Rules pinned to the reference (every form):
//   distance  frobenius_norm_squared<4>(subtract<4,1>(p[gid], p[sel])) (utils/eigen_utils.hpp:245-253, :333-335): dot<4> is
//             the fma chain fma(dw,dw, fma(dz,dz, fma(dy,dy, fma(dx,dx, 0)))) over all FOUR components (w included, unlike
//             sp_math.h's dist2), point minus selected.
//   update    d[gid] = sycl::min(d[gid], dist) (farthest_point_sampling_operator.hpp:71) by the library's pinned rule
//             (y < x) ? y : x with x the old value: a NaN distance keeps the old value, so d never holds NaN.
//   argmax    std::max_element (:77-83) returns the FIRST maximum: the lowest index wins a tie. d is +0 .. FLT_MAX (never NaN,
//             never -0: a sum of squares from +0), so the 64-bit key (float bits of d) << 32 | (0xffffffff - index) orders as
//             the reference does, and a maximum over keys is the same whatever order it is taken in.
//   start     d[] = FLT_MAX (:47); the first index is the caller's (the reference draws it from its own mt19937, :51-53).
#include <algorithm>
#include <atomic>
#include <cfloat>

#include "sp_common.h"
#include "sp_internal.h"

void sp_set_error(const char* msg);

namespace sp {
struct PersistGuard;  // registration.hip: one persistent launch at a time per device (registration_device.h)
PersistGuard* persist_acquire(hipStream_t st, unsigned grid);
void persist_release(PersistGuard* g, hipStream_t st);

namespace {

constexpr int kFpsBlock = 1024;                                   // one-workgroup form: 16 waves
constexpr int kFpsWaves = kFpsBlock / kWave;
constexpr int kFpsMaxPer = 16;                                    // points per lane: 5 VGPRs each, 80 of the 128 a 1024-lane workgroup has
constexpr size_t kFpsOneWgCap = (size_t)kFpsBlock * kFpsMaxPer;   // 16384 points
constexpr int kStepBlock = 256;                                   // per-sample form
constexpr unsigned kStepMaxGrid = 4096;                           // (room for the grid sweep of the timing script)
constexpr unsigned kStepGrid = 256;                               // default grid cap of the per-sample form: measured, DESIGN §4.5
constexpr int kPersistMaxGrid = kNumCU;                           // persistent form: at most one workgroup per CU
constexpr int kPersistMaxPer = 8;                                 // (16 points per lane spill beside the record poll)
constexpr size_t kPersistCap = (size_t)kPersistMaxGrid * kFpsBlock * kPersistMaxPer;  // 2 M points
constexpr int kRecordWords = 8;                                   // a record: 6 granules {value, tag} (+2 unused)
constexpr unsigned long long kFpsBudget = 50ull * 100000ull;      // 50 ms of wall_clock64 (100 MHz) per wait
// workspace: FpsState | per-sample keys [kStepMaxGrid] | persistent records [2][kPersistMaxGrid][8] | d[n]
constexpr size_t kPartialOffset = 256;
constexpr size_t kRecordOffset = kPartialOffset + (size_t)kStepMaxGrid * 8;
constexpr size_t kDistOffset = kRecordOffset + 2 * (size_t)kPersistMaxGrid * kRecordWords * 8;

struct FpsState {
    unsigned ticket;   // arrivals of the current per-sample launch (the last arriver resets it)
    unsigned sel[2];   // the index chosen by launch `it` is sel[it & 1]; sel[0] starts as the first index
    unsigned status;   // 0, or 2: a wait of the persistent form ran out (sp_fps_status); zeroed by every call
};

typedef unsigned long long u64;

__device__ __forceinline__ float fps_d2(const float4 p, const float4 s) {
    const float dx = p.x - s.x, dy = p.y - s.y, dz = p.z - s.z, dw = p.w - s.w;
    return fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, 0.0f))));
}
__device__ __forceinline__ float fps_min(float x, float y) { return (y < x) ? y : x; }  // sycl::min(x, y), DESIGN §2
__device__ __forceinline__ u64 fps_key(float d, unsigned i) { return ((u64)__float_as_uint(d) << 32) | (0xffffffffu - i); }

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u64 dpp_u64_or_zero(u64 x) {
    const unsigned lo = (unsigned)dpp_or_zero<CTRL, ROW_MASK>((int)(unsigned)x);
    const unsigned hi = (unsigned)dpp_or_zero<CTRL, ROW_MASK>((int)(unsigned)(x >> 32));
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 max_u64(u64 a, u64 b) { return a > b ? a : b; }
// Maximum key of the wave, in every lane: wave_sum_to_lane63's DPP ladder with max for +, then lane 63 read back. Every lane of
// the wave must be active. 0 (what a lane outside a row reads) is below every key of a point.
__device__ __forceinline__ u64 wave_max_key(u64 k) {
    k = max_u64(k, dpp_u64_or_zero<0x111, 0xf>(k));  // row_shr:1
    k = max_u64(k, dpp_u64_or_zero<0x112, 0xf>(k));  // row_shr:2
    k = max_u64(k, dpp_u64_or_zero<0x114, 0xf>(k));  // row_shr:4
    k = max_u64(k, dpp_u64_or_zero<0x118, 0xf>(k));  // row_shr:8
    k = max_u64(k, dpp_u64_or_zero<0x142, 0xa>(k));  // row_bcast:15
    k = max_u64(k, dpp_u64_or_zero<0x143, 0xc>(k));  // row_bcast:31
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
    return ((u64)hi << 32) | lo;
}

struct alignas(16) FpsSlot {  // a wave's winner of one sample
    u64 key;
    float x, y, z, w;
    unsigned pad[2];
};

// One workgroup, P points per lane: lane t holds points t + k * 1024 (k < P); a lane past n holds (0, 0, 0, 0) with d = +0,
// whose key is below that of every point (same d, higher index) and which no update changes (min(+0, dist >= 0 or NaN) = +0).
// Per sample: update, the lane's first maximum (k ascending = index ascending, strict >), the wave's by DPP, the winning lane
// writes {key, x, y, z, w} to the slot of its wave (double-buffered by sample parity: a slot of parity p is rewritten only after
// the NEXT barrier, which every reader of it has passed), one barrier, and every lane reads the 16 slots: the next point's
// coordinates come from the slot, no global load sits on the dependent chain. Selected points are kept as bits per lane.
template <int P>
__global__ __launch_bounds__(kFpsBlock) void fps_one_wg_kernel(const float4* __restrict__ pts, unsigned n, unsigned S, unsigned first,
                                                               uint32_t* __restrict__ order, uint8_t* __restrict__ flags,
                                                               float* __restrict__ min_d2, FpsState* __restrict__ state) {
    __shared__ FpsSlot slots[2][kFpsWaves];
    const unsigned t = threadIdx.x, wave = t / kWave;
    if (t == 0) state->status = 0u;
    float x[P], y[P], z[P], w[P], d[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const unsigned i = t + (unsigned)k * kFpsBlock;
        float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < n) p = pts[i];
        x[k] = p.x; y[k] = p.y; z[k] = p.z; w[k] = p.w;
        d[k] = i < n ? FLT_MAX : 0.0f;
    }
    float4 s = pts[first];
    unsigned picked = (first % kFpsBlock == t) ? 1u << (first / kFpsBlock) : 0u;
    if (t == 0) order[0] = first;
    for (unsigned it = 1; it < S; ++it) {
        float bd = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
        int bk = 0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            d[k] = fps_min(d[k], fps_d2(make_float4(x[k], y[k], z[k], w[k]), s));
            if (k == 0 || d[k] > bd) { bd = d[k]; bk = k; sx = x[k]; sy = y[k]; sz = z[k]; sw = w[k]; }
        }
        const u64 mine = fps_key(bd, t + (unsigned)bk * kFpsBlock);
        const u64 wk = wave_max_key(mine);
        FpsSlot* const slot = slots[it & 1];
        if (mine == wk) {  // one lane per wave (keys are distinct)
            slot[wave].key = wk;
            slot[wave].x = sx; slot[wave].y = sy; slot[wave].z = sz; slot[wave].w = sw;
        }
        __syncthreads();
        u64 best = slot[0].key;
        int bw = 0;
#pragma unroll
        for (int v = 1; v < kFpsWaves; ++v) {
            const u64 kv = slot[v].key;
            if (kv > best) { best = kv; bw = v; }
        }
        s = make_float4(slot[bw].x, slot[bw].y, slot[bw].z, slot[bw].w);
        const unsigned gi = 0xffffffffu - (unsigned)best;
        if (gi % kFpsBlock == t) picked |= 1u << (gi / kFpsBlock);
        if (t == 0) order[it] = gi;
    }
    unsigned tt = t;
    asm volatile("" : "+v"(tt));  // (the stores' addresses are made here, not held in VGPRs through the sample loop)
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const unsigned i = tt + (unsigned)k * kFpsBlock;
        if (i < n) {
            if (min_d2) min_d2[i] = d[k];
            if (flags) flags[i] = (uint8_t)((picked >> k) & 1u);
        }
    }
}

// Per-sample form, set-up: d[] = FLT_MAX, flags = 0, the state's ticket = 0 and sel[0] = first, order[0] = first.
__global__ __launch_bounds__(kStepBlock) void fps_init_kernel(float* __restrict__ d, uint8_t* __restrict__ flags, unsigned n,
                                                              FpsState* __restrict__ st, unsigned first, uint32_t* __restrict__ order) {
    const unsigned stride = gridDim.x * kStepBlock;
    for (unsigned i = blockIdx.x * kStepBlock + threadIdx.x; i < n; i += stride) {
        d[i] = FLT_MAX;
        if (flags) flags[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->ticket = 0u;
        st->status = 0u;
        st->sel[0] = first;
        st->sel[1] = first;
        order[0] = first;
    }
}

// Maximum key of a 256-lane workgroup, valid in thread 0 (every thread must call it).
__device__ __forceinline__ u64 block_max_key(u64 k, u64* s_keys) {
    const u64 wk = wave_max_key(k);
    if ((threadIdx.x & (kWave - 1)) == 0) s_keys[threadIdx.x / kWave] = wk;
    __syncthreads();
    u64 b = s_keys[0];
#pragma unroll
    for (int v = 1; v < kStepBlock / kWave; ++v) b = max_u64(b, s_keys[v]);
    return b;
}

// Per-sample form, sample `it` (1 <= it < S): the update by the point chosen by launch it - 1 (sel[(it - 1) & 1]; sel[0] = the
// first index for it = 1), the workgroup's first maximum, then the ticket: each workgroup stores its key (one 8-byte store at
// agent scope), releases, counts in; the last to arrive acquires, reads every key (the maximum is the same in any order) and
// stores the next index to sel[it & 1] and order[it], and resets the ticket for the next launch.
__global__ __launch_bounds__(kStepBlock) void fps_step_kernel(const float4* __restrict__ pts, unsigned n, float* __restrict__ d,
                                                              FpsState* st, u64* partial, unsigned it, uint32_t* __restrict__ order) {
    __shared__ u64 s_keys[kStepBlock / kWave];
    __shared__ unsigned s_last;
    const float4 s = pts[st->sel[(it - 1) & 1]];
    const unsigned stride = gridDim.x * kStepBlock;
    u64 best = 0;
    for (unsigned i = blockIdx.x * kStepBlock + threadIdx.x; i < n; i += stride) {  // index ascending: strict > keeps the first
        const float v = fps_min(d[i], fps_d2(pts[i], s));
        d[i] = v;
        const u64 key = fps_key(v, i);
        if (key > best) best = key;
    }
    const u64 b = block_max_key(best, s_keys);
    if (threadIdx.x == 0) {
        __hip_atomic_store(partial + blockIdx.x, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned prev = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;  // (uniform over the workgroup)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    u64 g = 0;
    for (unsigned j = threadIdx.x; j < gridDim.x; j += kStepBlock)
        g = max_u64(g, __hip_atomic_load(partial + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();  // (s_keys is reused)
    const u64 all = block_max_key(g, s_keys);
    if (threadIdx.x == 0) {
        const unsigned next = 0xffffffffu - (unsigned)all;
        st->sel[it & 1] = next;
        order[it] = next;
        __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Persistent form, set-up: the records of both parities zeroed (a tag is a sample number >= 1, so no zeroed granule matches),
// the status word cleared. Every call re-initialises what its launch polls.
__global__ __launch_bounds__(kStepBlock) void fps_persist_prep_kernel(u64* __restrict__ rec, unsigned words, FpsState* __restrict__ st) {
    for (unsigned i = blockIdx.x * kStepBlock + threadIdx.x; i < words; i += gridDim.x * kStepBlock) rec[i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->status = 0u;
}

// Persistent form: workgroup g holds points g * 1024 * P + t + k * 1024 (the one-workgroup layout, shifted), every workgroup
// resident (the guard and G <= CUs). Per sample: the one-workgroup step gives the workgroup's winner {key, x, y, z, w}; lanes
// 0-5 publish it as six granules {value, tag = sample} (record [sample & 1][g], one 8-byte agent-scope store each: a granule is
// its own flag); lane t < G polls the six granules of record t until every tag of every record matches (__syncthreads_and),
// bounded by `budget` ticks of wall_clock64, with s_sleep between polls; then the maximum key over the records (keys are
// distinct, so every workgroup finds the same one) and the next point's coordinates from the winning record. Records of parity
// p are rewritten two samples later, after every workgroup has read them (it needed this sample's records to publish the next).
// A wait that runs out: status = 2 and the workgroup leaves; the outputs are then incomplete and sp_fps_status says so.
template <int P>
__global__ __launch_bounds__(kFpsBlock) void fps_persistent_kernel(const float4* __restrict__ pts, unsigned n, unsigned S,
                                                                   unsigned first, uint32_t* __restrict__ order,
                                                                   uint8_t* __restrict__ flags, float* __restrict__ min_d2,
                                                                   u64* rec, FpsState* state, unsigned long long budget) {
    __shared__ FpsSlot slots[2][kFpsWaves];
    __shared__ FpsSlot gslots[2][kPersistMaxGrid / kWave];
    __shared__ unsigned s_wait;
    const unsigned t = threadIdx.x, wave = t / kWave, G = gridDim.x, g = blockIdx.x;
    const unsigned base = g * (unsigned)(kFpsBlock * P);
    float x[P], y[P], z[P], w[P], d[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const unsigned i = base + t + (unsigned)k * kFpsBlock;
        float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < n) p = pts[i];
        x[k] = p.x; y[k] = p.y; z[k] = p.z; w[k] = p.w;
        d[k] = i < n ? FLT_MAX : 0.0f;
    }
    float4 s = pts[first];
    unsigned picked = 0u;
    if (first - base < (unsigned)(kFpsBlock * P) && (first - base) % kFpsBlock == t) picked = 1u << ((first - base) / kFpsBlock);
    if (g == 0 && t == 0) order[0] = first;
    for (unsigned it = 1; it < S; ++it) {
        // the workgroup's winner (fps_one_wg_kernel's step)
        float bd = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
        int bk = 0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            d[k] = fps_min(d[k], fps_d2(make_float4(x[k], y[k], z[k], w[k]), s));
            if (k == 0 || d[k] > bd) { bd = d[k]; bk = k; sx = x[k]; sy = y[k]; sz = z[k]; sw = w[k]; }
        }
        const u64 mine = fps_key(bd, base + t + (unsigned)bk * kFpsBlock);
        const u64 wk = wave_max_key(mine);
        FpsSlot* const slot = slots[it & 1];
        if (mine == wk) {
            slot[wave].key = wk;
            slot[wave].x = sx; slot[wave].y = sy; slot[wave].z = sz; slot[wave].w = sw;
        }
        __syncthreads();
        u64 best = slot[0].key;
        int bw = 0;
#pragma unroll
        for (int v = 1; v < kFpsWaves; ++v) {
            const u64 kv = slot[v].key;
            if (kv > best) { best = kv; bw = v; }
        }
        // publish: six granules, one 8-byte store each
        u64* const rows = rec + (size_t)(it & 1) * G * kRecordWords;
        if (t < 6) {
            const unsigned v = t == 0 ? (unsigned)(best >> 32) : t == 1 ? (unsigned)best
                             : __float_as_uint(t == 2 ? slot[bw].x : t == 3 ? slot[bw].y : t == 4 ? slot[bw].z : slot[bw].w);
            __hip_atomic_store(rows + (size_t)g * kRecordWords + t, ((u64)it << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // poll every record until all six tags of all G records match
        unsigned gv[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        const unsigned long long t0 = wall_clock64();
        for (;;) {
            bool ok = true;
            if (t < G) {
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const u64 q = __hip_atomic_load(rows + (size_t)t * kRecordWords + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    gv[j] = (unsigned)q;
                    ok = ok && (unsigned)(q >> 32) == it;
                }
            }
            if (__syncthreads_and(ok ? 1 : 0)) break;
            if (t == 0) s_wait = (wall_clock64() - t0 > budget) ? 1u : 0u;
            __syncthreads();
            if (s_wait) {
                if (t == 0) __hip_atomic_store(&state->status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;  // (uniform: every lane read the same s_wait)
            }
            __builtin_amdgcn_s_sleep(1);
        }
        // the same reduction of the same records in every workgroup
        const u64 k2 = t < G ? (((u64)gv[0] << 32) | gv[1]) : 0ull;
        const u64 wk2 = wave_max_key(k2);
        FpsSlot* const gs = gslots[it & 1];
        if (t < G && k2 == wk2) {
            gs[wave].key = wk2;
            gs[wave].x = __uint_as_float(gv[2]); gs[wave].y = __uint_as_float(gv[3]);
            gs[wave].z = __uint_as_float(gv[4]); gs[wave].w = __uint_as_float(gv[5]);
        }
        __syncthreads();
        const unsigned nw = (G + kWave - 1) / kWave;
        u64 gb = gs[0].key;
        int gw = 0;
#pragma unroll
        for (int v = 1; v < kPersistMaxGrid / kWave; ++v) {
            if ((unsigned)v < nw) {
                const u64 kv = gs[v].key;
                if (kv > gb) { gb = kv; gw = v; }
            }
        }
        s = make_float4(gs[gw].x, gs[gw].y, gs[gw].z, gs[gw].w);
        const unsigned gi = 0xffffffffu - (unsigned)gb;
        if (gi - base < (unsigned)(kFpsBlock * P) && (gi - base) % kFpsBlock == t) picked |= 1u << ((gi - base) / kFpsBlock);
        if (g == 0 && t == 0) order[it] = gi;
    }
    unsigned tt = t;
    asm volatile("" : "+v"(tt));
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const unsigned i = base + tt + (unsigned)k * kFpsBlock;
        if (i < n) {
            if (min_d2) min_d2[i] = d[k];
            if (flags) flags[i] = (uint8_t)((picked >> k) & 1u);
        }
    }
}

// flags[order[j]] = 1 for j < S (flags zeroed by fps_init_kernel)
__global__ __launch_bounds__(kStepBlock) void fps_flags_kernel(const uint32_t* __restrict__ order, unsigned S, unsigned n,
                                                               uint8_t* __restrict__ flags) {
    const unsigned j = blockIdx.x * kStepBlock + threadIdx.x;
    if (j < S) {
        const unsigned i = order[j];
        if (i < n) flags[i] = 1;
    }
}

template <int P>
void launch_one_wg(const float4* pts, unsigned n, unsigned S, unsigned first, uint32_t* order, uint8_t* flags, float* min_d2,
                   FpsState* state, hipStream_t st) {
    fps_one_wg_kernel<P><<<1, kFpsBlock, 0, st>>>(pts, n, S, first, order, flags, min_d2, state);
}
template <int P>
void launch_persistent(unsigned G, const float4* pts, unsigned n, unsigned S, unsigned first, uint32_t* order, uint8_t* flags,
                       float* min_d2, u64* rec, FpsState* state, hipStream_t st) {
    fps_persistent_kernel<P><<<G, kFpsBlock, 0, st>>>(pts, n, S, first, order, flags, min_d2, rec, state, kFpsBudget);
}

// One-shot latch per device: sp_fps_status saw a persistent launch run out of its wait budget, so the next automatic choice on
// that device takes the per-sample form (the facade re-runs at once).
constexpr int kMaxFpsDevices = 64;
std::atomic<int> g_avoid_persistent[kMaxFpsDevices];
int current_device() {
    int dev = 0;
    return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxFpsDevices) ? dev : -1;
}

// Points per lane of the persistent form: the smallest P that needs at most 64 workgroups, else the most points per lane. Measured
// (DESIGN §4.5): more records to poll cost more than longer steps — 1 M points take 4.1 us per sample in 128 workgroups of 8
// points per lane against 6.1 us in 256 of 4; at 70 k, 35 workgroups of 2 beat 69 of 1 by 5 %.
int persistent_per_lane(size_t n) {
    for (int P = 1; P <= kPersistMaxPer; P *= 2)
        if (div_up(n, (size_t)kFpsBlock * P) <= 64u) return P;
    return div_up(n, (size_t)kFpsBlock * kPersistMaxPer) <= (unsigned)kPersistMaxGrid ? kPersistMaxPer : 0;
}

int fps_run(int form, const float* points, size_t n, size_t sampling_num, uint32_t first_index, uint32_t* order_out,
            uint8_t* flags_out_opt, float* min_d2_out_opt, void* workspace, size_t workspace_bytes, void* stream) {
    // form: low byte 0 auto, 1 one workgroup, 2 per sample, 3 persistent; second byte a knob for the timing script: the
    // per-sample grid cap in units of 256 workgroups, or the persistent form's points per lane (0: the library's choice)
    const int knob = form >> 8;
    form &= 0xff;
    const bool bad_knob = knob < 0 || (form == 2 && knob * 256 > (int)kStepMaxGrid) ||
                          (form == 3 && knob != 0 && (knob > kPersistMaxPer || (knob & (knob - 1)) != 0 ||
                                                      div_up(n, (size_t)kFpsBlock * knob) > (unsigned)kPersistMaxGrid)) ||
                          (form != 2 && form != 3 && knob != 0);
    if (n == 0 || !points || !order_out || !workspace || first_index >= n || sampling_num == 0 || sampling_num > n ||
        n >= ((size_t)1 << 32) || workspace_bytes < sp_fps_workspace_bytes(n, sampling_num) || form < 0 || form > 3 || bad_knob ||
        (form == 1 && n > kFpsOneWgCap) || (form == 3 && n > kPersistCap)) {
        sp_set_error("[sp_farthest_point_sampling] invalid argument (n == 0 or >= 2^32, a null pointer, first_index >= n, "
                     "sampling_num == 0 or > n, a workspace smaller than sp_fps_workspace_bytes, or a form that cannot take n)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    const float4* pts = reinterpret_cast<const float4*>(points);
    const unsigned N = (unsigned)n, S = (unsigned)sampling_num;
    char* ws = static_cast<char*>(workspace);
    FpsState* state = reinterpret_cast<FpsState*>(ws);
    const bool forced = form != 0;
    if (form == 0) {
        const int dev = current_device();
        const bool avoid = dev >= 0 && g_avoid_persistent[dev].exchange(0) != 0;
        form = n <= kFpsOneWgCap ? 1 : (n <= kPersistCap && !avoid) ? 3 : 2;
    }
    if (form == 1) {
        const size_t per = (n + kFpsBlock - 1) / kFpsBlock;
        if (per <= 1) launch_one_wg<1>(pts, N, S, first_index, order_out, flags_out_opt, min_d2_out_opt, state, st);
        else if (per <= 2) launch_one_wg<2>(pts, N, S, first_index, order_out, flags_out_opt, min_d2_out_opt, state, st);
        else if (per <= 4) launch_one_wg<4>(pts, N, S, first_index, order_out, flags_out_opt, min_d2_out_opt, state, st);
        else if (per <= 8) launch_one_wg<8>(pts, N, S, first_index, order_out, flags_out_opt, min_d2_out_opt, state, st);
        else launch_one_wg<16>(pts, N, S, first_index, order_out, flags_out_opt, min_d2_out_opt, state, st);
        return launch_status();
    }
    if (form == 3) {
        const int P = knob ? knob : persistent_per_lane(n);
        const unsigned G = div_up(n, (size_t)kFpsBlock * P);
        // the guard first: no other stream's persistent launch (GICP or FPS) may still be running, the stream is not capturing,
        // and G fits the device's CUs; check and launch are one critical section
        PersistGuard* const guard = persist_acquire(st, G);
        if (guard) {
            u64* rec = reinterpret_cast<u64*>(ws + kRecordOffset);
            fps_persist_prep_kernel<<<1, kStepBlock, 0, st>>>(rec, 2u * G * kRecordWords, state);
            switch (P) {
                case 1: launch_persistent<1>(G, pts, N, S, first_index, order_out, flags_out_opt, min_d2_out_opt, rec, state, st); break;
                case 2: launch_persistent<2>(G, pts, N, S, first_index, order_out, flags_out_opt, min_d2_out_opt, rec, state, st); break;
                case 4: launch_persistent<4>(G, pts, N, S, first_index, order_out, flags_out_opt, min_d2_out_opt, rec, state, st); break;
                default: launch_persistent<8>(G, pts, N, S, first_index, order_out, flags_out_opt, min_d2_out_opt, rec, state, st); break;
            }
            const int rc = launch_status();
            persist_release(guard, st);
            return rc;
        }
        if (forced) {
            sp_set_error("[sp_farthest_point_sampling] the persistent form is not available now (stream capturing, another stream's "
                         "persistent launch may still run, or the grid exceeds the device's compute units)");
            return SP_ERR_RUNTIME;
        }
        form = 2;
    }
    u64* partial = reinterpret_cast<u64*>(ws + kPartialOffset);
    float* d = min_d2_out_opt ? min_d2_out_opt : reinterpret_cast<float*>(ws + kDistOffset);
    const unsigned cap = knob ? (unsigned)knob * 256u : kStepGrid;
    const unsigned grid = (unsigned)std::min<size_t>(div_up(n, kStepBlock), cap);
    fps_init_kernel<<<grid, kStepBlock, 0, st>>>(d, flags_out_opt, N, state, first_index, order_out);
    for (unsigned it = 1; it < S; ++it)
        fps_step_kernel<<<grid, kStepBlock, 0, st>>>(pts, N, d, state, partial, it, order_out);
    if (flags_out_opt) fps_flags_kernel<<<div_up(S, kStepBlock), kStepBlock, 0, st>>>(order_out, S, N, flags_out_opt);
    return launch_status();
}

}  // namespace
}  // namespace sp

extern "C" size_t sp_fps_workspace_bytes(size_t n, size_t sampling_num) {
    (void)sampling_num;
    return sp::kDistOffset + ((n * sizeof(float) + 255) & ~(size_t)255);
}

extern "C" int sp_fps_status(const void* workspace, void* stream) {
    if (!workspace) return SP_ERR_INVALID_ARGUMENT;
    unsigned status = 0;
    hipStream_t st = sp::as_stream(stream);
    const sp::FpsState* state = static_cast<const sp::FpsState*>(workspace);
    if (hipMemcpyAsync(&status, &state->status, sizeof status, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return SP_ERR_HIP;
    if (status == 2u) {
        const int dev = sp::current_device();
        if (dev >= 0) sp::g_avoid_persistent[dev].store(1);
        sp_set_error("[sp_farthest_point_sampling] a wait of the persistent form ran into its time limit (not every workgroup was "
                     "resident: another process or a CU-masked stream holds compute units); the sample is incomplete. The next "
                     "call on this device takes the per-sample form: call again");
        return SP_ERR_RUNTIME;
    }
    return SP_OK;
}

extern "C" int sp_farthest_point_sampling(const float* points, size_t n, size_t sampling_num, uint32_t first_index,
                                          uint32_t* order_out, uint8_t* flags_out_opt, float* min_d2_out_opt, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    return sp::fps_run(0, points, n, sampling_num, first_index, order_out, flags_out_opt, min_d2_out_opt, workspace,
                       workspace_bytes, stream);
}

extern "C" int sp_internal_fps(int form, const float* points, size_t n, size_t sampling_num, uint32_t first_index,
                               uint32_t* order_out, uint8_t* flags_out_opt, float* min_d2_out_opt, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return sp::fps_run(form, points, n, sampling_num, first_index, order_out, flags_out_opt, min_d2_out_opt, workspace,
                       workspace_bytes, stream);
}
