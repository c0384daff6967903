// Shared launch helpers for the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/sycl_points_amd.h"

namespace sp {

constexpr int kWave = 64;            // gfx950 wavefront
constexpr int kNumCU = 256;          // MI355X
constexpr int kBlock = 256;          // default workgroup: 4 waves, one per SIMD

inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }

inline int hip_status(hipError_t e) { return e == hipSuccess ? SP_OK : SP_ERR_HIP; }

// Launch-time check: converts a failed launch into SP_ERR_HIP (no sync; graph-capture safe). It also reports, once, a
// failure a KERNEL of an earlier call raised through device_error_word() — by then the call that hit it has returned
// SP_OK, so the message names the kernel and says so (capi_common.hip).
int launch_status();
// One word of pinned host memory per process that kernels can write (system scope) when a "cannot happen" guard trips — a
// look-back poll that ran out (sp_lookback.h) — so that it is not lost: nullptr when the allocation failed (no device).
unsigned* device_error_word();
constexpr unsigned kDevErrLookback = 1u;
constexpr unsigned kDevErrBounds = 2u;  // sp_grid_create_bounded: a finite point outside the bounds the caller vouched for

inline unsigned div_up(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// Grid for a memory-bound grid-stride kernel: enough workgroups to fill 256 CUs x 8, no more.
inline unsigned stream_grid(size_t n, int block = kBlock, int per_thread = 1) {
    const size_t want = (n + (size_t)block * per_thread - 1) / ((size_t)block * per_thread);
    const size_t cap = (size_t)kNumCU * 8;
    return (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
}

// Zero `bytes` bytes (a multiple of 4) at p with a KERNEL. Every enqueue-only entry point uses this instead of
// hipMemsetAsync: on ROCm 7.2 a memset NODE of a captured hipGraph was observed (tests/test_gpu_multirank.py, the fan-in
// ticket counter; also the 64 KB row reset of the rows_all_reduced = 1 loop) not to be ordered before the kernel node that
// follows it in the captured stream when the graph is replayed — eager launches and the first replay hide it.
int zero_async(void* p, size_t bytes, hipStream_t st);  // capi_common.hip; returns SP_OK / SP_ERR_HIP
// true when sp_knn_bruteforce answers nq queries against nt targets by its one launch that keeps the targets in LDS
// (knn_bruteforce.hip; sp_knn_tree's backend rule asks it too).
bool small_applies(size_t nq, size_t nt);

// Device scratch for the structure builds (sp_grid_create and friends): the temporaries of a build (sort keys, rocPRIM
// workspaces, a few counters) are idle again when the build returns (it synchronises its stream), so they are kept and
// handed to the next build instead of going back to hipFree / hipMalloc, which cost ~0.1 ms apiece on this runtime
// (eleven of them made a 1M-point grid build 1.9 ms for 0.2 ms of kernels). Bounded: at most kKeep idle buffers are kept,
// the smallest is dropped first. The arrays of objects that outlive the call (a grid, a prepared target) come from the same
// pool through pooled_alloc / pooled_free: their destroy waits for the device to go idle (what hipFree does implicitly)
// before the buffers are offered to the next build.
hipError_t scratch_acquire(void** ptr, size_t bytes, hipStream_t st = nullptr);  // capi_common.hip; st: the stream the buffer will be used on (a buffer released behind the same stream's work is taken without waiting)
void* pinned_mailbox();  // capi_common.hip: 256 bytes of pinned host memory per host thread (nullptr: none), for small read-backs
void scratch_release(void* ptr);
template <class T> hipError_t pooled_alloc(T** ptr, size_t bytes, hipStream_t st = nullptr) { return scratch_acquire(reinterpret_cast<void**>(ptr), bytes, st); }
inline void pooled_free(void* ptr) { if (ptr) scratch_release(ptr); }  // caller: nothing on the device still uses ptr

// The streams an object's arrays have been used on (every entry point notes its stream): when the object is destroyed its
// buffers go back to the pool TAGGED with one event per stream (recorded then), and the pool hands a buffer out again only
// once its events have completed — no hipDeviceSynchronize in a destructor, so destroying an object neither stalls other
// streams nor breaks a stream capture that is running beside it. More than kMax distinct streams: the destroy path falls
// back to the device-wide wait.
struct StreamSet {
    static constexpr int kMax = 8;
    hipStream_t s[kMax];
    int n = 0;
    bool overflow = false;
    void note(hipStream_t st) {
        for (int i = 0; i < n; ++i)
            if (s[i] == st) return;
        if (n < kMax) s[n++] = st; else overflow = true;
    }
    void merge(const StreamSet& o) {
        for (int i = 0; i < o.n; ++i) note(o.s[i]);
        overflow = overflow || o.overflow;
    }
};
void scratch_release_after(void* ptr, const StreamSet& streams);  // capi_common.hip
inline void pooled_free_after(void* ptr, const StreamSet& streams) { if (ptr) scratch_release_after(ptr, streams); }
struct ScratchBuf {  // RAII handle
    void* p = nullptr;
    hipError_t get(size_t bytes, hipStream_t st = nullptr) { return scratch_acquire(&p, bytes, st); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    ~ScratchBuf() { if (p) scratch_release(p); }
    /// hand the buffer back while work on `streams` may still use it (the pool waits for their events before reuse)
    void release_after(const StreamSet& streams) { if (p) { scratch_release_after(p, streams); p = nullptr; } }
    ScratchBuf() = default;
    ScratchBuf(const ScratchBuf&) = delete;
    ScratchBuf& operator=(const ScratchBuf&) = delete;
};

// wave64 butterfly sum; every lane ends with the total.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// wave64 sum delivered to lane 63 only, on the VALU's DPP path (no LDS crossbar): an inclusive scan inside each row of 16
// lanes (row_shr 1, 2, 4, 8; lanes shifted in from outside the row read 0), then row_bcast:15 into rows 1 and 3 and
// row_bcast:31 into rows 2 and 3. `__shfl_xor` costs a ds_bpermute per step (measured: the 28-value workgroup reduction at
// the end of the GICP kernels took 6 us of a 27 us launch with it). Fixed tree: reproducible.
// The tree that reaches lane 63 is perfectly balanced with xor pairing: inside a row, row_shr 1, 2, 4, 8 make lane 15 add lanes
// that differ in bit 0, then bit 1, bit 2, bit 3 (lane 15 never reads a shifted-in zero); row_bcast:15 adds row 0 into row 1 and
// row 2 into row 3 (bit 4), row_bcast:31 adds (r0 + r1) into (r2 + r3) (bit 5). Float addition is commutative bit for bit, so
// ANY network that performs the same pairings level by level, in the order xor 1, 2, 4, 8, 16, 32, yields the same bits
// (NaN payloads aside): wave_reduce_transposed below is one, for many values at once. These two serve single values.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_or_zero(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xf, true);
}
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
    v += __int_as_float(dpp_or_zero<0x111, 0xf>(__float_as_int(v)));  // row_shr:1
    v += __int_as_float(dpp_or_zero<0x112, 0xf>(__float_as_int(v)));  // row_shr:2
    v += __int_as_float(dpp_or_zero<0x114, 0xf>(__float_as_int(v)));  // row_shr:4
    v += __int_as_float(dpp_or_zero<0x118, 0xf>(__float_as_int(v)));  // row_shr:8   -> lane 15 of every row: the row total
    v += __int_as_float(dpp_or_zero<0x142, 0xa>(__float_as_int(v)));  // row_bcast:15 -> rows 1 and 3 add the row before
    v += __int_as_float(dpp_or_zero<0x143, 0xc>(__float_as_int(v)));  // row_bcast:31 -> rows 2 and 3 add lane 31
    return v;                                                          // lane 63: the wave total
}
__device__ __forceinline__ unsigned wave_sum_u32_to_lane63(unsigned v) {
    v += (unsigned)dpp_or_zero<0x111, 0xf>((int)v);
    v += (unsigned)dpp_or_zero<0x112, 0xf>((int)v);
    v += (unsigned)dpp_or_zero<0x114, 0xf>((int)v);
    v += (unsigned)dpp_or_zero<0x118, 0xf>((int)v);
    v += (unsigned)dpp_or_zero<0x142, 0xa>((int)v);
    v += (unsigned)dpp_or_zero<0x143, 0xc>((int)v);
    return v;
}

// The same tree for NV values of a lane at once, transposed ("halving"): at the level of lane bit L a lane keeps half of its
// live values and sends the other half to lane ^ (1 << L). The live values are taken in pairs (a, b): the lane whose bit L is 0
// ends with a_own + a_partner, the lane whose bit is 1 with b_own + b_partner; an odd value out takes the plain butterfly step
// of that level (both lanes end with the pair sum). m live values become m / 2 + (m & 1), so NV <= 32 values are one value per
// lane after the xor 16 level, and the xor 32 step leaves that value's wave total in both halves. 28 values cost
// 14 + 7 + 4 + 2 + 1 + 1 = 29 pair steps where wave_sum_to_lane63 costs 28 x 6, and every total is the ladder's, bit for bit.
// Value -> lane: wave_transposed_value(NV, lane) is the index of the value whose total `lane` holds. Reading the levels
// backwards from the single value that is left, position p' of the level above came from the pair (2 p', 2 p' + 1), of which
// the lane's bit chose one, or from the odd value out. For NV = 28 that is lane & 31 for lanes & 31 below 28 (bit 0 chose
// inside a pair of values, bit 1 inside a pair of pairs, ...), and lanes 28 .. 31 of each half repeat 24 .. 27; for two values
// it is lane & 1.
// The moves: quad_perm [1,0,3,2], quad_perm [2,3,0,1] and row_ror:8 (xor 1, 2, 8) fold into the add; xor 4 is a move by
// quad_perm [3,2,1,0] and row_half_mirror folded into the add (two instructions; row_shl:4 into banks 0 and 2 plus row_shr:4 into
// banks 1 and 3 does not fold and costs four); xor 16 and xor 32 are v_permlane16_swap / v_permlane32_swap of (a, b),
// after which one add of the two registers IS the keep / send selection (a single value is swapped with a copy of itself).
__host__ __device__ constexpr int wave_transposed_value(int nv, unsigned lane) {
    int m[7] = {nv, 0, 0, 0, 0, 0, 0};
    for (int l = 0; l < 6; ++l) m[l + 1] = m[l] / 2 + (m[l] & 1);
    int p = 0;
    for (int l = 5; l >= 0; --l) p = p < m[l] / 2 ? 2 * p + (int)((lane >> l) & 1u) : m[l] - 1;
    return p;
}
__device__ __forceinline__ int wave_word(float v) { return __float_as_int(v); }
__device__ __forceinline__ int wave_word(unsigned v) { return (int)v; }
__device__ __forceinline__ void wave_unword(int w, float& v) { v = __int_as_float(w); }
__device__ __forceinline__ void wave_unword(int w, unsigned& v) { v = (unsigned)w; }
// x of lane ^ (1 << LEVEL), LEVEL 0 .. 3 (inside a row of 16 lanes)
template <int LEVEL>
__device__ __forceinline__ int wave_xor_word(int x) {
    static_assert(LEVEL >= 0 && LEVEL <= 3, "row levels only");
    if constexpr (LEVEL == 0) return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true);   // quad_perm:[1,0,3,2]
    else if constexpr (LEVEL == 1) return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true);  // quad_perm:[2,3,0,1]
    else if constexpr (LEVEL == 3) return __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, true);  // row_ror:8
    else  // xor 4 = xor 3, then xor 7: quad_perm:[3,2,1,0], then row_half_mirror
        return __builtin_amdgcn_update_dpp(0, __builtin_amdgcn_update_dpp(0, x, 0x1B, 0xf, 0xf, true), 0x141, 0xf, 0xf, true);
}
// One level for one pair: `keep` is the lane's own half of the pair, `send` the half its partner keeps.
template <int LEVEL, class T>
__device__ __forceinline__ T wave_pair_step(T a, T b, bool bit) {
    int r0, r1;
    if constexpr (LEVEL <= 3) {
        r0 = wave_word(bit ? b : a);
        r1 = wave_xor_word<LEVEL>(wave_word(bit ? a : b));
    } else {  // rows 1, 3 (halves 1) of the first register change places with rows 0, 2 (half 0) of the second
        static_assert(LEVEL == 4 || LEVEL == 5, "a wave has six levels");
        const auto s = LEVEL == 4 ? __builtin_amdgcn_permlane16_swap((unsigned)wave_word(a), (unsigned)wave_word(b), false, false)
                                  : __builtin_amdgcn_permlane32_swap((unsigned)wave_word(a), (unsigned)wave_word(b), false, false);
        r0 = (int)s[0];
        r1 = (int)s[1];
    }
    T x, y;
    wave_unword(r0, x);
    wave_unword(r1, y);
    return x + y;
}
template <int LEVEL, class T>
__device__ __forceinline__ T wave_butterfly_step(T v) {
    if constexpr (LEVEL <= 3) {
        T y;
        wave_unword(wave_xor_word<LEVEL>(wave_word(v)), y);
        return v + y;
    } else {
        return wave_pair_step<LEVEL>(v, v, false);
    }
}
template <int LEVEL, int M, int NV, class T>
__device__ __forceinline__ void wave_transposed_level(T (&v)[NV], unsigned lane) {
    if constexpr (LEVEL < 6) {
        const bool bit = ((lane >> LEVEL) & 1u) != 0;
#pragma unroll
        for (int j = 0; j < M / 2; ++j) v[j] = wave_pair_step<LEVEL>(v[2 * j], v[2 * j + 1], bit);  // (j <= 2 j: nothing unread is overwritten)
        if constexpr ((M & 1) != 0) v[M / 2] = wave_butterfly_step<LEVEL>(v[M - 1]);
        wave_transposed_level<LEVEL + 1, M / 2 + (M & 1)>(v, lane);
    }
}
// v: the lane's NV values (float, or unsigned for counters: the same network with integer adds); they are overwritten. Returns
// the wave total of value wave_transposed_value(NV, lane), in every lane.
template <int NV, class T>
__device__ __forceinline__ T wave_reduce_transposed(T (&v)[NV], unsigned lane) {
    static_assert(NV >= 1 && NV <= 32, "one value per lane of a half after the xor 16 level");
    wave_transposed_level<0, NV>(v, lane);
    return v[0];
}

struct Mat4Arg {  // a 4x4 passed by value in the kernarg segment (column-major)
    float m[16];
};

}  // namespace sp
