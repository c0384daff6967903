// Device-built octree for exact kNN with lists of up to 100 neighbours (knn::Octree, algorithms/knn/octree.hpp:27-844).
//
// The reference builds its octree on the host by recursion (octree.hpp:233-274, 388-475) and searches it with one work-item
// per query, a 100-entry heap and a 32-entry stack per work-item (octree.hpp:684-844). Here:
//   build   bounding box of the finite points (integer atomics), widened as octree.hpp:267-269 does -> 63-bit Morton key per
//           point, 21 bits per axis, each axis scaled by its own extent (a key prefix of 3 d bits is an octree cell of depth d, and
//           cells halve per axis like the reference's octants) -> the library's radix sort -> every point finds the depth of its
//           leaf by narrowing its key-prefix range level by level (the reference's split rule, octree.hpp:416-418, is monotone
//           in the depth: the count only shrinks, the edge only halves) -> one exclusive scan numbers the nodes in PRE-ORDER
//           (a node is "started" by the first point of its range, so a child's index is always above its parent's) -> every
//           point writes the nodes it starts, the children of an internal node being the non-empty octants of its range ->
//           leaf boxes by integer atomics, the boxes of the internal nodes by one launch per level, deepest first.
//           Nothing recurses, no workgroup waits for another, and every loop is bounded by the depth cap (21), by 32 halvings
//           of a range, or by a count the launch was given.
//   boxes   the box a node is pruned by is the TIGHT min / max of the points below it (as bvh.hip's): it contains each of
//           them in float arithmetic by construction. The cell a key prefix stands for is never used as a box — a cell edge
//           computed from the cell number is rounded and need not contain a point that was binned into it.
//   search  one WAVE per query. The k best are a sorted list held across the lanes in registers (one entry per lane for k <= 64,
//           two for k <= 100), a leaf's points are scored 64 at a time, a node's eight children are tested in eight lanes and
//           pushed nearest-last onto a per-wave stack in LDS of 7 * 21 + 1 entries. Exact, ties to the lowest index (the rule of
//           sp_knn_bruteforce, sp_grid_search and sp_bvh_search; the reference's heap leaves it to the traversal), and nothing
//           is dropped (the reference's stack drops nodes when it is full).
//   remove  lazy, one pass over the stored points (octree.hpp:276-380): a removed point keeps its slot with id -1.
#include <algorithm>

#include "radix_sort.h"
#include "sp_math.h"
#include "sp_spatial.h"
#include "sp_wave_select.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

constexpr int kOctMaxK = 100;
constexpr int kOctMaxDepth = 21;               // levels of a 63-bit key (the reference stops at 32: coincident points only)
constexpr int kOctStack = 7 * kOctMaxDepth + 1;  // an internal node is replaced by <= 8 children, <= 21 internal nodes on a path
constexpr int kOctWaves = kBlock / kWave;      // queries per workgroup
constexpr uint64_t kOctInvalidKey = 1ull << 63;  // behind every key of a finite point

// One node as the search reads it and sp_octree_export hands it out: 16 words.
struct OctNode {
    float lo[3], hi[3];  // tight box of the points below (during the build: order-preserving unsigned encodings)
    uint32_t is_leaf, depth;
    int32_t u[8];        // internal: child per octant (-1: empty); leaf: u[0] = first slot, u[1] = slots, zeros
};
static_assert(sizeof(OctNode) == 64, "sp_octree_export promises 64 bytes per node");

// device words of a build
enum { kMetaStored = 0, kMetaNodes = 1, kMetaLeaves = 2, kMetaDepth = 3, kMetaError = 4, kMetaWords = 8 };

__global__ void oct_init_kernel(unsigned* bbox, unsigned* meta) {
    bbox_sentinel(bbox);
    if (threadIdx.x < kMetaWords) meta[threadIdx.x] = 0u;
}
// root[0..2] / root[3..5]: the box of the root CELL (the points' box widened by max(1e-5, resolution / 2) per side,
// octree.hpp:267-269); root[6]: its longest edge. Only the keys and the split rule use it.
__global__ void oct_root_kernel(const unsigned* __restrict__ bbox, float resolution, float* __restrict__ root) {
    if (threadIdx.x != 0) return;
    const float eps = fmaxf(1e-5f, resolution * 0.5f);
    float edge = 0.0f;
    for (int a = 0; a < 3; ++a) {
        const float lo = ordered_float(bbox[a]) - eps, hi = ordered_float(bbox[3 + a]) + eps;
        root[a] = lo;
        root[3 + a] = hi;
        edge = fmaxf(edge, hi - lo);
    }
    root[6] = edge;
}

__global__ __launch_bounds__(kBlock) void oct_key_kernel(const float4* __restrict__ pts, unsigned n, const float* __restrict__ root,
                                                         uint64_t* __restrict__ keys, unsigned* __restrict__ vals,
                                                         unsigned* __restrict__ meta) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    bool ok = false;
    if (i < n) {
        const float4 p = pts[i];
        uint64_t key = kOctInvalidKey;  // non-finite points: behind all others, in no leaf, never a neighbour
        ok = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
        if (ok) {
            const float box[6] = {root[0], root[1], root[2], root[3], root[4], root[5]};
            key = morton_key_in_box(p.x, p.y, p.z, box, kOctCells);
        }
        keys[i] = key;
        vals[i] = i;
    }
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&meta[kMetaStored], (unsigned)__builtin_popcountll(m));
}

// Per stored point i (keys sorted): the depth L of its leaf, the first point of that leaf, the shallowest depth d0 at which i
// is the first point of its node (22: never), and the number of nodes it starts, L - d0 + 1.
// The range [lo, hi) of the points that share i's key prefix of 3 d bits is narrowed level by level while the node splits:
// more than max_points points, the cell's longest edge above the resolution, depth below 21 (octree.hpp:416-418).
__global__ __launch_bounds__(kBlock) void oct_depth_kernel(const uint64_t* __restrict__ keys, unsigned n,
                                                           const unsigned* __restrict__ meta, const float* __restrict__ root,
                                                           float resolution, unsigned max_points, uint8_t* __restrict__ leaf_depth,
                                                           uint8_t* __restrict__ first_depth, unsigned* __restrict__ leaf_first,
                                                           unsigned* __restrict__ starts) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned m = meta[kMetaStored];
    if (i >= m) { starts[i] = 0u; return; }
    const uint64_t ki = keys[i];
    const float edge0 = root[6];
    unsigned lo = 0u, hi = m;
    int d = 0;
    while (hi - lo > max_points && ldexpf(edge0, -d) > resolution && d < kOctMaxDepth) {
        ++d;
        const int s = 63 - 3 * d;
        const uint64_t p = ki >> s;
        unsigned a = lo, b = i;  // first j in [lo, i] with prefix(j) == p
        while (a < b) {
            const unsigned mid = a + ((b - a) >> 1);
            if ((keys[mid] >> s) < p) a = mid + 1u; else b = mid;
        }
        lo = a;
        a = i + 1u; b = hi;      // first j in (i, hi] with prefix(j) > p
        while (a < b) {
            const unsigned mid = a + ((b - a) >> 1);
            if ((keys[mid] >> s) > p) b = mid; else a = mid + 1u;
        }
        hi = a;
    }
    int d0 = 0;
    if (i > 0u) {
        const uint64_t x = keys[i - 1u] ^ ki;  // (bit 63 is clear in both)
        d0 = x == 0ull ? kOctMaxDepth + 1 : (__clzll((long long)x) - 1) / 3 + 1;
    }
    leaf_depth[i] = (uint8_t)d;
    first_depth[i] = (uint8_t)d0;
    leaf_first[i] = lo;
    starts[i] = d >= d0 ? (unsigned)(d - d0 + 1) : 0u;
}

// Every point writes the nodes it starts: node base[i] + (d - d0) for d0 <= d <= L, the deepest being its leaf. The range of
// a node ends where the key prefix changes; the children of an internal node are the non-empty octants of its range, each
// numbered through ITS first point. Boxes start empty (encoded).
__global__ __launch_bounds__(kBlock) void oct_nodes_kernel(const uint64_t* __restrict__ keys, unsigned* __restrict__ meta,
                                                           const uint8_t* __restrict__ leaf_depth,
                                                           const uint8_t* __restrict__ first_depth, const unsigned* __restrict__ base,
                                                           OctNode* __restrict__ nodes, unsigned node_cap) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned m = meta[kMetaStored];
    if (i >= m) return;
    const int L = leaf_depth[i], d0 = first_depth[i];
    if (L < d0) return;
    const uint64_t ki = keys[i];
    const unsigned b0 = base[i];
    unsigned end = m;
    for (int d = d0; d <= L; ++d) {  // (<= 22 trips)
        const int s = 63 - 3 * d;
        const uint64_t p = ki >> s;
        unsigned a = i + 1u, b = end;
        while (a < b) {
            const unsigned mid = a + ((b - a) >> 1);
            if ((keys[mid] >> s) > p) b = mid; else a = mid + 1u;
        }
        end = a;
        const unsigned id = b0 + (unsigned)(d - d0);
        if (id >= node_cap) {  // cannot happen (the bound of sp_octree_create); never write outside the table
            meta[kMetaError] = 1u;
            return;
        }
        uint4 w[4];
        w[0] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0u);
        w[1] = make_uint4(0u, 0u, d == L ? 1u : 0u, (unsigned)d);
        if (d == L) {
            w[2] = make_uint4(i, end - i, 0u, 0u);
            w[3] = make_uint4(0u, 0u, 0u, 0u);
        } else {
            const int s2 = 60 - 3 * d;  // the octant at depth d + 1
            unsigned child[8];
            unsigned prev = i;
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                unsigned nb = end;  // first point of an octant above o
                if (o < 7) {
                    unsigned a2 = prev, b2 = end;
                    while (a2 < b2) {
                        const unsigned mid = a2 + ((b2 - a2) >> 1);
                        if (((unsigned)(keys[mid] >> s2) & 7u) > (unsigned)o) b2 = mid; else a2 = mid + 1u;
                    }
                    nb = a2;
                }
                child[o] = nb > prev ? base[prev] + (unsigned)(d + 1 - (int)first_depth[prev]) : 0xffffffffu;
                prev = nb;
            }
            w[2] = make_uint4(child[0], child[1], child[2], child[3]);
            w[3] = make_uint4(child[4], child[5], child[6], child[7]);
        }
        uint4* const dst = reinterpret_cast<uint4*>(nodes + id);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[q] = w[q];
    }
}

// Leaf boxes: every stored point into the box of its leaf. The points of a wave are neighbours in key order, so mostly one
// leaf: then the wave reduces first and one lane adds.
__global__ __launch_bounds__(kBlock) void oct_leaf_box_kernel(const float4* __restrict__ spts, const unsigned* __restrict__ meta,
                                                              const uint8_t* __restrict__ leaf_depth,
                                                              const uint8_t* __restrict__ first_depth,
                                                              const unsigned* __restrict__ leaf_first, const unsigned* __restrict__ base,
                                                              OctNode* __restrict__ nodes, unsigned node_cap) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const bool act = i < meta[kMetaStored];
    unsigned id = 0xffffffffu;
    unsigned e[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    if (act) {
        const unsigned f = leaf_first[i];
        id = base[f] + (unsigned)((int)leaf_depth[i] - (int)first_depth[f]);
        const float4 p = spts[i];
        e[0] = e[3] = ordered_bits(p.x);
        e[1] = e[4] = ordered_bits(p.y);
        e[2] = e[5] = ordered_bits(p.z);
    }
    const bool ok = act && id < node_cap;
    const unsigned id0 = (unsigned)__builtin_amdgcn_readfirstlane((int)id);
    if (__all(ok && id == id0)) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                e[a] = min(e[a], (unsigned)__shfl_xor((int)e[a], o, 64));
                e[3 + a] = max(e[3 + a], (unsigned)__shfl_xor((int)e[3 + a], o, 64));
            }
        if ((threadIdx.x & 63) != 0) return;
    } else if (!ok) {
        return;
    }
    unsigned* const box = reinterpret_cast<unsigned*>(nodes + id);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(box + a, e[a]);
        atomicMax(box + 3 + a, e[3 + a]);
    }
}
// The boxes of the internal nodes of depth `depth` from their children's (one level deeper: written by the launch before).
__global__ __launch_bounds__(kBlock) void oct_level_box_kernel(OctNode* __restrict__ nodes, const unsigned* __restrict__ meta,
                                                               unsigned node_cap, unsigned depth) {
    const unsigned j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= min(meta[kMetaNodes], node_cap)) return;
    const uint4* const rec = reinterpret_cast<const uint4*>(nodes + j);
    const uint4 head = rec[1];  // (hi.y, hi.z, is_leaf, depth)
    if (head.z != 0u || head.w != depth) return;
    const uint4 c0 = rec[2], c1 = rec[3];
    const unsigned child[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    unsigned e[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
#pragma unroll
    for (int o = 0; o < 8; ++o)
        if (child[o] < node_cap) {
            const unsigned* const cb = reinterpret_cast<const unsigned*>(nodes + child[o]);
#pragma unroll
            for (int a = 0; a < 3; ++a) { e[a] = min(e[a], cb[a]); e[3 + a] = max(e[3 + a], cb[3 + a]); }
        }
    unsigned* const box = reinterpret_cast<unsigned*>(nodes + j);
#pragma unroll
    for (int a = 0; a < 6; ++a) box[a] = e[a];
}
// Encoded boxes -> floats; the counts sp_octree_info reports.
__global__ __launch_bounds__(kBlock) void oct_finish_kernel(OctNode* __restrict__ nodes, unsigned* __restrict__ meta, unsigned node_cap) {
    const unsigned j = blockIdx.x * kBlock + threadIdx.x;
    const bool act = j < min(meta[kMetaNodes], node_cap);
    unsigned leaf = 0u, depth = 0u;
    if (act) {
        unsigned* const box = reinterpret_cast<unsigned*>(nodes + j);
#pragma unroll
        for (int a = 0; a < 6; ++a) box[a] = __float_as_uint(ordered_float(box[a]));
        leaf = nodes[j].is_leaf;
        depth = nodes[j].depth;
    }
    const unsigned long long lm = __ballot(leaf != 0u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) depth = max(depth, (unsigned)__shfl_xor((int)depth, o, 64));
    if ((threadIdx.x & 63) == 0) {
        if (lm) atomicAdd(&meta[kMetaLeaves], (unsigned)__builtin_popcountll(lm));
        if (depth) atomicMax(&meta[kMetaDepth], depth);
    }
}

__device__ __forceinline__ float box_d2(float lx, float ly, float lz, float hx, float hy, float hz, float qx, float qy, float qz) {
    const float dx = fmaxf(fmaxf(lx - qx, qx - hx), 0.0f), dy = fmaxf(fmaxf(ly - qy, qy - hy), 0.0f),
                dz = fmaxf(fmaxf(lz - qz, qz - hz), 0.0f);
    // never above dist2 to any point inside the (tight) box: per axis the box's gap is at most the point's, and the factor
    // covers the different rounding of the two sums (bvh.hip's bound) — a box is skipped only when strictly beyond the k-th
    return fmaf(dx, dx, fmaf(dy, dy, dz * dz)) * 0.999999f;
}

// One wave per query. TWO: the list has two entries per lane (positions lane and 64 + lane), for 64 < k <= 100.
template <bool TWO>
__global__ __launch_bounds__(kBlock) void octree_search_kernel(const OctNode* __restrict__ nodes, const float4* __restrict__ spts,
                                                               unsigned stored, const float4* __restrict__ queries, unsigned nq, int k,
                                                               QueryPose pose, int32_t* __restrict__ idx_out,
                                                               float* __restrict__ d2_out) {
    __shared__ int st_node[kOctWaves][kOctStack];
    __shared__ float st_d[kOctWaves][kOctStack];
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned w = threadIdx.x >> 6;
    const Rigid T = load_pose(pose);
    const int kth_lane = (k - 1) & 63;  // the k-th entry: lo for k <= 64, hi above
    // (no barrier below: the waves of a workgroup share nothing)
    for (size_t qi = (size_t)blockIdx.x * kOctWaves + w; qi < nq; qi += (size_t)gridDim.x * kOctWaves) {
        float qx, qy, qz;
        load_query(queries, (unsigned)qi, T, qx, qy, qz);
        unsigned long long lo = kNoCand, hi = kNoCand, kth = kNoCand;  // sorted ascending over lo[0..63], hi[0..63]

        // the slots [start, start + count) against the list: every candidate nearer than the k-th goes in at its rank, the
        // entries behind it move up by one position (lane 63 of lo hands on to lane 0 of hi)
        auto scan = [&](unsigned start, unsigned count) {
#pragma unroll 1
            for (unsigned b = 0; b < count; b += 64u) {
                const bool in = b + (unsigned)lane < count;
                const float4 p = spts[start + (in ? b + (unsigned)lane : 0u)];
                const int id = __float_as_int(p.w);
                // (a removed point has id -1; a NaN or infinite distance has a bit pattern above FLT_MAX's: never below the k-th)
                const unsigned long long key = (in && id >= 0) ? cand_key(dist2(qx, qy, qz, p.x, p.y, p.z), id) : ~0ull;
                unsigned long long todo = __ballot(key < kth);
                while (todo) {
                    const int src = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const unsigned long long v = bcast_k(key, src);
                    if (!(v < kth)) continue;  // the k-th entry moved since the ballot
                    int rank = __builtin_popcountll(__ballot(lo < v));
                    if (TWO) rank += __builtin_popcountll(__ballot(hi < v));
                    const unsigned long long ul = shift_up1_k(lo);
                    if (TWO) {
                        unsigned long long uh = shift_up1_k(hi);
                        const unsigned long long carry = bcast_k(lo, 63);
                        if (lane == 0) uh = carry;
                        const int r2 = rank - 64;
                        hi = lane < r2 ? hi : (lane == r2 ? v : uh);
                    }
                    lo = lane < rank ? lo : (lane == rank ? v : ul);
                    kth = bcast_k(TWO ? hi : lo, kth_lane);
                }
            }
        };

        int top = 0;
        bool overflow = false;
        if (isfinite(qx) && isfinite(qy) && isfinite(qz) && stored != 0u) {
            if (lane == 0) { st_node[w][0] = 0; st_d[w][0] = 0.0f; }
            top = 1;
        }
        // every node is pushed at most once (by its parent) and popped at most once: the walk ends
        while (top > 0) {
            --top;
            __builtin_amdgcn_wave_barrier();
            const int nd = __builtin_amdgcn_readfirstlane(st_node[w][top]);
            const float dd = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(st_d[w][top])));
            if (dd > key_d2(kth)) continue;  // the list has filled up since the push
            const OctNode* const N = nodes + nd;
            if (N->is_leaf) {
                scan((unsigned)N->u[0], (unsigned)N->u[1]);
                continue;
            }
            const int c = lane < 8 ? N->u[lane & 7] : -1;
            float dc = FLT_MAX;
            if (c >= 0) {
                const OctNode* const C = nodes + c;
                dc = box_d2(C->lo[0], C->lo[1], C->lo[2], C->hi[0], C->hi[1], C->hi[2], qx, qy, qz);
            }
            // (a box exactly AT the k-th distance may hold a point at that distance with a lower index: it is entered)
            const bool reach = c >= 0 && !(dc > key_d2(kth));
            const unsigned rm = (unsigned)__ballot(reach);
            const int cnt = __builtin_popcount(rm);
            if (top + cnt > kOctStack) {  // cannot happen (kOctStack); never write outside the stack
                overflow = true;
                break;
            }
            int pos = 0;  // farthest first, nearest last: the number of reachable siblings that are farther
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float dj = bcast_f(dc, j);
                pos += (((rm >> j) & 1u) && (dj > dc || (dj == dc && j > lane))) ? 1 : 0;
            }
            if (reach) { st_node[w][top + pos] = c; st_d[w][top + pos] = dc; }
            top += cnt;
        }
        if (overflow) {  // start over and look at every stored point
            lo = hi = kth = kNoCand;
            scan(0u, stored);
        }
        const size_t o = qi * (size_t)k;
        if (lane < k) {
            idx_out[o + lane] = lo == kNoCand ? -1 : key_idx(lo);
            d2_out[o + lane] = lo == kNoCand ? FLT_MAX : key_d2(lo);
        }
        if (TWO && 64 + lane < k) {
            idx_out[o + 64 + lane] = hi == kNoCand ? -1 : key_idx(hi);
            d2_out[o + 64 + lane] = hi == kNoCand ? FLT_MAX : key_d2(hi);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// stats[0] = points kept, stats[1] = largest new id + 1 (also of a new id that was refused: the host sees it is out of range).
__global__ __launch_bounds__(kBlock) void oct_remove_kernel(float4* __restrict__ spts, unsigned stored, const uint8_t* __restrict__ flags,
                                                            const int32_t* __restrict__ new_indices, unsigned n_flags,
                                                            unsigned* __restrict__ stats) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    bool kept = false;
    unsigned next = 0u;
    if (i < stored) {
        const int id = __float_as_int(spts[i].w);
        if (id >= 0 && (unsigned)id < n_flags) {  // (a live id is always below the id range the host checked n_flags against)
            const int nid = new_indices[id];
            if (flags[id] == 1 && nid >= 0) {
                next = (unsigned)nid + 1u;
                kept = (unsigned)nid < n_flags;
                if (kept) spts[i].w = __int_as_float(nid);
            } else {
                spts[i].w = __int_as_float(-1);
            }
        }
    }
    const unsigned long long km = __ballot(kept);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) next = max(next, (unsigned)__shfl_xor((int)next, o, 64));
    if ((threadIdx.x & 63) == 0) {
        if (km) atomicAdd(&stats[0], (unsigned)__builtin_popcountll(km));
        if (next) atomicMax(&stats[1], next);
    }
}

__global__ __launch_bounds__(kBlock) void oct_export_kernel(const OctNode* __restrict__ nodes, unsigned n_nodes,
                                                            const float4* __restrict__ spts, unsigned stored,
                                                            uint4* __restrict__ nodes_out, int32_t* __restrict__ ids_out) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (nodes_out && i < 4u * n_nodes) nodes_out[i] = reinterpret_cast<const uint4*>(nodes)[i];
    if (ids_out && i < stored) ids_out[i] = __float_as_int(spts[i].w);
}

// At most 21 levels hold internal nodes, the nodes of a level are disjoint and an internal node holds more than
// max_points points; the leaves are disjoint and non-empty, and each is the root or the child of an internal node.
size_t octree_node_bound(size_t n, size_t max_points) {
    const size_t internal = (size_t)kOctMaxDepth * (n / (max_points + 1));
    const size_t leaves = std::min(n, 8 * internal + 1);
    return std::max<size_t>(internal + leaves, 1);
}

}  // namespace
}  // namespace sp

struct sp_octree {
    float resolution = 0.0f;
    size_t max_points = 0;
    size_t stored = 0;      // slots of `pts`: the finite points of the build, in leaf order
    size_t kept = 0;        // of them still alive
    uint64_t next_id = 0;   // the ids in use are below it (octree.hpp's next_point_id_)
    size_t n_nodes = 0, n_leaves = 0, depth = 0;
    float4* pts = nullptr;  // w = the point's id, -1 once removed
    sp::OctNode* nodes = nullptr;
    mutable sp::StreamSet streams;
};

extern "C" void sp_octree_destroy(sp_octree* t) {
    if (!t) return;
    sp::pooled_free_after(t->pts, t->streams);
    sp::pooled_free_after(t->nodes, t->streams);
    delete t;
}

extern "C" int sp_octree_create(const float* points, size_t n, float resolution, size_t max_points_per_node, void* stream,
                                sp_octree** out) {
    using namespace sp;
    if (!out || (n && !points)) {
        sp_set_error("[Octree::build] null `points` or `out`");
        return SP_ERR_INVALID_ARGUMENT;
    }
    *out = nullptr;
    const size_t max_points = std::min<size_t>(max_points_per_node, 0x7fffffffu);
    const size_t cap = octree_node_bound(n, max_points);
    if (n >= (1ull << 30) || cap >= (1ull << 30)) {
        sp_set_error("[Octree::build] too many points for 2^30 nodes");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    sp_octree* t = new sp_octree();
    t->resolution = resolution;
    t->max_points = max_points_per_node;
    t->next_id = n;
    t->streams.note(st);
    if (n == 0) {
        *out = t;
        return SP_OK;
    }
    auto fail = [&](const char* msg) {
        sp_set_error(msg);
        (void)hipStreamSynchronize(st);
        sp_octree_destroy(t);
        return SP_ERR_HIP;
    };
    ScratchBuf b_small, b_kin, b_kout, b_vin, b_vout, b_tmp, b_ld, b_fd, b_lf, b_base, b_scan;
    const size_t tmp_bytes = radix_sort_u64_workspace_bytes(n);
    const size_t scan_bytes = exclusive_scan_u32_workspace_bytes(n);
    hipError_t e = pooled_alloc(&t->pts, n * sizeof(float4), st);
    if (e == hipSuccess) e = pooled_alloc(&t->nodes, cap * sizeof(OctNode), st);
    if (e == hipSuccess) e = b_small.get(64 * sizeof(unsigned), st);  // bbox [0, 6), root [8, 15), meta [16, 24)
    if (e == hipSuccess) e = b_kin.get(n * 8, st);
    if (e == hipSuccess) e = b_kout.get(n * 8, st);
    if (e == hipSuccess) e = b_vin.get(n * 4, st);
    if (e == hipSuccess) e = b_vout.get(n * 4, st);
    if (e == hipSuccess) e = b_tmp.get(tmp_bytes ? tmp_bytes : 16, st);
    if (e == hipSuccess) e = b_ld.get(n, st);
    if (e == hipSuccess) e = b_fd.get(n, st);
    if (e == hipSuccess) e = b_lf.get(n * 4, st);
    if (e == hipSuccess) e = b_base.get(n * 4, st);
    if (e == hipSuccess) e = b_scan.get(scan_bytes ? scan_bytes : 16, st);
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    const float4* pts = reinterpret_cast<const float4*>(points);
    unsigned* const bbox = b_small.as<unsigned>();
    float* const root = reinterpret_cast<float*>(bbox + 8);
    unsigned* const meta = bbox + 16;
    uint64_t *kin = b_kin.as<uint64_t>(), *kout = b_kout.as<uint64_t>();
    unsigned *vin = b_vin.as<unsigned>(), *vout = b_vout.as<unsigned>();
    const unsigned n32 = (unsigned)n, cap32 = (unsigned)cap, g = div_up(n, kBlock), gn = div_up(cap, kBlock);
    // 1. the root cell and the keys
    oct_init_kernel<<<1, 64, 0, st>>>(bbox, meta);
    bbox_kernel<><<<std::min(stream_grid(n, kBlock, 4), 256u), kBlock, 0, st>>>(pts, n32, bbox);
    oct_root_kernel<<<1, 64, 0, st>>>(bbox, resolution, root);
    oct_key_kernel<<<g, kBlock, 0, st>>>(pts, n32, root, kin, vin, meta);
    // 2. key order
    bool in_b = false;
    if (radix_sort_pairs_u64(kin, kout, vin, vout, n, 64, b_tmp.p, tmp_bytes, &in_b, st) != SP_OK) return fail("[Octree::build] sort failed");
    if (!in_b) { kout = kin; vout = vin; }
    gather_by_order_kernel<><<<g, kBlock, 0, st>>>(pts, vout, n32, t->pts, meta + kMetaStored);
    // 3. leaf depths, node numbers (pre-order), nodes
    oct_depth_kernel<<<g, kBlock, 0, st>>>(kout, n32, meta, root, resolution, (unsigned)max_points, b_ld.as<uint8_t>(),
                                          b_fd.as<uint8_t>(), b_lf.as<unsigned>(), b_base.as<unsigned>());
    if (exclusive_scan_u32(b_base.as<unsigned>(), b_base.as<unsigned>(), n, meta + kMetaNodes, b_scan.p, scan_bytes, st) != SP_OK)
        return fail("[Octree::build] scan failed");
    oct_nodes_kernel<<<g, kBlock, 0, st>>>(kout, meta, b_ld.as<uint8_t>(), b_fd.as<uint8_t>(), b_base.as<unsigned>(), t->nodes, cap32);
    // 4. boxes: leaves from their points, then one level of internal nodes per launch, deepest first
    oct_leaf_box_kernel<<<g, kBlock, 0, st>>>(t->pts, meta, b_ld.as<uint8_t>(), b_fd.as<uint8_t>(), b_lf.as<unsigned>(),
                                             b_base.as<unsigned>(), t->nodes, cap32);
    for (int d = kOctMaxDepth - 1; d >= 0; --d) oct_level_box_kernel<<<gn, kBlock, 0, st>>>(t->nodes, meta, cap32, (unsigned)d);
    oct_finish_kernel<<<gn, kBlock, 0, st>>>(t->nodes, meta, cap32);
    unsigned h_own[kMetaWords];
    unsigned* const h = pinned_mailbox() ? static_cast<unsigned*>(pinned_mailbox()) : h_own;
    if (launch_status() != SP_OK || hipMemcpyAsync(h, meta, kMetaWords * sizeof(unsigned), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail("[Octree::build] build failed");  // scratch idle from here
    if (h[kMetaError] || h[kMetaNodes] > cap32) {
        sp_set_error("[Octree::build] node bound exceeded");
        sp_octree_destroy(t);
        return SP_ERR_RUNTIME;
    }
    t->stored = t->kept = h[kMetaStored];
    t->n_nodes = h[kMetaNodes];
    t->n_leaves = h[kMetaLeaves];
    t->depth = h[kMetaDepth];
    *out = t;
    return SP_OK;
}

extern "C" size_t sp_octree_size(const sp_octree* t) { return t ? t->kept : 0; }

extern "C" int sp_octree_info(const sp_octree* t, int what, uint64_t* out) {
    if (!t || !out) {
        sp_set_error("[Octree] null `octree` or `out`");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const bool empty = t->kept == 0;
    switch (what) {
        case SP_OCTREE_NODES: *out = empty ? 0 : t->n_nodes; break;
        case SP_OCTREE_LEAVES: *out = empty ? 0 : t->n_leaves; break;
        case SP_OCTREE_DEPTH: *out = empty ? 0 : t->depth; break;
        case SP_OCTREE_NEXT_ID: *out = t->next_id; break;
        case SP_OCTREE_SLOTS: *out = empty ? 0 : t->stored; break;
        default:
            sp_set_error("[Octree] unknown `what`");
            return SP_ERR_INVALID_ARGUMENT;
    }
    return SP_OK;
}

extern "C" int sp_octree_search(const sp_octree* t, const float* queries, size_t nq, size_t k, const float* transT,
                                int transT_on_device, int32_t* idx_out, float* d2_out, void* stream) {
    using namespace sp;
    if (k > (size_t)kOctMaxK) {  // octree.hpp:629
        sp_set_error("[Octree::knn_search_async] Requested neighbor count `k` exceeds the supported maximum (100)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (!t) {
        sp_set_error("[Octree::knn_search_async] null `octree`");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (nq && k && (!idx_out || !d2_out)) {
        sp_set_error("[Octree::knn_search_async] null `idx_out` or `d2_out`");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (nq && !queries) {
        sp_set_error("[Octree::knn_search_async] null `queries`");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (nq == 0 || k == 0) return SP_OK;
    if (nq >= (1ull << 32)) {
        sp_set_error("[Octree::knn_search_async] more than 2^32 queries");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    t->streams.note(st);
    if (t->kept == 0) {
        fill_empty_kernel<><<<div_up(nq * k, kBlock), kBlock, 0, st>>>(idx_out, d2_out, nq * k);
        return launch_status();
    }
    const QueryPose pose = query_pose(transT, transT_on_device);
    const float4* q = reinterpret_cast<const float4*>(queries);
    const unsigned grid = (unsigned)std::min<size_t>(div_up(nq, kOctWaves), (size_t)kNumCU * 64);
    if (k <= 64)
        octree_search_kernel<false><<<grid, kBlock, 0, st>>>(t->nodes, t->pts, (unsigned)t->stored, q, (unsigned)nq, (int)k, pose, idx_out,
                                                            d2_out);
    else
        octree_search_kernel<true><<<grid, kBlock, 0, st>>>(t->nodes, t->pts, (unsigned)t->stored, q, (unsigned)nq, (int)k, pose, idx_out,
                                                           d2_out);
    return launch_status();
}

extern "C" int sp_octree_remove_by_flags(sp_octree* t, const uint8_t* flags, const int32_t* new_indices, size_t n_flags,
                                         void* stream) {
    using namespace sp;
    if (!t || (n_flags && (!flags || !new_indices))) {
        sp_set_error("[Octree::remove_nodes_by_flags] null `octree`, `flags` or `new_indices`");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (n_flags != t->next_id) {  // octree.hpp:285-289
        sp_set_error("[Octree::remove_nodes_by_flags] flags and indices must match the octree point identifier range");
        return SP_ERR_RUNTIME;
    }
    auto reset = [&]() { t->kept = 0; t->next_id = 0; };  // octree.hpp:212-228: the empty tree
    if (n_flags == 0 || t->kept == 0) {  // octree.hpp:291-294
        reset();
        return SP_OK;
    }
    hipStream_t st = as_stream(stream);
    t->streams.note(st);
    ScratchBuf b_stats;
    if (b_stats.get(2 * sizeof(unsigned), st) != hipSuccess) {
        sp_set_error("[Octree::remove_nodes_by_flags] out of device memory");
        return SP_ERR_HIP;
    }
    unsigned h_own[2];
    unsigned* const h = pinned_mailbox() ? static_cast<unsigned*>(pinned_mailbox()) : h_own;
    int rc = zero_async(b_stats.p, 2 * sizeof(unsigned), st);
    if (rc == SP_OK) {
        oct_remove_kernel<<<div_up(t->stored, kBlock), kBlock, 0, st>>>(t->pts, (unsigned)t->stored, flags, new_indices,
                                                                       (unsigned)n_flags, b_stats.as<unsigned>());
        rc = launch_status();
    }
    if (rc == SP_OK && hipMemcpyAsync(h, b_stats.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st) != hipSuccess) rc = SP_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) rc = SP_ERR_HIP;  // the scratch is idle again
    if (rc != SP_OK) return rc;
    const size_t kept = h[0], next = h[1];  // next = largest new id + 1
    if (next > n_flags) {  // octree.hpp:329-332 (as there, the points relabelled before the throw stay relabelled)
        sp_set_error("[Octree::remove_nodes_by_flags] remapped point identifier in indices exceeds the allocated range");
        t->kept = kept;
        return SP_ERR_RUNTIME;
    }
    if (kept == 0) {  // octree.hpp:363-366
        reset();
        return SP_OK;
    }
    t->kept = kept;
    t->next_id = std::max<uint64_t>(next, kept);  // octree.hpp:368-379
    return SP_OK;
}

extern "C" int sp_octree_export(const sp_octree* t, void* nodes_out, int32_t* point_ids_out, void* stream) {
    using namespace sp;
    if (!t) {
        sp_set_error("[Octree] null `octree`");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (t->kept == 0 || (!nodes_out && !point_ids_out)) return SP_OK;
    hipStream_t st = as_stream(stream);
    t->streams.note(st);
    const size_t work = std::max(4 * t->n_nodes, t->stored);
    oct_export_kernel<<<div_up(work, kBlock), kBlock, 0, st>>>(t->nodes, (unsigned)t->n_nodes, t->pts, (unsigned)t->stored,
                                                             static_cast<uint4*>(nodes_out), point_ids_out);
    return launch_status();
}
