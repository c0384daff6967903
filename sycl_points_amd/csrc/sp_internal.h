/*
 * Internal measurement / tuning switches of libsycl_points_amd.so — NOT part of the C ABI (include/sycl_points_amd.h).
 *
 * They exist for tests/ (bit-identity of every shortcut against the path without it), bench.py (timing one launch of a
 * pair) and scratch/. Every switch lives in the handle it acts on: nothing here is process-global, so a caller that never
 * includes this header can never be affected by one that does. Results are identical under every setting except
 * SP_INTERNAL_FUSED_STAGE_MASK, which drops launches.
 */
#ifndef SP_INTERNAL_H
#define SP_INTERNAL_H

#include "../../include/sycl_points_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    /* sp_gicp_source: launches issued by sp_gicp_iteration_fused / sp_gicp_align_* for this source
     * (bit 0 = per-iteration kernels, bit 1 = final reduce + solve / finish kernel). Default 3. */
    SP_INTERNAL_FUSED_STAGE_MASK = 0,
    /* sp_gicp_source: 2 (default) carry a correspondence to the next iteration when either certificate proves it unchanged,
     * 1 first certificate only, 0 always search. Takes effect at once (the cache is dropped). */
    SP_INTERNAL_FUSED_REUSE = 1,
    /* sp_gicp_source: NN walk inside the fused kernel: -1 (default) 2x2x2 fast path iff the source is cell-sorted,
     * 0 ring walk, 1 fast path. */
    SP_INTERNAL_FUSED_FAST_NN = 2,
    /* sp_grid: self-kNN kernel: 0 (default) chosen by k (lane per point up to k = 7, lane-per-query selection above), 2 wave-cooperative
     * kernel, 3 the selection from k = 7 (wave-cooperative below). Any other value: SP_ERR_INVALID_ARGUMENT. */
    SP_INTERNAL_SELF_KNN_MODE = 3,
    /* sp_gicp_source: sp_gicp_align_fused, when the convergence criteria can be met, runs the TAIL of the alignment as one
     * launch that loops on the device (1, default; taken when every workgroup of the grid is resident) or every iteration
     * as a launch of its own (0). Same bits either way. */
    SP_INTERNAL_FUSED_PERSISTENT = 4,
    /* sp_gicp_source: first iteration of that tail (default 4; 0: the whole alignment as one launch). */
    SP_INTERNAL_FUSED_PERSISTENT_FROM = 5,
    /* sp_bvh: searches for 2 <= k <= 21 with the lane's k best in a heap (1, default) or by the sorted-insertion kernel
     * that serves every other search (0). Same lists either way. */
    SP_INTERNAL_BVH_SELF_HEAP = 6,
    /* sp_bvh: external queries (400 k or more) are searched in the order of the tree's Morton curve (1, default) or as given (0).
     * Same lists either way. */
    SP_INTERNAL_BVH_SORT_QUERIES = 7,
    /* sp_grid: the same for sp_grid_search / sp_grid_radius_search: in cell order (1, default) or as given (0). */
    SP_INTERNAL_GRID_SORT_QUERIES = 8,
    /* sp_gicp_source: sp_gicp_align_optimize on a source of up to 2048 points: one wave per point in the linearisation steps
     * (1, default) or one lane per point (0). Same correspondences either way; the sums are grouped differently. */
    SP_INTERNAL_OPT_WAVE_QUERY = 9,
    /* sp_gicp_source: sp_gicp_align_optimize, wave-per-point launches of up to 2048 points: an LM / dog-leg trial step also
     * linearises at the trial pose (1, default: an accepted trial's next linearisation is then already there) or not (0). The
     * same sequence of optimiser decisions either way. */
    SP_INTERNAL_OPT_FUSE_TRIALS = 10,
    /* sp_bvh: every search also leaves its two walk counters — queries the heap kernel handed on to the sorted-insertion kernel,
     * slots of the deep-stack arena claimed — in two words the handle owns, copied behind the search on its stream (1), or
     * nothing is copied (0, default). Read with sp_internal_bvh_walk_counts. Same launches, same lists either way. */
    SP_INTERNAL_BVH_WALK_COUNTS = 11
};

int sp_internal_source_option(sp_gicp_source* source, int option, int value);
int sp_internal_grid_option(sp_grid* grid, int option, int value);
int sp_internal_bvh_option(sp_bvh* bvh, int option, int value);
/* The walk counters of the handle's last search under SP_INTERNAL_BVH_WALK_COUNTS (waits for that search's stream): zeros for a
 * search that did not go through the heap kernel; SP_ERR_INVALID_ARGUMENT when no search has kept any. An arena claim is counted
 * for every lane that asked for a slot, served or not. */
int sp_internal_bvh_walk_counts(const sp_bvh* bvh, uint32_t* handed_on_out, uint32_t* arena_claims_out);
/* Process-wide: grids of up to 8192 points and fewer than 32768 cells are built by one launch of one workgroup (1, default) or by the
 * general chain of launches (0); < 0 only asks. Returns the previous setting. Same structure bit for bit. */
int sp_internal_grid_small_build(int enable);
/* Device pointer to the per-launch log of an sp_gicp_align_* workspace: entry k = number of source points launch k had to
 * search for (the others reused their previous correspondence by certificate). *n_entries_out = entries kept (64). */
const uint32_t* sp_internal_align_searched_log(void* workspace, size_t* n_entries_out);
/* The prepared source's buffer: whole tiles for the n_max of sp_gicp_source_create, sp_internal_source_tile_floats floats. Tile t
 * holds the prepared points 64 t .. 64 t + 63 in 9 x 64 floats: word 64 k + l of the tile is sub-plane k (x y z | xx xy xz yy yz zz:
 * the point, the plane-regularised covariance's upper triangle) of point 64 t + l. The lanes of the last tile past the prepared n
 * and, for POINT_TO_DISTRIBUTION, the covariance sub-planes are not written. sp_internal_source_tiles_copy copies the whole buffer
 * to (to_source = 0) or from (1) a device buffer of that many floats. */
size_t sp_internal_source_tile_floats(const sp_gicp_source* source);
int sp_internal_source_tiles_copy(sp_gicp_source* source, float* device_buffer, size_t n_floats, int to_source, void* stream);
/* The library's own stable radix sort of (u32 key, u32 value) pairs on the low `bits` key bits (csrc/radix_sort.hip), for its
 * test: all pointers are device pointers, the four arrays are overwritten, *result_in_b_out (host) says which pair holds
 * the sorted data. workspace: sp_internal_radix_sort_workspace_bytes(n). */
size_t sp_internal_radix_sort_workspace_bytes(size_t n);
int sp_internal_radix_sort_u32(uint32_t* keys_a, uint32_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, size_t n,
                               unsigned bits, void* workspace, size_t workspace_bytes, int* result_in_b_out, void* stream);
/* The same sort by the key bits [first_bit, bits) only, and with the first pass's tile histograms already at the start of the
 * workspace (first_hist_ready != 0: hist[digit * tiles + tile], laid out as sp_internal_radix_first_pass says; first_bit 0). */
int sp_internal_radix_sort_u32_ex(uint32_t* keys_a, uint32_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, size_t n,
                                  unsigned bits, unsigned first_bit, int first_hist_ready, void* workspace,
                                  size_t workspace_bytes, int* result_in_b_out, void* stream);
/* radix_first_pass(n, bits) (csrc/radix_sort.h) on the host: out4 = {tiles, tile_keys, digit_bits, mask}. */
void sp_internal_radix_first_pass(size_t n, unsigned bits, unsigned* out4);
/* The sort of (u64 key, u32 value) pairs on the low `bits` <= 64 key bits; workspace as for the u32 sort. */
int sp_internal_radix_sort_u64(uint64_t* keys_a, uint64_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, size_t n,
                               unsigned bits, void* workspace, size_t workspace_bytes, int* result_in_b_out, void* stream);
/* The one-launch exclusive scan (csrc/radix_sort.hip, csrc/sp_lookback.h): device pointers, in == out allowed, the total
 * below 2^30; *total_out_or_null (device) receives the total. */
size_t sp_internal_exclusive_scan_workspace_bytes(size_t n);
int sp_internal_exclusive_scan_u32(const uint32_t* in, uint32_t* out, size_t n, uint32_t* total_out_or_null, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* sp_math.h's atan2f (the one the polar keys are made of) on the host, element by element: out[i] = atan2(y[i], x[i]). */
void sp_internal_atan2f_host(const float* y, const float* x, size_t n, float* out);
/* sp_farthest_point_sampling in a form of the caller's choice (low byte): 0 the library's choice (what the public entry does),
 * 1 one workgroup (n <= 16384, else SP_ERR_INVALID_ARGUMENT), 2 a launch per sample, 3 persistent (n <= 2^21; SP_ERR_RUNTIME
 * when the guard is not to be had). Second byte, for the timing script's sweeps: form 2's grid cap in units of 256 workgroups,
 * form 3's points per lane (1, 2, 4, 8); 0 the library's choice. Same order, flags and distances in every form. */
int sp_internal_fps(int form, const float* points, size_t n, size_t sampling_num, uint32_t first_index, uint32_t* order_out,
                    uint8_t* flags_out_opt, float* min_d2_out_opt, void* workspace, size_t workspace_bytes, void* stream);
/* sp_math.h's symmetric_eigen3 and inverse on the device and nothing else, one lane per row, for their tests. covs / mats / vecs_out /
 * out: n rows of 16 floats, the stored covariance layout (a column-major 4x4 whose 3x3 block counts); vals_out: n rows of 3 floats,
 * ascending; column k of a vecs_out row is the eigenvector of eigenvalue k. All device pointers, rows 16-byte aligned. */
int sp_internal_eigen3(const float* covs, size_t n, float* vals_out, float* vecs_out, void* stream);
int sp_internal_inverse3(const float* mats, size_t n, float* out, void* stream);
/* The pieces the search structures share (csrc/sp_spatial.h) on their own, for their tests; all pointers are device pointers,
 * points are rows of 4 floats.
 * sp_internal_bbox: the sentinel, then (n > 0) the shared bounding-box kernel on `workgroups` (1 .. 256) workgroups: six
 * order-preserving words, min xyz | max xyz over the finite points. */
int sp_internal_bbox(const float* points, size_t n, unsigned workgroups, uint32_t* box6_words_out, void* stream);
/* The Morton key of every point in the box [lo3, hi3] with the BVH's cells per axis (mode 0) or the octree's (mode 1);
 * ~0 for a non-finite point. */
int sp_internal_morton_keys(const float* points, size_t n, const float* lo3, const float* hi3, int mode, uint64_t* keys_out,
                            void* stream);
/* sorted_insert<kcap, order>, one lane per row: the row's m candidates (d, idx: rows x m) in the given sequence into a list of
 * (FLT_MAX, -1); the first k slots go to d_out / idx_out (rows x k). order 0: by distance, first arrival wins ties (kcap 1, 10,
 * 100); 1: (distance, index) lexicographic (kcap 1, 10, 32). */
int sp_internal_sorted_insert(int order, int kcap, int k, const float* d, const int32_t* idx, size_t rows, size_t m, float* d_out,
                              int32_t* idx_out, void* stream);
/* block_reduce_store (csrc/registration_device.h), the workgroup reduction that ends every launch of the registration kernels, on
 * its own: one workgroup of `block` lanes (64, 256 or 1024); lane l brings the nv floats lane_values[l * nv ..] (nv: 28, the sums
 * of a linearisation, or 1) and the two integers lane_counts[2 l], lane_counts[2 l + 1]. row_out: the partial row, 32 words: nv
 * sums, the first integer's sum as a uint32 bit pattern, the second's as a float value, zeros. All device pointers. */
int sp_internal_block_reduce(const float* lane_values, const uint32_t* lane_counts, int block, int nv, float* row_out, void* stream);
/* The wave form of the iteration finish (csrc/sp_wave_solve.h: the 6x6 LDL^T solve and the pose update on the lanes of one wave) on
 * its own: one launch, n independent cases, one wave each. Per case: totals, 30 floats (the 21 sums of H's upper triangle row-major,
 * the 6 of b, 3 that are not read); params, 3 floats (lambda, criteria_rotation, criteria_translation); T, 16 floats, the pose, updated
 * in place. Out per case: delta8_out, 8 floats (delta, converged, ok, as sp_gn_update gives them); x_out, 6 floats, the raw solution of
 * (H + lambda I) x = -b. All device pointers. */
int sp_internal_finish_wave(const float* totals, const float* params, float* T, float* delta8_out, float* x_out, size_t n,
                            void* stream);
/* The form sp_scan_context_db_search computes its products in, for A/B measurements on one box: 0 the matrix cores (the default, what
 * the header specifies), 1 the vector unit (a lane per candidate column, the query's columns as scalar operands, the running sums
 * rotated across the lanes; it sums a shift's columns in cyclic order from column sectors - s, so its low bits may differ).
 * Process-wide. Returns the previous form, or -1 for an unknown one. */
int sp_internal_scan_context_search_form(int form);

#ifdef __cplusplus
}
#endif
#endif /* SP_INTERNAL_H */
