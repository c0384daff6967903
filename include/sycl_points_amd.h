/*
 * sycl_points_amd — C ABI of the MI355X (gfx950) hot path.
 *
 * The reference (fateshelled/sycl_points) is a header-only C++/SYCL library with no C ABI: its device code is
 * reached through C++ templates. This header is the boundary a maintainer would bind instead of
 * those SYCL kernels; every entry point cites the reference interface it replaces
 * (paths relative to /root/reference/cpp/include/sycl_points/).
 *
 * Conventions
 *  - all array pointers are DEVICE pointers (HBM) unless the parameter name ends in `_host`;
 *  - points / normals are float[4] (x,y,z,w), covariances are float[16] column-major 4x4 with the 3x3 block used
 *    (Eigen::Vector4f / Eigen::Matrix4f storage, points/types.hpp:11-18); entries outside the 3x3 block are
 *    written as 0 and ignored on input; transforms are float[16] column-major (Eigen::Matrix4f::data());
 *  - every call only ENQUEUES work on `stream` (a hipStream_t, may be NULL for the default stream) and returns
 *    immediately; no call allocates or synchronises unless its comment says so, so a sequence of calls can be
 *    captured into a hipGraph;
 *  - return value: SP_OK, or an error code whose meaning mirrors the C++ exception the reference would throw;
 *    sp_last_error() returns the message (thread local).
 */
#ifndef SYCL_POINTS_AMD_H
#define SYCL_POINTS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_OK 0
#define SP_ERR_INVALID_ARGUMENT 1 /* reference: std::invalid_argument */
#define SP_ERR_RUNTIME 2          /* reference: std::runtime_error    */
#define SP_ERR_HIP 3              /* reference: sycl::exception from wait_and_throw */

/* 7: sp_knn_tree_* — the accelerated KDTree's structures and its choice among them moved into the library from both front ends */
#define SP_ABI_VERSION 7
int sp_abi_version(void);
/* The library keeps device buffers it no longer needs (temporaries of a build, the arrays of a destroyed grid / tree / target) in
 * a pool, tagged with the stream whose work may still use them: a later call on the SAME stream takes them without waiting (stream
 * order), nobody else does. A caller that is about to destroy a stream it has passed to the library calls this first (the
 * facade's DeviceQueue does): it waits for the stream and clears its tags. Without it such buffers stay out of use until the
 * pool's sweep (a device-wide wait once 32 of them have piled up). */
void sp_stream_retired(void* stream);
const char* sp_last_error(void);

/* Number of devices visible / select the device for the calling thread (utils/sycl_utils.hpp:398-465). */
int sp_device_count(void);
int sp_set_device(int device);

/* ------------------------------------------------------------------------------------------------ KNN */

/* Brute-force kNN (algorithms/knn/bruteforce.hpp:24-96, kernel K1).
 * Exact; k <= 20 (SP_ERR_INVALID_ARGUMENT otherwise — the reference has no check and overruns its arrays);
 * strict '<' so the lowest target index wins ties; rows ascending by squared distance, padded with -1 / FLT_MAX.
 * workspace: sp_knn_bruteforce_workspace_bytes(nq, nt, k) bytes. */
size_t sp_knn_bruteforce_workspace_bytes(size_t nq, size_t nt, size_t k);
int sp_knn_bruteforce(const float* queries, size_t nq, const float* targets, size_t nt, size_t k, int32_t* idx_out,
                      float* d2_out, void* workspace, size_t workspace_bytes, void* stream);
/* From 16 K targets on, the search bounds every query's k-th distance first (chunk minima of an approximate distance with a
 * proven error term) and evaluates the reference's expression only where a neighbour can be. That first pass runs on the
 * matrix cores (bf16-split operands, v_mfma_f32_32x32x16_bf16); valu != 0 selects its packed-fp32 VALU form instead, for
 * measurement (process-wide; the results do not depend on it).
 * Target clouds of 256 .. 12032 points (a voxel-downsampled scan) are answered by ONE launch that keeps the whole cloud in LDS
 * (a wave per four queries: lane minima -> bound of the k-th distance -> the targets within it -> 64-lane sort); valu == 2
 * switches that path off (the general ones then serve every size), valu == 3 on again (default). Same lists. */
int sp_knn_bruteforce_set_pass_a(int valu);

/* KD-tree (algorithms/knn/kdtree.hpp:142-766).
 * sp_kdtree_create: KDTree::build (kdtree.hpp:165-178, 292-413) — host median-split build from HOST points
 *   (same split rule, same std::nth_element, so the same topology as the reference), then upload. Allocates and
 *   synchronises. leaf_threshold default in the reference is 16.
 * sp_kdtree_search: KDTree::knn_search_async (kdtree.hpp:203-224, 424-562, kernel K2): neighbours of transT*q,
 *   traversal order, tie rule (first visited wins) and the 16-entry far stack of the reference;
 *   k <= 100 else SP_ERR_RUNTIME ("`k` is too large", kdtree.hpp:221-223). A query with a non-finite coordinate gets a row
 *   of (-1, FLT_MAX), where the reference's tree writes NaN distances for k > 1.
 * sp_kdtree_radius_search: KDTree::radius_search_async (kdtree.hpp:251-280, 574-719, kernel K3).
 * sp_kdtree_remove_by_flags: KDTree::remove_nodes_by_flags (kdtree.hpp:282-284, 721-765, kernel K4);
 *   flags 1 = keep, 0 = remove; new_indices[p] must be >= 0 for kept points (filter_by_flags.hpp:97-99). */
typedef struct sp_kdtree sp_kdtree;
int sp_kdtree_create(const float* points_host, size_t n, size_t leaf_threshold, void* stream, sp_kdtree** out);
void sp_kdtree_destroy(sp_kdtree* tree);
size_t sp_kdtree_size(const sp_kdtree* tree); /* number of points */
int sp_kdtree_search(const sp_kdtree* tree, const float* queries, size_t nq, size_t k, const float* transT,
                     int transT_on_device, int32_t* idx_out, float* d2_out, void* stream);
int sp_kdtree_radius_search(const sp_kdtree* tree, const float* queries, size_t nq, size_t max_k, float radius,
                            const float* transT, int transT_on_device, int32_t* idx_out, float* d2_out, void* stream);
int sp_kdtree_remove_by_flags(sp_kdtree* tree, const uint8_t* flags, const int32_t* new_indices, size_t n_flags,
                              void* stream);

/* GridKNN — an MI355X-native KNNBase implementation (no counterpart file in the reference; it plugs into the
 * KNNBase::knn_search_async seam, algorithms/knn/knn.hpp:14-61, exactly as KDTree / Octree do).
 * Exact kNN on a uniform cell grid built ON THE DEVICE from device points (bounding box, cell ids, radix sort,
 * cell_start table): a handful of independent loads per query instead of the KD-tree's chain of dependent node loads.
 * Results are bit-identical to sp_knn_bruteforce (same distance arithmetic, ties to the lowest index), k <= 20.
 * sp_grid_create allocates and synchronises. cell_size <= 0: chosen so that a cell holds `points_per_cell` points on
 * average (<= 0: 2). */
typedef struct sp_grid sp_grid;
int sp_grid_create(const float* points, size_t n, float cell_size, float points_per_cell, void* stream, sp_grid** out);
/* The same with the cell size steered by what the build measures instead of by the bounding-box volume alone: while the OCCUPIED
 * cells hold well more points than those of a uniform cloud at `points_per_cell` would (a cloud of surfaces — a voxel-downsampled
 * LiDAR scan fills 2 % of its box), the cell shrinks by the dimension the measurements imply and the grid is built again (at
 * most three more sorts; none for a uniform cloud; the table stays below 32 M cells). What Registration::align's in-loop search
 * uses when it stands in for the caller's KDTree (knn/kdtree.hpp:463-553 is density-agnostic; a fixed-volume grid is not). */
int sp_grid_create_adaptive(const float* points, size_t n, float points_per_cell, void* stream, sp_grid** out);
/* sp_grid_create for a caller that already knows a box holding every finite point (min x, y, z, max x, y, z): the bounding-box
 * kernel, its read-back and the wait for it are skipped — the build then never waits for its stream. What voxel downsampling
 * leaves is such a cloud: its voxels' key box is known on the host (the facade's VoxelGrid hands it on with the cloud). The box
 * is vouched for: a finite point outside the grid it implies raises the library's device error word (reported by a later call)
 * and that grid's searches are not exact. */
int sp_grid_create_bounded(const float* points, size_t n, const float* bounds_min_max6, float cell_size, float points_per_cell,
                           void* stream, sp_grid** out);
void sp_grid_destroy(sp_grid* grid);
size_t sp_grid_size(const sp_grid* grid);
float sp_grid_cell_size(const sp_grid* grid);
/* Points in the fullest cell (measured on the first call: one small kernel and a blocking read-back; cached). The grid's searches assume near-uniform density (a query scans its 27
 * cells): a value far above the points-per-cell target says that a hierarchy (sp_bvh_*) serves this cloud better. */
uint32_t sp_grid_max_cell_points(const sp_grid* grid);
/* idx_out[i] = original index of the i-th point in the grid's cell order (z-major, then y, then x; stable inside a cell).
 * A cloud stored in this order (it is also the order VoxelGrid::downsampling produces, voxel_downsampling.hpp:146-288:
 * sorted by voxel key) keeps neighbouring lanes on neighbouring cells of ANY grid it is later searched against, so
 * sp_gicp_source_prepare can skip its per-alignment sort (SP_SOURCE_PRESORTED). */
int sp_grid_order(const sp_grid* grid, uint32_t* idx_out, void* stream);
/* KNNBase::knn_search_async on the grid (k <= 20). For k > 10 the call takes nq + 1 words of scratch from the library's
 * buffer pool for its duration (the list of queries a first, 27-cell pass could not prove): inside a stream capture that
 * works once the pool holds such a buffer, i.e. after one eager call of the same size. Queries in the cell order of any grid
 * (sp_grid_order) are served three times faster than in random order (their candidates share cache lines); 400 k queries or
 * more are therefore sorted by cell first (a key per query and the library's radix sort, scratch from the pool as above; rows
 * still by query number). */
int sp_grid_search(const sp_grid* grid, const float* queries, size_t nq, size_t k, const float* transT,
                   int transT_on_device, int32_t* idx_out, float* d2_out, void* stream);
/* The grid's counterpart of KDTree::radius_search_async (knn/kdtree.hpp:251-280, 574-719): the max_k nearest target
 * points within `radius` of transT*q, ascending, padded with -1 / FLT_MAX; max_k <= 20 (SP_ERR_RUNTIME otherwise).
 * Bit-identical to sp_kdtree_radius_search on tie-free data. */
int sp_grid_radius_search(const sp_grid* grid, const float* queries, size_t nq, size_t max_k, float radius,
                          const float* transT, int transT_on_device, int32_t* idx_out, float* d2_out, void* stream);
/* The grid's counterpart of KDTree::remove_nodes_by_flags (knn/kdtree.hpp:282-284, 721-765) with the same arguments as
 * sp_kdtree_remove_by_flags: flags 1 = keep, 0 = remove; a kept point p is relabelled new_indices[p]; points whose
 * index is >= n_flags are left alone. The cell order survives removal, so the kept points are compacted without a
 * sort and the cell table is rebased (about 0.1 ms per 1M points). Allocates and synchronises; sp_grid_size shrinks.
 * Objects that borrow the grid (sp_gicp_target) must be re-created afterwards. */
int sp_grid_remove_by_flags(sp_grid* grid, const uint8_t* flags, const int32_t* new_indices, size_t n_flags,
                            void* stream);

/* Self-kNN of the cloud a grid was built on, with the covariance / normal estimation optionally fused in
 * (covariance::estimate_async(knn, points, k), feature/covariance.hpp:305-311, and estimate_normals_async(knn, ...),
 * :451-459, when the KNNBase is a GridKNN over the same cloud). Any of idx_out+d2_out / covs_out / normals_out may be
 * NULL; rows are written at the points' ORIGINAL indices. Neighbour lists are bit-identical to sp_knn_bruteforce of the
 * cloud against itself, covariances bit-identical to sp_cov_estimate on those lists. k <= 20.
 * workspace: sp_grid_self_workspace_bytes(grid). */
size_t sp_grid_self_workspace_bytes(const sp_grid* grid);
int sp_grid_self_knn(const sp_grid* grid, size_t k, int32_t* idx_out, float* d2_out, float* covs_out, float* normals_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The same for the queries at grid positions [pos_first, pos_first + pos_count) only (position = index in the grid's cell
 * order, sp_grid_order); the other rows of the outputs are left untouched. This is how the pre-loop (k = 20 neighbours +
 * covariances of the target) is sharded by query over the ranks of a multi-GPU run: every rank holds the
 * whole grid, searches 1/N of the positions, and the covariance rows are exchanged with one all-gather:
 *   sp_grid_gather_rows   rows of this rank's positions, caller's order -> position order (a contiguous chunk to send)
 *   sp_allgather          (multi-GPU section)
 *   sp_grid_scatter_rows  position order -> caller's order, for all positions
 * row_bytes must be a multiple of 16 (a covariance row is 64, a point / normal 16). */
int sp_grid_self_knn_range(const sp_grid* grid, size_t k, size_t pos_first, size_t pos_count, int32_t* idx_out,
                           float* d2_out, float* covs_out, float* normals_out, void* workspace, size_t workspace_bytes,
                           void* stream);
int sp_grid_gather_rows(const sp_grid* grid, const void* rows, size_t row_bytes, size_t pos_first, size_t pos_count,
                        void* out_by_position, void* stream);
int sp_grid_scatter_rows(const sp_grid* grid, const void* in_by_position, size_t row_bytes, size_t pos_first,
                         size_t pos_count, void* rows, void* stream);

/* ------------------------------------------------------------------------------ covariance / normals */

/* covariance::estimate_async (algorithms/feature/covariance.hpp:16-47, 260-311, kernel K5). */
int sp_cov_estimate(const float* points, size_t n, const int32_t* knn_idx, size_t k, float* covs_out, void* stream);
/* covariance::estimate_robust_async (feature/covariance.hpp:97-250, 323-381): M-estimated neighbourhood covariance —
 * weighted estimate, Mahalanobis distances to it, their median (x mad_scale, floored at min_robust_scale) as the scale of
 * the IRLS weights, robust_max_iterations times. k <= 64 ("neighbor K is too large. MAX_K is 64" -> SP_ERR_RUNTIME);
 * robust_type SP_LOSS_NONE is sp_cov_estimate. */
int sp_cov_estimate_robust(const float* points, size_t n, const int32_t* knn_idx, size_t k, int robust_type,
                           float mad_scale, float min_robust_scale, size_t robust_max_iterations, float* covs_out,
                           void* stream);
/* covariance::kernel::normalize_covariance (feature/covariance.hpp:76-95) over a covariance array (in place allowed). */
int sp_cov_normalize(const float* covs, size_t n, float* covs_out, void* stream);
/* covariance::estimate_normals_async (covariance.hpp:49-65, 417-459, kernel K6). */
int sp_normals_from_knn(const float* points, size_t n, const int32_t* knn_idx, size_t k, float* normals_out,
                        void* stream);
/* covariance::extract_normals_async (covariance.hpp:465-503, kernel K7). */
int sp_normals_from_cov(const float* points, const float* covs, size_t n, float* normals_out, void* stream);
/* covariance::kernel::update_covariance_plane applied to a whole array (covariance.hpp:67-74); in place allowed. */
int sp_cov_update_plane(const float* covs, size_t n, float* covs_out, void* stream);

/* ------------------------------------------------------------------- device-built tree (any density profile) */

/* KDTree::build + knn_search_async (algorithms/knn/kdtree.hpp:292-413, 424-562) for callers that rebuild the structure every
 * frame (pipeline/submapping.hpp:197, pipeline/pointcloud_processing.hpp:64) on clouds whose density varies by orders of
 * magnitude (raw LiDAR scans): a bounding-volume hierarchy over the Morton-sorted points, leaves of 16 points, built ENTIRELY on
 * the device (bounding box, 30-bit Morton keys, radix sort, boxes level by level: a fraction of a millisecond per 1M points
 * against 30 ms for the host's recursive nth_element) and balanced by count, so it is indifferent to where the points are
 * (GridKNN is the faster structure on near-uniform clouds, sp_grid_*). sp_bvh_create allocates and synchronises.
 *   sp_bvh_search    exact kNN, 1 <= k <= 32, queries searched at transT * q (NULL: identity; host or device matrix as for
 *                    sp_kdtree_search); rows as KNNResult (knn/result.hpp:12-34): ascending, -1 / FLT_MAX padded; ties to the
 *                    lowest index — bit-identical to sp_knn_bruteforce. The queries may come in any order (400 k or more are
 *                    searched along the tree's own curve, rows still by query number; scratch from the library's pool).
 *   sp_bvh_self_knn  the cloud's own points as queries (row i = neighbours of point i, itself first), walked in tree order. */
typedef struct sp_bvh sp_bvh;
int sp_bvh_create(const float* points, size_t n, void* stream, sp_bvh** out);
void sp_bvh_destroy(sp_bvh* bvh);
size_t sp_bvh_size(const sp_bvh* bvh);
int sp_bvh_search(const sp_bvh* bvh, const float* queries, size_t nq, size_t k, const float* transT, int transT_on_device,
                  int32_t* idx_out, float* d2_out, void* stream);
int sp_bvh_self_knn(const sp_bvh* bvh, size_t k, int32_t* idx_out, float* d2_out, void* stream);
/* KDTree::radius_search_async (knn/kdtree.hpp:574-719) on the device-built hierarchy: per query the max_k (<= 32) nearest of the
 * points within `radius` (squared distance <= radius^2, inclusive as in the reference), ascending, -1 / FLT_MAX padded; ties to
 * the lowest index. Same arguments as sp_kdtree_radius_search. */
int sp_bvh_radius_search(const sp_bvh* bvh, const float* queries, size_t nq, size_t max_k, float radius, const float* transT,
                         int transT_on_device, int32_t* idx_out, float* d2_out, void* stream);
/* KDTree::remove_nodes_by_flags (knn/kdtree.hpp:282-284, 721-765), same arguments as sp_kdtree_remove_by_flags: flags 1 = keep,
 * 0 = remove; a kept point p is relabelled new_indices[p] (an order-preserving relabelling, as FilterByFlags::calculate_indices
 * gives, common/filter_by_flags.hpp:30-57); points whose index is >= n_flags are left alone. Lazy, as in the reference: the
 * removed points stay in their leaves but can no longer be found (no rebuild, no compaction; sp_bvh_size does not change);
 * sp_bvh_self_knn afterwards writes the rows of the kept points at their new indices. Allocates scratch and synchronises. */
int sp_bvh_remove_by_flags(sp_bvh* bvh, const uint8_t* flags, const int32_t* new_indices, size_t n_flags, void* stream);
/* The points the tree was built on, back in their original order (x, y, z, 1): the tree keeps its own copy, like the nodes of
 * the reference's KDTree, so a caller that needs them again later (the facade builds the reference-topology KD-tree lazily,
 * for radius search / lazy delete) does not depend on the source cloud still being there. */
int sp_bvh_export_points(const sp_bvh* bvh, float* points_out, void* stream);

/* ------------------------------------------------------------------- device-built octree (k up to 100) */

/* knn::Octree (algorithms/knn/octree.hpp:27-844) built ENTIRELY on the device (csrc/octree.hip states how), for lists of up to
 * 100 neighbours: the hierarchy (sp_bvh_*) stops at 32, the grid and the brute-force search at 20.
 *   sp_octree_create   Octree::build (octree.hpp:233-274, 388-475, 581-596): the box of the finite points widened by
 *                      max(1e-5, resolution / 2) per side (:267-269); a node splits while it holds more than max_points_per_node
 *                      points, its cell's longest edge exceeds `resolution` and its depth is below 21 (:416-418; the reference
 *                      allows 32, which shows only in leaves of coincident points). Non-finite points go into no leaf and are never
 *                      neighbours, as in sp_knn_bruteforce. Point i gets the id i. Allocates and synchronises; n == 0: an empty
 *                      tree, no device work.
 *   sp_octree_size     size() (:118): the points still kept.
 *   sp_octree_info     SP_OCTREE_NODES, _LEAVES, _DEPTH (the deepest node), _NEXT_ID (the ids in use are below it,
 *                      next_point_id_ :273, :368-379), _SLOTS (entries of sp_octree_export's point_ids_out).
 *   sp_octree_search   knn_search_async (:599-630, 684-844): exact kNN, 0 <= k <= 100, queries searched at transT * q (NULL:
 *                      identity; host or device matrix as for sp_kdtree_search); rows as KNNResult (knn/result.hpp:12-34):
 *                      ascending by (distance, index), -1 / FLT_MAX padded, every entry written; ties to the lowest index
 *                      (bit-identical to sp_knn_bruteforce; the reference's heap leaves the order of ties to its traversal and
 *                      its 32-entry stack drops nodes when full: nothing is dropped here). k > 100 (:629), a null handle or null
 *                      outputs: SP_ERR_INVALID_ARGUMENT before any device work. Enqueue only.
 *   sp_octree_remove_by_flags  remove_nodes_by_flags (:276-380): a stored point with id p is kept iff flags[p] == 1 and
 *                      new_indices[p] >= 0, and is then relabelled new_indices[p]; the others can no longer be found (no
 *                      rebuild; the boxes stay valid supersets). n_flags must equal SP_OCTREE_NEXT_ID (:285-289) and every new
 *                      id of a kept point be below it (:329-332), else SP_ERR_RUNTIME with the reference's text. Afterwards
 *                      SP_OCTREE_NEXT_ID = max(largest new id + 1, points kept) (:368-379); nothing kept: the empty tree with
 *                      next id 0 (:363-366). Synchronises (one 8-byte read-back).
 *   sp_octree_export   for tests and bindings: nodes_out receives 64 bytes per node (:65-80) — box min xyz, box max xyz (the
 *                      tight box of the points below, floats), is_leaf, depth, then the eight child indices (-1: none; always
 *                      above the node's own) or start, count and six zeros; point_ids_out the ids in leaf order (-1: removed).
 *                      Either may be NULL. Device pointers; enqueue only. */
typedef struct sp_octree sp_octree;
enum { SP_OCTREE_NODES = 0, SP_OCTREE_LEAVES = 1, SP_OCTREE_DEPTH = 2, SP_OCTREE_NEXT_ID = 3, SP_OCTREE_SLOTS = 4 };
int sp_octree_create(const float* points, size_t n, float resolution, size_t max_points_per_node, void* stream, sp_octree** out);
void sp_octree_destroy(sp_octree* octree);
size_t sp_octree_size(const sp_octree* octree);
int sp_octree_info(const sp_octree* octree, int what, uint64_t* out);
int sp_octree_search(const sp_octree* octree, const float* queries, size_t nq, size_t k, const float* transT, int transT_on_device,
                     int32_t* idx_out, float* d2_out, void* stream);
int sp_octree_remove_by_flags(sp_octree* octree, const uint8_t* flags, const int32_t* new_indices, size_t n_flags, void* stream);
int sp_octree_export(const sp_octree* octree, void* nodes_out, int32_t* point_ids_out, void* stream);

/* ------------------------------------------------------------------- accelerated KDTree (which structure answers) */

/* KDTree (knn/kdtree.hpp:142-766) with the structure chosen per search: the one object behind the facade's KDTree and
 * sycl_points_amd.api.KDTree(accelerate=True); csrc/knn_tree.hip states the rule. sp_knn_tree_create keeps a copy of the points
 * (stream-ordered, no synchronisation); the reference's tree (below 1024 points: at once, synchronising), the hierarchy
 * (sp_bvh_*) and a grid on the tree's own cloud are built on first need, allocating and synchronising as their creates do.
 *   sp_knn_tree_backend  the structure (SP_KNN_*) sp_knn_tree_search answers the same arguments from; may build the grid.
 *   sp_knn_tree_search   as sp_kdtree_search, k <= 100 (SP_ERR_RUNTIME). own_cloud != 0: the caller states that the queries are
 *                        the points the tree was built on, unchanged since; it counts only while nothing was removed and
 *                        without a transform. transT NULL or a host identity: no transform; a device transT always is one.
 *                        A query with a non-finite coordinate gets a row of (-1, FLT_MAX) from whichever structure answers,
 *                        where the reference's tree writes NaN distances for k > 1.
 *   sp_knn_tree_radius_search / sp_knn_tree_remove_by_flags  as sp_kdtree_*; a removal reaches every structure, also one built
 *                        later, ends the own-cloud, grid and brute-force shortcuts, and synchronises.
 *   sp_knn_tree_set_reference_order  != 0: every search uses the reference's tree (its first-visited tie order).
 *   sp_knn_tree_info     SP_KNN_TREE_*: point count, nothing removed yet, hierarchy built, grid built. */
typedef struct sp_knn_tree sp_knn_tree;
enum { SP_KNN_HOST_TREE = 0, SP_KNN_HIERARCHY = 1, SP_KNN_GRID = 2, SP_KNN_BRUTE_FORCE = 3 };
enum { SP_KNN_TREE_SIZE = 0, SP_KNN_TREE_PRISTINE = 1, SP_KNN_TREE_HIERARCHY_BUILT = 2, SP_KNN_TREE_GRID_BUILT = 3 };
int sp_knn_tree_create(const float* points, size_t n, size_t leaf_threshold, void* stream, sp_knn_tree** out);
void sp_knn_tree_destroy(sp_knn_tree* tree);
int sp_knn_tree_backend(sp_knn_tree* tree, size_t nq, size_t k, const float* transT, int transT_on_device, int own_cloud,
                        void* stream, int* backend_out);
int sp_knn_tree_search(sp_knn_tree* tree, const float* queries, size_t nq, size_t k, const float* transT, int transT_on_device,
                       int own_cloud, int32_t* idx_out, float* d2_out, void* stream);
int sp_knn_tree_radius_search(sp_knn_tree* tree, const float* queries, size_t nq, size_t max_k, float radius,
                              const float* transT, int transT_on_device, int32_t* idx_out, float* d2_out, void* stream);
int sp_knn_tree_remove_by_flags(sp_knn_tree* tree, const uint8_t* flags, const int32_t* new_indices, size_t n_flags,
                                void* stream);
int sp_knn_tree_set_reference_order(sp_knn_tree* tree, int enable);
int sp_knn_tree_info(const sp_knn_tree* tree, int what, uint64_t* out);

/* --------------------------------------------------------------------------------------- voxel grid */

/* filter::kernel::compute_voxel_bit (algorithms/common/voxel_constants.hpp:36-62, kernel K9).
 * inv_voxel_size is 1.0f / voxel_size computed once on the host (filter/voxel_downsampling.hpp:27). */
int sp_voxel_keys(const float* points, size_t n, float inv_voxel_size, uint64_t* keys_out, void* stream);

/* VoxelGrid::downsampling (filter/voxel_downsampling.hpp:50-79, 146-288): per-voxel mean of the points (and of rgb
 * and timestamps, median of intensities, when those attribute pointers are non-NULL), voxels with
 * point_sum.w < min_voxel_count dropped, output in ascending key order. The host std::sort + sequential
 * run-length mean of the reference is replaced by a device radix sort of (key, index) (64-bit keys here: 8 passes; see the
 * boxed form below for the fast path) and a segmented reduction;
 * within a voxel points are summed in ascending index order (the reference's order is unspecified: its sort is
 * unstable). *n_out_dev (a device uint32) receives the voxel count; out arrays must hold n entries and must not overlap
 * the inputs.
 * workspace: sp_voxel_downsample_workspace_bytes(n) bytes. */
size_t sp_voxel_downsample_workspace_bytes(size_t n);
int sp_voxel_downsample(const float* points, size_t n, float inv_voxel_size, size_t min_voxel_count,
                        const float* rgb, const float* intensities, const float* timestamps, float* points_out,
                        float* rgb_out, float* intensities_out, float* timestamps_out, uint64_t* keys_out_opt,
                        uint32_t* n_out_dev, void* workspace, size_t workspace_bytes, void* stream);

/* The same operation with the bounding box of the cloud's voxel coordinates known to the HOST (box6 = min x,y,z, max x,y,z
 * of the 21-bit key fields; sp_voxel_key_box computes it on the device: read it back, or keep the previous scan's box and
 * check *status_dev_opt). The keys are then compressed to the voxel's position in the box — same order — and sorted by
 * exactly the bits the box needs (3 passes of the hand-written radix sort for a 200^3 box; the unboxed call sorts the 64-bit
 * keys in 8 passes of the same sort: the sort is most of the run time). Results are identical to sp_voxel_downsample.
 * *status_dev_opt receives the number of valid points whose voxel lies outside the box: non-zero means the box did not
 * cover the cloud and the outputs must be discarded. A NULL, empty or too large box (>= 2^32 - 1 cells) falls back to the
 * 64-bit path.
 * box_shards_dev_opt (SP_VOXEL_BOX_SHARDS shards of SP_VOXEL_BOX_SHARD_STRIDE ints — one 128-byte line each — of which the
 * first 6 are used): the key kernel also records THIS cloud's coordinate box on the way — fold the shards (min of
 * [s][0..2], max of [s][3..5]; an empty cloud leaves INT32_MAX / INT32_MIN) for the next call's guess, or for the exact box
 * of a redo when *status_dev_opt != 0. No separate pass over the points. */
#define SP_VOXEL_BOX_SHARDS 16
#define SP_VOXEL_BOX_SHARD_STRIDE 32
int sp_voxel_key_box(const float* points, size_t n, float inv_voxel_size, int32_t* box6_dev, void* stream);
int sp_voxel_downsample_boxed(const float* points, size_t n, float inv_voxel_size, size_t min_voxel_count,
                              const float* rgb, const float* intensities, const float* timestamps, float* points_out,
                              float* rgb_out, float* intensities_out, float* timestamps_out, uint64_t* keys_out_opt,
                              uint32_t* n_out_dev, const int32_t* box6_host, uint32_t* status_dev_opt,
                              int32_t* box_shards_dev_opt, void* workspace, size_t workspace_bytes, void* stream);
/* sp_voxel_downsample_boxed with ONE record in place of the status word and the sharded box (VoxelGrid::downsampling,
 * voxel_downsampling.hpp:146-288, frame after frame):
 *   report8 = {voxels written, valid points outside box6 (non-zero: discard the outputs and call again with the box below),
 *              THIS cloud's key box min x, y, z, max x, y, z (INT32_MAX / INT32_MIN when no point is valid)}
 * stored once by the call's last kernel, word 0 LAST and behind a system-scope release: report8 may be the device pointer of
 * host-mapped pinned memory whose word 0 the caller armed with a value no count takes and spins on — no copy, no
 * synchronisation. (The other outputs may still be in flight when word 0 lands; work enqueued on the stream stays ordered
 * behind them.) The key kernel's workgroups leave one record each in the workspace and the last kernel folds them, so there are
 * no atomics to initialise: one launch fewer than the boxed call, two with its read-back. n_out_dev_opt may be NULL. */
int sp_voxel_downsample_report(const float* points, size_t n, float inv_voxel_size, size_t min_voxel_count,
                               const float* rgb, const float* intensities, const float* timestamps, float* points_out,
                               float* rgb_out, float* intensities_out, float* timestamps_out, uint64_t* keys_out_opt,
                               uint32_t* n_out_dev_opt, const int32_t* box6_host, uint32_t* report8, void* workspace,
                               size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------- polar grid */

/* PolarGrid (filter/polar_downsampling.hpp:104-452): VoxelGrid's device path with the polar key in place of the Cartesian one.
 * coord: SP_COORD_LIDAR (azimuth = atan2(y, x), elevation = atan2(z, sqrt(x^2 + y^2))) or SP_COORD_CAMERA (azimuth = atan2(x, z),
 * elevation = atan2(-y, sqrt(x^2 + z^2))), algorithms/common/coordinate_system.hpp. d_inv, e_inv, a_inv: 1.0f / the distance,
 * elevation and azimuth voxel sizes (radians for the angles), computed once on the host (polar_downsampling.hpp:116-118).
 * An invalid coord or an inverse size that is not positive and finite: SP_ERR_INVALID_ARGUMENT. */
enum { SP_COORD_LIDAR = 0, SP_COORD_CAMERA = 1 };

/* kernel::compute_polar_bit<coord> (polar_downsampling.hpp:30-100): DISTANCE in bits 0-20, POLAR (elevation) in 21-41, AZIMUTH
 * in 42-62; ~0 for a non-finite point, r == 0, a zero horizontal term or a field outside [0, 2^21). The angles come from the
 * library's own atan2f (within 2 ulp of the correctly rounded value), not the device's: sp_polar_keys_host computes the same
 * keys bit for bit on the host (points_host, keys_out_host: host memory). */
int sp_polar_keys(const float* points, size_t n, int coord, float d_inv, float e_inv, float a_inv, uint64_t* keys_out,
                  void* stream);
int sp_polar_keys_host(const float* points_host, size_t n, int coord, float d_inv, float e_inv, float a_inv,
                       uint64_t* keys_out_host);
/* sp_voxel_key_box for the polar key: box6 = min, max of the distance, elevation and azimuth fields. */
int sp_polar_key_box(const float* points, size_t n, int coord, float d_inv, float e_inv, float a_inv, int32_t* box6_dev,
                     void* stream);
/* PolarGrid::downsampling (polar_downsampling.hpp:200-236, 316-440): sp_voxel_downsample_report with the polar key — the same
 * 8-word report record (box6_host and report8[2..7] are boxes of the polar fields), the same outputs per voxel (mean of points,
 * rgb and timestamps, median of intensities; point_sum.w < min_voxel_count dropped; ascending key order; within a voxel points
 * summed in ascending index order), the same workspace: sp_voxel_downsample_workspace_bytes(n). The key host std::sort and
 * sequential walk of the reference are replaced by the device radix sort and segmented reduction. */
int sp_polar_downsample_report(const float* points, size_t n, int coord, float d_inv, float e_inv, float a_inv,
                               size_t min_voxel_count, const float* rgb, const float* intensities, const float* timestamps,
                               float* points_out, float* rgb_out, float* intensities_out, float* timestamps_out,
                               uint64_t* keys_out_opt, uint32_t* n_out_dev_opt, const int32_t* box6_host, uint32_t* report8,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------- transform */

/* transform::transform_async (algorithms/common/transform.hpp:14-37, 45-94, kernel K14); in place allowed;
 * covs / normals may be NULL. */
int sp_transform(const float* points, const float* covs, const float* normals, size_t n, const float* transT_host,
                 float* points_out, float* covs_out, float* normals_out, void* stream);

/* deskew::deskew_point_cloud_constant_velocity's kernel (algorithms/deskew/relative_pose_deskew.hpp:120-172): every point is
 * moved from the sensor frame at its own sampling time into the frame at the end of the motion delta_twist6_host (se3_log of
 * the motion over scan_duration_seconds, rotation first, HOST memory). Per point: ts = t_ms * 1e-3f; a non-finite ts copies
 * the row (point, normal, all 16 floats of the covariance); otherwise tau = clamp(ts / scan_duration_seconds, 0, 1),
 * M = se3_exp(twist * tau), p' = M p, n' = (R n, 0), C' = R (C3 R^T) in the top-left 3x3 of a zeroed 4x4, R the rotation of M.
 * covs / normals may be NULL (together with their outputs). In place allowed (*_out == *_in): every row is read before it
 * is written, so an in-place call returns the rotated normals and covariances — the reference, which zeroes its outputs
 * before it reads its inputs, returns zeros there. A null points / timestamp_offsets_ms / points_out / twist, covs or normals
 * given without their output or the other way round, a duration that is not positive and finite, n >= 2^32 ->
 * SP_ERR_INVALID_ARGUMENT before any HIP call. n == 0: SP_OK, nothing enqueued. Enqueue only. */
int sp_deskew_constant_velocity(const float* points, const float* covs, const float* normals,
                                const float* timestamp_offsets_ms, size_t n, const float* delta_twist6_host,
                                float scan_duration_seconds, float* points_out, float* covs_out, float* normals_out,
                                void* stream);
/* se3_log(prev^-1 * cur), inverse and product as Eigen's Isometry3f forms them (relative_pose_deskew.hpp:103-104,
 * pipeline/velocity_update.hpp:71-72): the twist sp_deskew_constant_velocity takes. Poses column-major 4x4. Host only. */
void sp_relative_twist_host(const float* prev_pose16, const float* cur_pose16, float* twist6_out);

/* ------------------------------------------------------------------- IMU preintegration and IMU deskew */

/* imu::IMUPreintegrationParams (algorithms/imu/imu_preintegration.hpp:138-166). */
typedef struct sp_imu_params {
    float gravity[3];  /* world frame, m/s^2; the reference's default is (0, 0, -9.80665) */
    float accel_scale; /* applied to raw accelerations before the bias is subtracted */
    float gyro_noise_density, accel_noise_density, gyro_bias_rw_density, accel_bias_rw_density;
} sp_imu_params;
/* imu::PreintegrationResult with its PreintegrationJacobians (imu_preintegration.hpp:98-135). Matrices column-major
 * (Eigen .data() order); covariance: 15x15, [dp, dphi, dv, dba, dbg]. */
typedef struct sp_imu_state {
    float Delta_R[9], Delta_v[3], Delta_p[3], pad0;
    double dt_total;
    float J_R_bg[9], J_v_bg[9], J_v_ba[9], J_p_bg[9], J_p_ba[9];
    float covariance[225];
} sp_imu_state;

/* imu::IMUPreintegration (imu_preintegration.hpp:180-529) on plain arrays; HOST only, no device is touched. bias6 is
 * (gyro_bias, accel_bias). Kept as in the reference: the midpoint step; the first sample only primes the integrator;
 * a sample whose stamp does not increase is dropped without replacing the previous one; a step with dt < 1e-9 is skipped;
 * Delta_R is renormalised through a quaternion every 100 steps; the covariance step sym(F Sigma F^T + G Qd G^T) is skipped
 * only when every noise density is zero and Sigma is zero (Eigen's isZero(): every |entry| <= 1e-5f). The reference's Eigen
 * products are plain multiply-add sums, k ascending, chains of factors left to right (Eigen's own order is not pinned).
 *   create   a handle in the state of the reference's constructor (no reset needed before the first sample)
 *   reset    :202-212; NULL bias6 = zero bias, NULL covariance225 = zero, NULL R_world_body9 = identity
 *   integrate  :217-230, one sample: absolute stamp in seconds, raw gyro (rad/s) and accel
 *   num_measurements  the samples accepted since the reset (has_measurements() is > 0)
 *   get      bias6 NULL: get_raw (:272); else get_corrected(bias6) (:244-269), the first-order bias correction with its
 *            quaternion round trip (rotation_matrix_to_quaternion, normalize, quaternion_to_rotation_matrix)
 *   predict_relative   predict_relative_transform (:307-330): T_body_i -> body_j, column-major 4x4
 *   predict_transform  predict_transform (:280-295): T_world_body_j
 * A null handle or a null argument not named optional above -> SP_ERR_INVALID_ARGUMENT. */
int sp_imu_preint_create(const sp_imu_params* params, void** handle_out);
void sp_imu_preint_destroy(void* handle);
int sp_imu_preint_reset(void* handle, const float* bias6_host, const float* covariance225_host, const float* R_world_body9_host);
int sp_imu_preint_integrate(void* handle, double timestamp, const float* gyro3_host, const float* accel3_host);
int sp_imu_preint_num_measurements(void* handle);
int sp_imu_preint_get(void* handle, const float* bias6_host, sp_imu_state* state_out);
int sp_imu_preint_predict_relative(void* handle, const float* R_world_body9_host, const float* v_world3_host,
                                   const float* bias6_host, float* T16_out_host);
int sp_imu_preint_predict_transform(void* handle, const float* T_world_body16_host, const float* v_world3_host,
                                    const float* bias6_host, float* T16_out_host);

/* deskew::IMUDeskewStatus (algorithms/deskew/imu_deskew.hpp:32-38) */
#define SP_IMU_DESKEW_SUCCESS 0
#define SP_IMU_DESKEW_INSUFFICIENT_IMU_COVERAGE 1
#define SP_IMU_DESKEW_NO_TIMESTAMPS 2
#define SP_IMU_DESKEW_INVALID_SCAN_DURATION 3
#define SP_IMU_DESKEW_EMPTY_CLOUD 4
/* Steps 1-3 of deskew::deskew_point_cloud_imu (imu_deskew.hpp:158-285), HOST only: the samples within 50 ms of the scan
 * window and the coverage checks; the virtual sample at scan_start_sec (the three lower_bound cases); the identity pose;
 * then one pose per sample with float(stamp - scan_start_sec) >= 0, T_lidar_rel = T_il * T_imu_rel * T_il^-1 with T_imu_rel
 * predict_relative_transform's, or (gyro_only != 0) get_corrected's Delta_R alone; the final coverage check. The rotation
 * becomes a quaternion by the library's rotation_matrix_to_quaternion twin, not Eigen::Quaternionf's constructor (:265).
 * stamps: n absolute seconds, ascending; gyro_accel: n rows of gyro xyz, accel xyz. traj_out: 8 floats per pose (q xyzw, t xyz,
 * stamp in seconds from scan start: deskew::IMUTrajectoryPose), room for `capacity` poses; n + 1 always suffices.
 * *status_out is an SP_IMU_DESKEW_* code (a scan_duration_sec <= 0 is INVALID_SCAN_DURATION); *n_traj_out is the number of
 * poses on SUCCESS, else 0. A null argument or a capacity that is too small -> SP_ERR_INVALID_ARGUMENT. */
int sp_imu_deskew_trajectory_host(const double* stamps_host, const float* gyro_accel_host, size_t n, double scan_start_sec,
                                  double scan_duration_sec, const float* T_imu_to_lidar16_host, const float* bias6_host,
                                  const sp_imu_params* params, const float* R_world_body9_host, const float* v_world3_host,
                                  int gyro_only, float* traj_out_host, size_t capacity, size_t* n_traj_out, int* status_out);
/* What sp_deskew_imu reads: n_traj - 1 rows of 16 floats, one per interval [i, i + 1] of the trajectory:
 * t_lo, t_hi, q0[4], omega[3], t0[3], t1 - t0[3], 0. omega = so3_log(quat_mult(conj(q0), +-q1)), the sign by dot<4>(q0, q1) < 0:
 * the first half of quat_slerp (imu_deskew.hpp:54-73), which the reference evaluates per point although it depends on the
 * interval alone. HOST only. Null pointers or n_traj < 2 -> SP_ERR_INVALID_ARGUMENT. */
int sp_imu_deskew_intervals_host(const float* traj_host, size_t n_traj, float* intervals_out_host);
/* deskew::deskew_point_cloud_imu's kernel (imu_deskew.hpp:330-411). intervals: DEVICE memory, the rows of
 * sp_imu_deskew_intervals_host, 16-byte aligned. Per point: t = t_ms * 1e-3f; a non-finite t copies the row (point, normal, all
 * 16 floats of the covariance); otherwise the reference's bisection (lo = 0, hi = n_intervals, mid = (lo + hi) / 2,
 * stamp[mid] <= t: the same interval as the reference for every table, ordered or not, and no index outside the table),
 * alpha = (t_hi > t_lo) ? clamp((t - t_lo) / (t_hi - t_lo), 0, 1) : 0, q = quat_mult(q0, so3_exp(omega * alpha)),
 * R = quaternion_to_rotation_matrix(q), p' = R p + fma(t1 - t0, alpha, t0) with w carried, n' = (R n, 0), C' = R (C3 R^T) in
 * the top-left 3x3 of a zeroed 4x4. covs / normals may be NULL (together with their outputs). In place allowed
 * (*_out == *_in): every row is read before it is written, so an in-place call returns the rotated normals and covariances -
 * the reference, which zeroes its outputs before it reads its inputs, returns zeros there. A null points /
 * timestamp_offsets_ms / points_out / intervals, covs or normals given without their output or the other way round,
 * n_intervals < 1 or >= 2^31, n >= 2^32 -> SP_ERR_INVALID_ARGUMENT before any HIP call. n == 0: SP_OK, nothing enqueued.
 * Enqueue only. */
int sp_deskew_imu(const float* points, const float* covs, const float* normals, const float* timestamp_offsets_ms, size_t n,
                  const float* intervals, size_t n_intervals, float* points_out, float* covs_out, float* normals_out,
                  void* stream);

/* ------------------------------------------------------------------- scan filters after kNN and covariances */

/* AngleIncidenceFilterOperator::apply's kernel and checks (filter/preprocess_operator/angle_incidence_filter_operator.hpp:23-110):
 * flags_out[i] = 1 keep / 0 remove. A point with a non-finite component is removed; the normal is normals[i] when normals is
 * given (it wins, :73), else extract_normal(p, covs[i]) — the function sp_normals_from_cov stores, so both paths agree bit for
 * bit; dot = dot<3>(p, n), denom = |p| * |n| (frobenius_norm<3>); denom <= 1e-6f is removed; so is |dot / denom| outside
 * [cos(max_angle), cos(min_angle)] (both cosines: std::cos on the host, :55-56). n == 0: SP_OK before any check, nothing enqueued.
 * Neither normals nor covs -> SP_ERR_RUNTIME; min_angle < 0, max_angle > pi/2 or min_angle >= max_angle ->
 * SP_ERR_INVALID_ARGUMENT, both with the reference's text (:27-34). The caller compacts with sp_compact_by_flags_multi on the same
 * stream. Enqueue only. */
int sp_angle_incidence_flags(const float* points, const float* normals, const float* covs, size_t n, float min_angle,
                             float max_angle, uint8_t* flags_out, void* stream);
/* intensity_correction::correct_intensity (filter/intensity_correction.hpp:20-135), in place:
 * I' = clamp(I * pow(|p| / ref_distance, exponent) * angle_factor * scale, min_intensity, max_intensity), the products in that
 * order (:34-37); angle_factor = pow(max(|cos|, 1e-3f), -angle_exponent) with the cosine of sp_angle_incidence_flags, and 1 when
 * angle_exponent == 0, when neither normals nor covs is given, or when denom <= 1e-6f. Normals win over covs (:100-128).
 * n == 0: SP_OK before any check. exponent < 0, ref_distance <= 0, a null intensities -> SP_ERR_RUNTIME with the reference's
 * text (:60-68). Enqueue only. */
int sp_intensity_correct(const float* points, const float* normals, const float* covs, float* intensities, size_t n,
                         float exponent, float scale, float min_intensity, float max_intensity, float ref_distance,
                         float angle_exponent, void* stream);
/* intensity_gaussian::kernel::compute (filter/intensity_gaussian.hpp:37-86) when mean_min <= 0: out[i] = sum w I / sum w over the
 * first k_use entries of row i of knn_indices (rows of k_stride entries), w = exp(-(dr^2 inv2_r + daz^2 inv2_az + del^2 inv2_el))
 * in the sensor-local basis of point i, inv2 = 0.5f / sigma^2 formed on the host; |p| < 1e-6f and sum w == 0 give I[i].
 * intensity_local_mean_norm::kernel::compute (filter/intensity_local_mean_norm.hpp:26-32) when mean_min > 0:
 * out[i] = I[i] / fmax(that mean, mean_min). A neighbour index outside [0, n) is skipped (the reference reads out of bounds;
 * KNNResult pads with -1). intensities_out must not be intensities_in (SP_ERR_INVALID_ARGUMENT): the kernel reads neighbours.
 * k_stride < 1, a sigma <= 0, a null intensities_in -> SP_ERR_RUNTIME with the text of the function mean_min selects (:103-111 /
 * :60-71); k_use outside [1, k_stride], n >= 2^31 -> SP_ERR_INVALID_ARGUMENT. n == 0: SP_OK before any check. Enqueue only. */
int sp_intensity_gaussian(const float* points, const float* intensities_in, const int32_t* knn_indices, size_t n, size_t k_stride,
                          size_t k_use, float sigma_azimuth, float sigma_elevation, float sigma_range, float mean_min,
                          float* intensities_out, void* stream);
/* intensity_zscore::kernel::compute (filter/intensity_zscore.hpp:17-32): over the first k_use entries of row i of knn_indices
 * (rows of k_stride entries), sum I and sum I^2 in index order, mean = sum I / float(k_use),
 * var = fmax(sum I^2 / float(k_use) - mean * mean, 0), sigma = sqrt(var); out[i] = 0 when sigma < sigma_min, else
 * (I[i] - mean) / sigma. A neighbour index outside [0, n) contributes nothing and the divisor stays k_use (the reference reads out
 * of bounds; KNNResult pads with -1). intensities_out must not be intensities_in (SP_ERR_INVALID_ARGUMENT): the kernel reads
 * neighbours; the caller swaps the new array in (:55-71). A null intensities_in, k_use < 3 -> SP_ERR_RUNTIME with the reference's
 * texts (:44, :52), in its order; a null knn_indices / intensities_out, k_use > k_stride, n >= 2^31 -> SP_ERR_INVALID_ARGUMENT.
 * n == 0: SP_OK before any check (:42). Every error is returned before any HIP call. Enqueue only. */
int sp_intensity_zscore(const float* intensities_in, const int32_t* knn_indices, size_t n, size_t k_stride, size_t k_use,
                        float sigma_min, float* intensities_out, void* stream);

/* ------------------------------------------------------------------- outlier filters on a kNN result of the cloud on itself */

/* OutlierRemoval::statistical's three kernels (filter/outlier_removal_filter.hpp:54-137) as three launches on `stream`, without the
 * reference's three waits and its host reads in between. knn_d2: n rows of k_stride SQUARED distances, ascending, FLT_MAX padding
 * (a KNNResult's distances); they are summed as they are (:78-84), so a padded row sums to inf or a huge value, as the reference's.
 *   mean_dist_out[i] = (d2[i][0] + ... + d2[i][k_use-1]) / float(k_use), in index order
 *   g = sum_i mean_dist_out[i] / float(n),  var = sum_i (g - mean_dist_out[i])^2 / float(n),  thr = g + stddev_mul * sqrt(var)
 *   flags_out[i] = mean_dist_out[i] > thr ? 0 (remove) : 1 (keep);   stats_out = {g, var, thr, float(n)} (device memory)
 * The two sums over i run in a fixed order (per lane, inside a wave, over the waves, over at most 1024 workgroups) that depends
 * on n and k_stride only: no float atomics, the same bits from every call on the same input (the reference's sycl::reduction has
 * no specified order). workspace: sp_outlier_workspace_bytes(n) bytes of device memory, 16-byte aligned.
 * n == 0: SP_OK, nothing enqueued. A null pointer, a workspace that is too small, k_use == 0, k_use > k_stride, k_stride > 2048,
 * n >= 2^31 -> SP_ERR_INVALID_ARGUMENT before any HIP call. The caller compacts with sp_compact_by_flags_multi on the same stream.
 * Enqueue only. */
size_t sp_outlier_workspace_bytes(size_t n);
int sp_outlier_statistical_flags(const float* knn_d2, size_t n, size_t k_stride, size_t k_use, float stddev_mul,
                                 uint8_t* flags_out, float* mean_dist_out /* n floats */, float* stats_out /* 4 floats, device */,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* OutlierRemoval::radius's kernel (filter/outlier_removal_filter.hpp:168-191): flags_out[i] = knn_d2[i][column] > radius ? 0 : 1
 * with column = min_k of rows of min_k + 1 entries. The SQUARED distance is compared with `radius` itself, as the reference
 * compares them (:178, :187-188). n == 0: SP_OK. A null pointer, column >= k_stride, n >= 2^31 -> SP_ERR_INVALID_ARGUMENT before
 * any HIP call. Enqueue only. */
int sp_outlier_radius_flags(const float* knn_d2, size_t n, size_t k_stride, size_t column, float radius, uint8_t* flags_out,
                            void* stream);

/* BoxFilterOperator kernel (filter/preprocess_operator/box_filter_operator.hpp:36-44, common.hpp:15-25, K10):
 * flags_out[i] = 1 keep / 0 remove. */
int sp_box_filter_flags(const float* points, size_t n, float min_distance, float max_distance, uint8_t* flags_out,
                        void* stream);
/* FilterByFlags (algorithms/common/filter_by_flags.hpp:30-57, 87-99) on the device: stable compaction of rows of
 * `row_bytes` bytes; new_indices_out_opt[i] = new index or -1; *n_out_dev = kept count.
 * workspace: sp_compact_workspace_bytes(n). */
size_t sp_compact_workspace_bytes(size_t n);
int sp_compact_by_flags(const void* rows, size_t n, size_t row_bytes, const uint8_t* flags, void* rows_out,
                        int32_t* new_indices_out_opt, uint32_t* n_out_dev, void* workspace, size_t workspace_bytes,
                        void* stream);
/* The same for several attribute arrays of one cloud at once (FilterByFlags is applied to points, covariances, normals, ...
 * in turn, preprocess_operator_base / filter_by_flags.hpp:87-99): ONE scan of the flags, one compaction launch per array,
 * one count. n_arrays <= 16; rows[a] has rows of row_bytes[a] bytes and goes to rows_out[a] (host arrays of device pointers). */
int sp_compact_by_flags_multi(const void* const* rows, const size_t* row_bytes, void* const* rows_out, int n_arrays, size_t n,
                              const uint8_t* flags, int32_t* new_indices_out_opt, uint32_t* n_out_dev, void* workspace,
                              size_t workspace_bytes, void* stream);

/* BoxFilter + FilterByFlags in one launch (+ one that zeroes the scan's state): the box test of sp_box_filter_flags on `points`,
 * the exclusive scan of its flags by decoupled look-back and the stable move of the kept rows of every attribute array — what
 * PreprocessFilter::box_filter does with a cloud (preprocess_operator/box_filter_operator.hpp:24-54 + common/filter_by_flags.hpp:
 * 30-57: a flags kernel, then one filter_by_flags per attribute). flags_out_opt receives the flags (1 keep, 0 remove), the other
 * arguments are sp_compact_by_flags_multi's (rows_out[a] == NULL: that array is not moved). Only enqueues. */
int sp_box_filter_compact_multi(const float* points, size_t n, float min_distance, float max_distance, const void* const* rows,
                                const size_t* row_bytes, void* const* rows_out, int n_arrays, uint8_t* flags_out_opt,
                                int32_t* new_indices_out_opt, uint32_t* n_out_dev, void* workspace, size_t workspace_bytes,
                                void* stream);

/* Rows picked by index, every attribute of a cloud in ONE launch: rows_out[a][j] = rows[a][indices[j]] for j < m (indices:
 * device memory, uint32). What random sampling is once the host has drawn its sample (preprocess_operator/
 * random_sampling_operator.hpp:24-51 draws on the host, then filters by flags, common/filter_by_flags.hpp:30-57: with the indices
 * in ascending order the result is that compaction's, without scanning the flags of the whole cloud per attribute).
 * n_arrays <= 16, row_bytes[a] a multiple of 4. Only enqueues. */
int sp_gather_rows_multi(const void* const* rows, const size_t* row_bytes, void* const* rows_out, int n_arrays,
                         const uint32_t* indices, size_t m, void* stream);

/* Farthest point sampling (filter/preprocess_operator/farthest_point_sampling_operator.hpp:27-91), the chain of argmax
 * decisions on the device: the reference runs a parallel_for, a wait and a host std::max_element over all n distances per
 * sample; here no sample goes back to the host. points: float4[n]; d[] starts at FLT_MAX; sample 0 is first_index (the
 * reference draws it from the operator's own std::mt19937, :51-53), then sampling_num - 1 steps of
 *   d[i] = sycl::min(d[i], |p[i] - p[sel]|^2)   (the fma chain over x, y, z AND w, eigen_utils.hpp:245-253, :333-335; the
 *                                                min is (y < x) ? y : x, so a NaN distance leaves d[i] as it was)
 *   sel  = the FIRST index of max d             (std::max_element: the lowest index wins a tie)
 * order_out[i] = the i-th selected index, repeats included (a cloud whose remaining distances are all 0 selects the same
 * index again); flags_out_opt[i] = 1 when i was selected, else 0; min_d2_out_opt = d after the last step. Bit-identical to
 * the reference. n == 0 or >= 2^32, a null points / order_out / workspace, first_index >= n, sampling_num == 0 or > n ->
 * SP_ERR_INVALID_ARGUMENT before any HIP call. Only enqueues (graph-capturable: under capture it takes a form whose
 * workgroups never wait for each other). workspace: sp_fps_workspace_bytes(n, sampling_num).
 *   sp_fps_status   clouds of 16 k to 2 M points may run as ONE persistent launch whose workgroups wait for each other; every
 *                   wait is bounded, and one that runs out (another process holding compute units) leaves the sample
 *                   incomplete and sets a status word in the workspace. This call reads it (it synchronises the stream):
 *                   SP_OK, or SP_ERR_RUNTIME, after which the next sp_farthest_point_sampling on the device takes a form
 *                   without waits: call it again. */
size_t sp_fps_workspace_bytes(size_t n, size_t sampling_num);
int sp_farthest_point_sampling(const float* points, size_t n, size_t sampling_num, uint32_t first_index, uint32_t* order_out,
                               uint8_t* flags_out_opt, float* min_d2_out_opt, void* workspace, size_t workspace_bytes,
                               void* stream);
int sp_fps_status(const void* workspace, void* stream);

/* Weighted and mixed random sampling (filter/preprocess_operator/weighted_sampling_operator.hpp:29-95,
 * mixed_random_sampling_operator.hpp:28-105). The reference loops over every point on the host (a std::log, a std::mt19937 draw
 * and a std::priority_queue step per positive weight, then a pass over all flags); here the host only draws, in the order the
 * reference draws, and the per-point work, the selection and the flags are the device's. All pointers but none are device
 * memory; every call only enqueues on `stream` (graph-capturable). n == 0 or >= 2^32, a null pointer, a short workspace, m == 0
 * or > n, n_positions == 0 or > n -> SP_ERR_INVALID_ARGUMENT before any HIP call.
 *   sp_weight_check  the checks of :43-61 (mixed: :57-62) in one pass: report_dev[0] = the number of weights > 0, report_dev[1]
 *                    = the lowest index of a weight that is not finite or < 0, 0xffffffff when there is none. The caller reads
 *                    the two words back: the only read-back a sampling call needs.
 *   sp_weighted_sample_flags  the loop of :67-90 (mixed: :51-80), Efraimidis-Spirakis. u_by_rank[j] is the draw of the j-th
 *                    point with a positive weight, in index order (std::uniform_real_distribution<float>(FLT_MIN, 1) on the
 *                    operator's generator; at least as many entries as there are positive weights). key = log(u) / w with the
 *                    correctly rounded binary32 logarithm and the IEEE division; the m largest keys are kept:
 *                    flags_out[i] = 1 keep / 0 remove. Equal keys at the threshold are kept as the reference's min-heap of
 *                    (key, index) keeps them, which replaces its top only when top.key < key: with K the m-th largest key and
 *                    c = m - #{key > K}, of the points with key == K that are among the first m points (index order) with
 *                    key >= K, the c with the highest indices. Fewer than m positive weights: all of them are kept (:66-69 of
 *                    the mixed operator). *selected_count_dev_opt = the number kept, min(m, positive weights). A pure function
 *                    of (weights, u_by_rank, m). workspace: sp_weighted_sample_workspace_bytes(n), 4 bytes per point.
 *   sp_uniform_fill_flags  the uniform part of the mixed operator (:82-99) once the host has run its partial Fisher-Yates on
 *                    positions: for every p in positions_sorted (ascending, distinct) the p-th point, counted from 0 in index
 *                    order, whose flag is not 1 gets flag 1; a p past the last such point selects nothing. workspace:
 *                    sp_uniform_fill_workspace_bytes(n). */
int sp_weight_check(const float* weights, size_t n, uint32_t* report_dev, void* stream);
size_t sp_weighted_sample_workspace_bytes(size_t n);
int sp_weighted_sample_flags(const float* weights, const float* u_by_rank, size_t n, size_t m, uint8_t* flags_out,
                             uint32_t* selected_count_dev_opt, void* workspace, size_t workspace_bytes, void* stream);
size_t sp_uniform_fill_workspace_bytes(size_t n);
int sp_uniform_fill_flags(uint8_t* flags, size_t n, const uint32_t* positions_sorted, size_t n_positions, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------- registration */

/* RegType (algorithms/registration/factor.hpp:18-32) and RobustLossType (algorithms/robust/robust.hpp:13-19). */
enum { SP_REG_POINT_TO_POINT = 0, SP_REG_POINT_TO_PLANE = 1, SP_REG_POINT_TO_DISTRIBUTION = 2, SP_REG_GICP = 3,
       SP_REG_GENZ = 4 };
enum { SP_LOSS_NONE = 0, SP_LOSS_HUBER = 1, SP_LOSS_TUKEY = 2, SP_LOSS_CAUCHY = 3, SP_LOSS_GEMAN_MCCLURE = 4 };

/* The reduced linear system, the 176 bytes the reference keeps in LinearizedDevice
 * (algorithms/registration/registration.hpp:26-84): H row-major, b, error, inlier count.
 * inlier_lo/inlier_hi carry the same count as two exactly-representable floats (count = hi*4096 + lo) so that a
 * float sum all-reduce over ranks stays exact. */
typedef struct sp_linearized {
    float H[36];
    float b[6];
    float error;
    uint32_t inlier;
    float inlier_lo;
    float inlier_hi;
    float pad[2];
} sp_linearized; /* 192 bytes */

typedef struct sp_factor_params { /* RegistrationFactorParams, registration_params.hpp:46-71 */
    int reg_type;
    int robust_type;
    float max_correspondence_distance;
    float robust_scale;
    float genz_alpha;               /* Registration::genz_alpha_ (registration.hpp:370,519) */
    float genz_planarity_threshold; /* registration_params.hpp:52-54 */
    /* RotationConstraint (registration_params.hpp:56-64; rotation_constraint.hpp:15-128): when enabled every inlier
     * correspondence adds the Jensen-Bregman LogDet divergence of (R Cs R^T, Ct), weighted by
     * rotation_constraint_weight and the robust kernel at rotation_robust_scale, to H, b and the error
     * (registration.hpp:630-650, 758-766). Needs source and target covariances. Only the unfused entry points
     * (sp_gicp_linearize / sp_gicp_error) carry the term; the prepared / one-call paths reject it. */
    int rotation_constraint_enable;
    float rotation_constraint_weight;
    float rotation_robust_scale;
} sp_factor_params;

/* Registration::linearize_parallel_reduction_async (registration.hpp:513-664, kernel K11): for every source point
 * whose neighbour distance nn_d2 <= max_corr^2, linearise the factor (factor.hpp:69-449), apply the robust weight
 * (robust.hpp:56-114) and sum H, b, error, inlier count into *out. src_covs / tgt_covs / tgt_normals may be NULL
 * where the reg_type does not need them (registration.hpp:539-543: Identity / Zero are substituted).
 * transT: current pose, host or device (transT_on_device). workspace: sp_gicp_workspace_bytes(n).
 * The reduction is a fixed tree: two runs on the same inputs give bit-identical sums. */
size_t sp_gicp_workspace_bytes(size_t n);
int sp_gicp_linearize(const float* src_points, const float* src_covs, size_t n, const float* tgt_points,
                      const float* tgt_covs, const float* tgt_normals, const int32_t* nn_idx, const float* nn_d2,
                      const float* transT, int transT_on_device, const sp_factor_params* params, sp_linearized* out,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Registration::compute_error_parallel_reduction (registration.hpp:678-777, kernel K12): out->error, out->inlier. */
int sp_gicp_error(const float* src_points, const float* src_covs, size_t n, const float* tgt_points,
                  const float* tgt_covs, const float* tgt_normals, const int32_t* nn_idx, const float* nn_d2,
                  const float* transT, int transT_on_device, const sp_factor_params* params, sp_linearized* out,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Registration::compute_icp_robust_weights_async (registration.hpp:412-462, kernel K13). */
int sp_icp_robust_weights(const float* src_points, const float* src_covs, size_t n, const float* tgt_points,
                          const float* tgt_covs, const float* tgt_normals, const int32_t* nn_idx, const float* nn_d2,
                          const float* transT, int transT_on_device, const sp_factor_params* params,
                          float* weights_out, void* stream);
/* Registration::compute_genz_alpha (registration.hpp:464-511): writes {inlier, planar} counts to counts_out[2]. */
int sp_genz_counts(const float* tgt_covs, const int32_t* nn_idx, const float* nn_d2, size_t n, float max_corr,
                   float planarity_threshold, uint32_t* counts_out, void* stream);

/* Prepared / fused GICP iteration (MI355X-native form of registration.hpp:229-234 = NN search + K11 in one pass).
 * The reference recomputes covariance::kernel::update_covariance_plane for both covariances of every correspondence in
 * every iteration (factor.hpp:249-255). The result depends on the covariance alone, so here it is computed once:
 *   sp_gicp_target_create : plane-regularised target covariances, packed 8 floats per point
 *                           (xx,xy,xz,yy | yz,zz,rho^2,0) and stored in the cell order of `grid` (which must have been built
 *                           on the target points and must outlive the object); sp_gicp_target_update recomputes in place.
 *                           rho = half the distance from the point to its nearest other target point (one k = 2
 *                           self-search on the grid; create allocates and synchronises): the iteration kernel keeps a
 *                           source point's previous correspondence t without searching when |T p - t| < rho_t, which
 *                           proves t is still the exact nearest neighbour.
 *   sp_gicp_source_create : buffers for a prepared source of up to n_max points (allocates).
 *   sp_gicp_source_prepare: (enqueue only) packed plane-regularised source covariances. sort_by_cell selects how
 *                           neighbouring lanes get neighbouring cells (their loads then share cache lines):
 *                             SP_SOURCE_ORDER_UNKNOWN (0) keep the caller's order, assume nothing (ring-walk search);
 *                             SP_SOURCE_SORT (1) reorder by the target-grid cell that transT*p falls into
 *                               (two radix-sort passes per alignment);
 *                             SP_SOURCE_PRESORTED (2) keep the caller's order, which is already spatially coherent —
 *                               sp_grid_order of any grid on the source, or the output order of voxel downsampling —
 *                               no sort, block-walk search: the fastest combination.
 *                           The order only changes which lane handles which point, never a result.
 *   sp_gicp_iteration_fused: per source point q = T p -> exact NN on the grid -> linearise with the packed
 *                           covariances -> reduce to *out. If nn_idx_out/nn_d2_out are non-NULL the correspondences
 *                           are also written, in ORIGINAL source order (for sp_gicp_error / compute_error_frozen); with
 *                           NULL outputs (here and in sp_gicp_align_*) the search is bounded by
 *                           max_correspondence_distance — a neighbour beyond it would be rejected anyway, so a source
 *                           point without a correspondence costs one block of cells instead of a walk out to wherever its
 *                           nearest target point is (clouds that only partly overlap). If
 *                           `gn` is non-NULL (single-GPU loops) the same launch also solves (H + lambda I) delta = -b
 *                           and updates the DEVICE pose transT in place, writing delta_out8 as sp_gn_update does; with
 *                           gn == NULL the caller all-reduces *out over ranks and calls sp_gn_update.
 * Same mathematics as sp_grid_search + sp_gicp_linearize; rounding differs (symmetric packing, upper-triangle H,
 * summation order). reg_type must be SP_REG_GICP or SP_REG_POINT_TO_DISTRIBUTION (the one the target was prepared for,
 * sp_gicp_target_prepare); every robust loss is supported. */
typedef struct sp_gicp_target sp_gicp_target;
typedef struct sp_gicp_source sp_gicp_source;
typedef struct sp_gn_params { float lambda, crit_rotation, crit_translation; } sp_gn_params;
enum { SP_SOURCE_ORDER_UNKNOWN = 0, SP_SOURCE_SORT = 1, SP_SOURCE_PRESORTED = 2 };
int sp_gicp_target_create(const sp_grid* grid, const float* tgt_covs, size_t n, void* stream, sp_gicp_target** out);
int sp_gicp_target_update(sp_gicp_target* target, const float* tgt_covs, void* stream);
/* The same without the reuse certificates (no k = 3 self-search: a fifth of the cost at 6 k points, where the search is
 * 0.1 ms of launch-bound work): every linearisation then searches every point, starting from its previous winner. What a
 * caller wants for a target it aligns ONE small source against — the reference's example builds a new target per frame and
 * aligns a 1000-point sample to it. sp_gicp_target_certify adds the certificates later (a target that turns out to be reused);
 * it synchronises, rewrites the rows and invalidates the correspondence caches of prepared sources. */
int sp_gicp_target_create_plain(const sp_grid* grid, const float* tgt_covs, size_t n, void* stream, sp_gicp_target** out);
int sp_gicp_target_certify(sp_gicp_target* target, const float* tgt_covs, void* stream);
int sp_gicp_target_has_certificates(const sp_gicp_target* target);
/* The same, choosing the factor the rows serve: SP_REG_GICP (what create makes: V diag(1e-3,1,1) V^T of the covariance) or
 * SP_REG_POINT_TO_DISTRIBUTION (linearize_point_to_distribution, factor.hpp:311-373: the information matrix itself,
 * inverse(Ct) of the RAW covariance, Zero when |det| < 1e-6, so the iteration inverts nothing per point and reads no source
 * covariance — sp_gicp_source_prepare then accepts src_covs == NULL). sp_gicp_target_update keeps the current choice. The
 * iteration / align / error entry points require params->reg_type to match (SP_ERR_INVALID_ARGUMENT otherwise). */
int sp_gicp_target_prepare(sp_gicp_target* target, const float* tgt_covs, int reg_type, void* stream);
void sp_gicp_target_destroy(sp_gicp_target* target);
int sp_gicp_source_create(size_t n_max, sp_gicp_source** out);
int sp_gicp_source_prepare(sp_gicp_source* source, const sp_gicp_target* target, const float* src_points,
                           const float* src_covs, size_t n, const float* transT, int transT_on_device, int sort_by_cell,
                           void* stream);
void sp_gicp_source_destroy(sp_gicp_source* source);
int sp_gicp_iteration_fused(const sp_gicp_target* target, const sp_gicp_source* source, float* transT,
                            int transT_on_device, const sp_factor_params* params, const sp_gn_params* gn,
                            int32_t* nn_idx_out, float* nn_d2_out, sp_linearized* out, float* delta_out8,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Registration::compute_error_parallel_reduction (registration.hpp:678-777, kernel K12) on the prepared path: the error of
 * the factor at transT_trial with the correspondences FROZEN at those of the last linearisation of `source` against
 * `target` (sp_gicp_iteration_fused / sp_gicp_align_*), read from the source's correspondence cache — what the trial steps
 * of optimize_levenberg_marquardt (:830-895) and optimize_powell_dogleg (:897-965) call per step. transT_lin_host is the
 * pose of that linearisation (host, column-major): the inlier gate nn_d2 <= max_corr^2 is evaluated there, as the
 * reference's frozen distances are. out->error / out->inlier (H, b are not written). SP_ERR_RUNTIME when nothing has
 * been linearised since sp_gicp_source_prepare. workspace: sp_gicp_workspace_bytes(n). */
int sp_gicp_error_prepared(const sp_gicp_target* target, const sp_gicp_source* source, const float* transT_lin_host,
                           const float* transT_trial, int trial_on_device, const sp_factor_params* params,
                           sp_linearized* out, void* workspace, size_t workspace_bytes, void* stream);
/* Registration::align's whole Gauss-Newton loop (registration.hpp:229-276) enqueued by ONE call; pose, convergence flag and
 * iteration count stay in a state block of the workspace, nothing is read back by the host. Per iteration:
 *   streaming launch its first act finishes the PREVIOUS iteration, in every workgroup for itself: the previous launch's
 *                    partial rows summed in a fixed order, (H + lambda I) delta = -b solved, T <- T * se3_exp(delta)
 *                    (workgroup 0 publishes the state); then every point: cached correspondence when its reuse certificate
 *                    holds, else exact NN on the grid -> linearise -> one partial row per workgroup.
 *   after the last   a one-workgroup launch finishes the last iteration the same way and writes the outputs.
 * Once is_converged() (registration.hpp:407-410) holds, the remaining launches return at once, as the reference breaks out
 * of its loop. All pointers are device memory:
 *   transT_device  in: initial guess, out: final pose (column-major 4x4)
 *   lin_out        system of the last executed iteration (optional)
 *   delta_out8     its delta[6], converged flag, solve-ok flag (optional)
 *   iterations_out number of Gauss-Newton steps applied (optional); the reference's result.iterations is this - 1
 *   nn_idx_out / nn_d2_out: neighbours of the last linearisation, in original source order (optional, both or none)
 * Workspace: sp_gicp_workspace_bytes(n). Graph-capturable. */
int sp_gicp_align_fused(const sp_gicp_target* target, const sp_gicp_source* source, float* transT_device,
                        const sp_factor_params* params, const sp_gn_params* gn, int max_iterations,
                        int32_t* nn_idx_out, float* nn_d2_out, sp_linearized* lin_out, float* delta_out8,
                        uint32_t* iterations_out, void* workspace, size_t workspace_bytes, void* stream);
/* The same loop one iteration at a time, for callers that put something between the iterations — on several GPUs (source
 * tile-sharded, target replicated) an all-reduce:
 *   for k in 0 .. max_iterations-1:  sp_gicp_align_step(k)                       (enqueue iteration k)
 *                                    all-reduce(sum) sp_gicp_align_rows(ws, k)   (32 KB of float32, in place, same stream order)
 *   sp_gicp_align_finish(last_k = max_iterations-1)
 * rows_all_reduced == 0: one GPU, the loop of sp_gicp_align_fused (iteration k is finished by step k + 1, or by finish:
 * lin_out and the state block describe iteration k only from then on). With rows_all_reduced != 0 the streaming launch leaves
 * its sums for the collective, and launch k + 1 (after the last one: finish) finishes iteration k from the all-reduced sums
 * in its prologue — the same sums and the same solve on every rank, hence the identical pose without a broadcast.
 * rows_all_reduced == 1: all partial rows travel (inlier counts as float VALUES, exact: < 2^24 per row); every rank must
 * all-reduce all of sp_gicp_align_rows' floats (rows a rank does not use are zeroed by step 0). All ranks must pass the same
 * rows_all_reduced. transT_device must not be written between step 0 and finish. */
int sp_gicp_align_step(const sp_gicp_target* target, const sp_gicp_source* source, float* transT_device,
                       const sp_factor_params* params, const sp_gn_params* gn, int k, int rows_all_reduced,
                       int32_t* nn_idx_out, float* nn_d2_out, sp_linearized* lin_out, void* workspace,
                       size_t workspace_bytes, void* stream);
float* sp_gicp_align_rows(void* workspace, int k, size_t* n_floats_out);
/* rows_all_reduced == 2 (the form sp_gicp_align_sharded uses): the launch reduces its own partial rows to ONE 128-byte row
 * inside the kernel — every workgroup stores its row write-through and takes an agent-scope ticket; the last arriver sums
 * the rows in the fixed order of the single-GPU loop (bit-identical to it) — and the caller all-reduces just
 * sp_gicp_align_row(ws, k): 28 sums, the inlier count as two exactly-summable floats (hi * 4096 + lo), the searched-point
 * count. */
float* sp_gicp_align_row(void* workspace, int k, size_t* n_floats_out);
int sp_gicp_align_finish(const sp_gicp_source* source, float* transT_device, const sp_gn_params* gn, int last_k,
                         int rows_all_reduced, sp_linearized* lin_out, float* delta_out8, uint32_t* iterations_out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Pose of the LAST LINEARISATION of an alignment enqueued through sp_gicp_align_* with last iteration index last_k (the
 * pose before the final update; the pose at which convergence was detected when the loop stopped early): what the
 * reference's neighbors_ are frozen at after align() (registration.hpp:229-234), i.e. the transT_lin of a following
 * sp_gicp_error_prepared / Registration::compute_error_frozen. Copies 16 floats (column-major) to transT_lin_out (host or
 * device memory) in stream order. */
int sp_gicp_align_linearization_pose(const void* workspace, int last_k, float* transT_lin_out, void* stream);
/* Registration::align's optimiser loop for EVERY OptimizationMethod (registration.hpp:201-276 with optimize_gauss_newton
 * :803-828, optimize_levenberg_marquardt :830-895, optimize_powell_dogleg :897-964 and dogleg_step.hpp:35-101) and, in the same
 * launch, the robust-scale annealing of pipeline::RobustAligner around it (pipeline/robust.hpp:78-111: one align() per level,
 * each starting at the pose the previous level ended on) — device-resident: ONE launch whose workgroups loop on the device,
 * ONE read-back (sp_align_result) per alignment. The reference crosses host <-> device twice per Gauss-Newton iteration and
 * 2 + inner tries times per LM iteration (:674-675, :685-686); its own example (LM + Geman-McClure + 3 levels on a 1000-point
 * sample, example_registration.cpp:29-55) is ~60 such round trips.
 *   step "linearise"  every source point: cached correspondence when its reuse certificate holds, else exact NN on the grid
 *                     -> K11 sums (28 floats + inlier count) -> one partial row per workgroup
 *   step "trial"      K12 of the trial pose over the correspondence-cache rows (frozen correspondences, sp_gicp_error_prepared's
 *                     arithmetic) -> one partial row per workgroup
 *   between steps     every workgroup waits for the rows of all workgroups (arrival counter, bounded wait), sums them in a fixed
 *                     order and runs the optimiser's state machine for itself — the same decisions in every workgroup:
 *                       GN      delta = LDLT(H + lambda I).solve(-b); T <- T exp(delta)
 *                       LM      up to lm_max_inner_iterations trials T exp(delta(lambda)): accept on new_error <= current_error
 *                               (lambda /= factor), stop on |new_error - last_error| <= 1e-6, else lambda *= factor
 *                       DOGLEG  compute_dogleg_step; predicted <= 0 -> shrink; one trial; rho < eta1 -> shrink, else accept
 *                               (rho > eta2 and a full step -> grow)
 *                     an outer iteration ends -> is_converged() or max_iterations ends the level -> next robust scale or done.
 * Workgroups have 256 lanes up to 64 K source points (the reference pipeline's default 1000-point random sample: 4 workgroups
 * on 4 compute units) and 1024 beyond; a launch of one workgroup (<= 256 points) needs no counter at all.
 * robust_scales[n_levels] (host, 1 <= n_levels <= SP_OPT_MAX_LEVELS): the robust scale of each level; lambda / trust radius /
 * result fields restart at every level as a fresh align() would. transT_device: in the initial guess, out the final pose.
 * result_device: sp_align_result in device memory, written once at the end (status 0 ok; 2 a wait ran out — not every workgroup
 * of the launch was resident, the pose is NaN: run again after sp_gicp_source_set_persistent(source, 0), which makes this
 * entry point return SP_ERR_RUNTIME "not available" so that the caller takes its per-step loop).
 * Only enqueues. SP_ERR_RUNTIME (nothing enqueued) when the launch cannot be resident now: the grid exceeds the device's compute
 * units, `stream` is capturing, or another stream's persistent launch may still be running. reg_type GICP or
 * POINT_TO_DISTRIBUTION as the target was prepared; no rotation constraint. Workspace: sp_gicp_workspace_bytes(n). */
enum { SP_OPT_GAUSS_NEWTON = 0, SP_OPT_LEVENBERG_MARQUARDT = 1, SP_OPT_POWELL_DOGLEG = 2 }; /* OptimizationMethod, registration_params.hpp:17-21 */
enum { SP_OPT_MAX_LEVELS = 8, SP_OPT_LOG_ENTRIES = 64 };
typedef struct sp_opt_params { /* RegistrationParams: optimization_method, max_iterations, criteria, gn, lm, dogleg (registration_params.hpp:74-114) */
    int method;
    int max_iterations;
    float crit_rotation, crit_translation;
    float gn_lambda;
    int lm_max_inner_iterations;
    float lm_lambda_factor, lm_init_lambda, lm_max_lambda, lm_min_lambda;
    float dl_initial_radius, dl_min_radius, dl_max_radius, dl_eta1, dl_eta2, dl_gamma_decrease, dl_gamma_increase;
} sp_opt_params;
typedef struct sp_opt_log_entry { /* one outer iteration */
    uint16_t level, iteration;
    uint16_t trials;     /* K12 evaluations of this iteration */
    uint16_t accepted;   /* 1 the pose moved (LM: new_error <= current_error; dog-leg: rho >= eta1; GN: always), 2 LM's
                            stagnation exit (|new_error - last_error| <= 1e-6: pose taken, `updated` false), 0 rejected */
    float damping;       /* lambda (LM) / trust-region radius (dog-leg) AFTER the iteration */
    float error;         /* RegistrationResult::error after the iteration */
} sp_opt_log_entry;
#define SP_ALIGN_RESULT_DONE 0x600DF00Du
typedef struct sp_align_result { /* RegistrationResult (result.hpp:12-28) of the LAST level + what the facade needs beside it */
    float T[16];         /* final pose, column-major */
    float T_lin[16];     /* pose of the last linearisation: the correspondence cache is frozen at it (compute_error_frozen) */
    float H[36];         /* row-major */
    float b[6];
    float error;         /* RegistrationResult::error (GN / dog-leg: of the last linearisation unless a trial was accepted) */
    float error_raw;     /* error of the last linearisation (RegistrationResult::error_raw; H_raw = H, b_raw = b on this path) */
    uint32_t inlier;
    uint32_t iterations; /* index of the last outer iteration of the last level (RegistrationResult::iterations) */
    uint32_t converged;
    uint32_t status;     /* 0 ok, 2 a wait between steps ran out (pose NaN) */
    uint32_t linearizations, trials; /* steps executed, all levels */
    uint32_t searched;   /* source points searched for, all linearisations (the rest reused their correspondence) */
    float damping;       /* final lambda / trust-region radius */
    uint32_t log_entries;
    uint32_t pad[3];     /* pad[0] = SP_ALIGN_RESULT_DONE, stored LAST (system-scope release) when the block is complete: result_device
                          * may be the device pointer of host-mapped pinned memory whose pad[0] the caller cleared and spins on — no
                          * read-back copy, no synchronisation (transT_device may be host-mapped too: 64 bytes each way) */
    sp_opt_log_entry log[SP_OPT_LOG_ENTRIES]; /* the first outer iterations, all levels in order */
} sp_align_result;
int sp_gicp_align_optimize(const sp_gicp_target* target, const sp_gicp_source* source, float* transT_device,
                           const sp_factor_params* params, const sp_opt_params* opt, const float* robust_scales, int n_levels,
                           sp_align_result* result_device, void* workspace, size_t workspace_bytes, void* stream);
/* 0: sp_gicp_align_fused runs every iteration as a launch of its own and sp_gicp_align_optimize reports "not available" — no
 * launch whose workgroups wait for each other is started for this source. Default 1. */
int sp_gicp_source_set_persistent(sp_gicp_source* source, int enable);
/* How sp_gicp_align_optimize's linearisation steps deal the source points: 0 a lane per point; 1 (default) a wave per point for
 * sources of up to 2048 points (more SIMDs than points: the step costs the longest chain of dependent loads, and 64 lanes scanning
 * one query's ball make that chain a handful of round trips); 2 a wave per point for sources of up to 131072 points — for a
 * target whose cells are crowded (sp_grid_max_cell_points in the hundreds or thousands: a raw LiDAR scan), where a lane's walk
 * through its block of cells is thousands of candidates long. Same correspondences in every mode. */
int sp_gicp_source_set_wave_per_point(sp_gicp_source* source, int mode);
/* MI355X extension: the same alignment (registration.hpp:201-276 with pipeline/robust.hpp:78-111 around it, every
 * OptimizationMethod, as sp_gicp_align_optimize runs it) of ONE prepared source against ONE prepared target from `batch` initial
 * guesses in ONE launch — relocalisation, start-up without a pose, a yaw sweep, loop-closure checks. The reference has no such
 * call: it would run align() once per guess, `batch` times the round trips of one alignment. Here workgroup b of a plain grid of
 * `batch` workgroups (256 lanes up to 256 source points, 1024 beyond) runs the whole alignment of hypothesis b: linearise and
 * trial steps over the source, the step's totals summed in LDS, one lane running the optimiser's state machine. A hypothesis
 * keeps its correspondence-cache rows (3 x float4 per point) in the caller's workspace, so the workgroups share nothing they
 * write and none waits for another: the launch needs no residency, works for any batch on any stream (a capturing one too, and
 * beside another stream's persistent launch), ignores sp_gicp_source_set_persistent / sp_gicp_source_set_wave_per_point, and
 * neither reads nor writes the source's own correspondence cache — an alignment of the same source before or after behaves as if
 * the batch had never run. The first linearisation of every hypothesis searches every point; later ones reuse the hypothesis's
 * own rows under the target's certificates.
 *   T_init_device   batch x 16 floats, column-major poses            T_out_device  the final poses (may alias T_init_device)
 *   results_device  batch blocks, each as sp_gicp_align_optimize writes its one (status always 0, pad[0] = SP_ALIGN_RESULT_DONE last)
 *   workspace       sp_gicp_align_batch_workspace_bytes(n, batch) bytes, at least batch * 48 * n; that function returns 0 for
 *                   n == 0, n > SP_ALIGN_BATCH_MAX_POINTS, batch == 0 or batch > SP_ALIGN_BATCH_MAX
 * Only enqueues. Arguments as for sp_gicp_align_optimize (n_levels, method, max_iterations in 1..65535, reg_type as the target
 * was prepared, no rotation constraint); SP_ERR_INVALID_ARGUMENT with a message, and nothing enqueued, also when batch or the
 * source's point count is outside the ranges above, the workspace is too small, or the target has no certificates
 * (sp_gicp_target_create_plain without sp_gicp_target_certify: there are no rows to freeze trials on).
 * sp_align_best_host (host memory only): the block with the most inliers among those with status 0, a finite pose, a finite
 * error and inlier > 0; ties to the smaller error, then to the lower index. *best_out = batch when no block qualifies (SP_OK). */
enum { SP_ALIGN_BATCH_MAX_POINTS = 16384, SP_ALIGN_BATCH_MAX = 65535 };
size_t sp_gicp_align_batch_workspace_bytes(size_t n, size_t batch);
int sp_gicp_align_batch(const sp_gicp_target* target, const sp_gicp_source* source, const float* T_init_device,
                        float* T_out_device, size_t batch, const sp_factor_params* params, const sp_opt_params* opt,
                        const float* robust_scales, int n_levels, sp_align_result* results_device, void* workspace,
                        size_t workspace_bytes, void* stream);
int sp_align_best_host(const sp_align_result* results_host, size_t batch, size_t* best_out);
/* The same optimiser for a HOST-driven loop (registration.hpp:201-276 around optimize_gauss_newton :803-828,
 * optimize_levenberg_marquardt :830-895, optimize_powell_dogleg :897-964, and pipeline/robust.hpp:100-111 for n_levels > 1): the
 * state machine one lane of sp_gicp_align_optimize's launch runs (csrc/sp_optimizer.h), compiled for the host from the same
 * source, fed by a caller that linearises and evaluates trials itself (any factor, pose terms on the host, a device that cannot
 * hold the launch resident). Host memory only: nothing is allocated on a device, no stream is touched.
 *   sp_opt_stepper_create      robust_scales[n_levels] (1 <= n_levels <= SP_OPT_MAX_LEVELS) as for sp_gicp_align_optimize: the
 *                              stepper hands the scale of the level in force back with every request. max_iterations 0: done at
 *                              once, the result is the initial guess (the reference's loop does not run, :227); no upper limit
 *                              (the log's 16-bit iteration field wraps; only the first SP_OPT_LOG_ENTRIES iterations are logged)
 *   sp_opt_stepper_next        what is wanted now: SP_OPT_WANT_LINEARIZE the reduced system at pose T with robust_scale;
 *                              SP_OPT_WANT_TRIAL the frozen-correspondence error and inlier count at the trial pose T over the
 *                              correspondences of the linearisation at T_lin; SP_OPT_WANT_DONE nothing (T: the final pose)
 *   sp_opt_stepper_linearized  the answer to LINEARIZE, after the caller has applied degenerate regularisation and the MAP prior
 *                              to it (registration.hpp:249-253)
 *   sp_opt_stepper_trial       the answer to TRIAL, the MAP prior's error added (:854, :933); rho_out (may be null): the gain
 *                              ratio of a dog-leg trial (:936, what the reference prints under verbose), 0 for LM
 *   sp_opt_stepper_result      the state as sp_gicp_align_optimize reports it (any time; pad[0] = SP_ALIGN_RESULT_DONE once done;
 *                              H, b, error_raw: of the system last handed in; searched 0)
 * An answer of the kind that was not asked for is SP_ERR_INVALID_ARGUMENT and changes nothing. */
enum { SP_OPT_WANT_DONE = 0, SP_OPT_WANT_LINEARIZE = 1, SP_OPT_WANT_TRIAL = 2 };
typedef struct sp_opt_request {
    int want;
    int level, iteration; /* annealing level and its outer iteration */
    float robust_scale;   /* robust_scales[level] */
    float T[16];          /* column-major */
    float T_lin[16];      /* pose of the latest linearisation */
    float damping;        /* lambda (LM) / trust-region radius (dog-leg) in force */
} sp_opt_request;
typedef struct sp_opt_stepper sp_opt_stepper;
int sp_opt_stepper_create(const sp_opt_params* opt, const float* T_init16, const float* robust_scales, int n_levels,
                          sp_opt_stepper** out);
void sp_opt_stepper_destroy(sp_opt_stepper* stepper);
int sp_opt_stepper_next(const sp_opt_stepper* stepper, sp_opt_request* out);
int sp_opt_stepper_linearized(sp_opt_stepper* stepper, const sp_linearized* lin_host);
int sp_opt_stepper_trial(sp_opt_stepper* stepper, float error, uint32_t inlier, float* rho_out);
int sp_opt_stepper_result(const sp_opt_stepper* stepper, sp_align_result* out);
/* Registration::optimize_gauss_newton (registration.hpp:791-828) as ONE device thread, so a whole fixed-length
 * iteration loop can stay on the stream with no host round trip:
 *   delta = LDLT(H + lambda*I).solve(-b);  T <- T * se3_exp(delta);  delta_out[0..5] = delta,
 *   delta_out[6] = 1.0f if converged (|rot| < crit_rot && |trans| < crit_trans) else 0, delta_out[7] = solve ok.
 * lin->inlier_lo/hi (possibly summed over ranks) are folded back into lin->inlier. T_dev is updated in place. */
int sp_gn_update(sp_linearized* lin, float* T_dev, float lambda, float crit_rotation, float crit_translation,
                 float* delta_out8, void* stream);
/* Host twin of the same arithmetic, for a host-driven loop (reads/writes HOST memory, no stream). */
int sp_gn_update_host(const sp_linearized* lin_host, float* T_host, float lambda, float crit_rotation,
                      float crit_translation, float* delta_out8_host);
/* lie::se3_exp (utils/eigen_utils.hpp:909-943) and the Isometry3f product used for T <- T*exp(delta), on the host. */
void sp_se3_exp_host(const float* twist6, float* T_out16);
void sp_rigid_mul_host(const float* A16, const float* B16, float* out16);
int sp_ldlt6_solve_host(const float* H36_rowmajor, const float* rhs6, float* x6);
/* compute_dogleg_step<6> (algorithms/registration/dogleg_step.hpp:35-101), the step geometry of
 * Registration::optimize_powell_dogleg (registration.hpp:897-965); trust-region bookkeeping stays with the caller. */
void sp_dogleg_step_host(const float* H36_rowmajor, const float* g6, float trust_region_radius, float* p_out6,
                         float* step_norm_out, float* predicted_reduction_out);

/* ---- pose-space terms applied to the reduced system on the host, between the device reduction and the solve
 * (Registration::align, registration.hpp:236-253). All matrices here are HOST memory; H row-major as in sp_linearized,
 * poses column-major 4x4. */
/* lie::se3_log (utils/eigen_utils.hpp:991-1034): rotation-first twist of a rigid transform. */
void sp_se3_log_host(const float* T16, float* twist6);
/* DegenerateRegularization::regularize (algorithms/registration/degenerate_regularization.hpp:41-110, NL-Reg): for the
 * rotation and the translation 3x3 block of H, every eigen-direction whose eigenvalue / inlier is below its threshold
 * gets a Tikhonov penalty base_factor * inlier * v v^T; H += P, b += P * se3_log(T_initial^-1 * T_current).
 * Nothing happens for type NONE or inlier == 0. */
enum { SP_DEGENERATE_REG_NONE = 0, SP_DEGENERATE_REG_NL_REG = 1 };
typedef struct sp_degenerate_reg_params { /* DegenerateRegularizationParams, :41-46 */
    int type;
    float rot_eigenvalue_threshold;   /* 10.0 */
    float trans_eigenvalue_threshold; /* 1.0 */
    float base_factor;                /* 1.0 */
} sp_degenerate_reg_params;
int sp_degenerate_regularize_host(const sp_degenerate_reg_params* params, float* H36_rowmajor, float* b6,
                                  uint32_t inlier, const float* T_current16, const float* T_initial16);
/* MapPrior (algorithms/registration/map_prior.hpp:14-213). update (:97-174): from the previous frame's raw Hessian,
 * raw error, inlier count and optimised pose, and the predicted pose of this frame, compute
 * Omega = R - R (Ad^T (H_raw / s^2) Ad + R)^-1 R with R = Q^-1 the motion-adaptive process noise; state->has_prior
 * stays 0 when the prior is disabled or cannot be formed. apply (:181-201): e = se3_log(T_pred^-1 T_est);
 * returns the prior cost e^T Omega e / 2 (0 without a prior) and, when H/b are given, adds Omega, Omega e and the cost
 * to H, b and *error. */
typedef struct sp_map_prior_params { /* MapPriorParams, :14-35 */
    int enabled;
    float rot_vel_sigma;    /* 1.0 */
    float trans_vel_sigma;  /* 1.0 */
    float rot_base_sigma;   /* 3.16e-2 */
    float trans_base_sigma; /* 1e-2 */
} sp_map_prior_params;
typedef struct sp_map_prior_state {
    int has_prior;
    float omega[36];      /* row-major */
    float T_pred_inv[16]; /* column-major */
} sp_map_prior_state;
int sp_map_prior_update_host(const sp_map_prior_params* params, const float* H_raw36_rowmajor, float error_raw,
                             uint32_t inlier, const float* T_prev16, const float* T_pred16, sp_map_prior_state* state);
float sp_map_prior_apply_host(const sp_map_prior_state* state, const float* T_est16, float* H36_rowmajor, float* b6,
                              float* error);

/* ---- host numerics of the per-frame odometry loop (pipeline/lidar_odometry.hpp and what it calls): 3x3 / 4x4 arithmetic the
 * reference writes with Eigen::SelfAdjointEigenSolver<Matrix3f>, AngleAxisf, Quaternionf and FromTwoVectors. HOST memory only,
 * no device is touched. Poses column-major 4x4, rotations column-major 3x3, H row-major as in sp_linearized. */
/* MotionPredictionMode (pipeline/motion_predictor.hpp:17-21) */
enum { SP_MOTION_LIDAR_CV = 0, SP_MOTION_GYRO_LIDAR_CV = 1, SP_MOTION_IMU_SE3 = 2 };
typedef struct sp_motion_axis_params { /* AdaptiveMotionPredictor::Params::AdaptiveAxis, adaptive_motion_predictor.hpp:22-27 */
    float factor_min;          /* 0.2: applied when the block is well constrained */
    float factor_max;          /* 1.0: applied when it is degenerate */
    float min_eigenvalue_low;  /* 1.0 (rotation: 5.0) */
    float min_eigenvalue_high; /* 10.0 */
} sp_motion_axis_params;
typedef struct sp_motion_predict_params { /* MotionPredictor::Params, motion_predictor.hpp:54-56 */
    sp_motion_axis_params rotation, translation;
    float velocity_ema_alpha; /* 1.0 = the raw velocity, 0.0 = frozen */
    int mode;                 /* SP_MOTION_* */
} sp_motion_predict_params;
/* The moving averages of AdaptiveMotionPredictor (:140-141), owned by the caller; zero-initialised = no value yet. */
typedef struct sp_motion_predict_state {
    int has_linear, has_angular;
    float linear[3];  /* m/s, previous LiDAR body frame */
    float angular[3]; /* rotation vector, rad/s */
} sp_motion_predict_state;
/* MotionPredictor::predict (motion_predictor.hpp:60-76) over AdaptiveMotionPredictor::predict (adaptive_motion_predictor.hpp:
 * 54-133). With mode IMU_SE3 and imu_se3_pose16 given, T_pred = that pose and nothing else happens (the averages are not
 * touched). Otherwise: both factors start at factor_max; with registrated != 0 and inlier > 0 each becomes
 * max * (1 - score) + min * score, score = clamp((lambda_min / inlier - low) / max(high - low, 1e-6), 0, 1), lambda_min the
 * smallest eigenvalue of H_raw's rotation (0..2) / translation (3..5) block. The velocities pass through
 * s <- alpha * v + (1 - alpha) * s (the first call stores v); an averaged angular speed that is not > 1e-6 rad/s is no rotation.
 * T_pred: t = t_odom + R_odom (v dt f_t), R = normalized(quat(R_odom) * quat(axis, |w| dt f_r)). With mode GYRO_LIDAR_CV and
 * gyro_delta_rotation9 given, the rotation of odom^-1 * T_pred is replaced by it. H_raw36 may be NULL when registrated == 0;
 * the two candidates may be NULL; factors2_out (rotation, translation) may be NULL. */
int sp_motion_predict_host(const sp_motion_predict_params* params, sp_motion_predict_state* state,
                           const float* linear_velocity3, const float* angular_velocity_rotvec3, const float* odom16, float dt,
                           const float* H_raw36_rowmajor, uint32_t inlier, int registrated, const float* gyro_delta_rotation9,
                           const float* imu_se3_pose16, float* T_pred16_out, float* factors2_out);
/* lidar_odometry.hpp:282-286: delta = prev^-1 * cur; linear3 = delta.t / dt; angle_axis4 = (AngleAxisf(delta.R).angle / dt,
 * axis xyz) - angle >= 0; the identity gives angle 0 about x. */
int sp_velocity_from_poses_host(const float* T_prev16, const float* T_cur16, float dt, float* linear3_out, float* angle_axis4_out);
/* Submap::is_keyframe (pipeline/submapping.hpp:144-161): *is_keyframe_out = distance >= distance_threshold || angle (degrees,
 * of AngleAxisf) >= angle_threshold_degrees || delta_time >= time_threshold_seconds, where delta_time is DBL_MAX unless
 * last_keyframe_time > 0.0. metrics3_out (may be NULL): distance, angle in degrees, delta_time. */
int sp_keyframe_decision_host(const float* T_last_keyframe16, const float* T_current16, double last_keyframe_time,
                              double timestamp, float distance_threshold, float angle_threshold_degrees,
                              float time_threshold_seconds, int* is_keyframe_out, double* metrics3_out);
typedef struct sp_initial_alignment_params { /* imu::InitialAlignmentParams, imu_initial_alignment.hpp:18-46 (what estimate reads) */
    float required_duration_sec; /* 1.0 */
    float max_gyro_std;          /* 0.01 rad/s */
    float max_accel_std;         /* 0.2 m/s^2 */
    float max_accel_norm_error;  /* 0.5 m/s^2 */
    int estimate_gyro_bias;      /* 1 */
} sp_initial_alignment_params;
typedef struct sp_initial_alignment_result { /* imu::InitialAlignmentResult, :54-65 */
    int success;
    int window_size;      /* samples the statistics were taken over (0 on the returns before the window is chosen) */
    float R_world_imu[9]; /* column-major */
    float gyro_bias[3], accel_mean[3], gyro_std[3], accel_std[3];
    float accel_norm, roll_rad, pitch_rad;
    char error_message[96]; /* the reference's text of the early return taken; empty on success */
} sp_initial_alignment_result;
/* imu::estimate_initial_alignment (imu_initial_alignment.hpp:85-204). stamps: n absolute seconds in buffer order; gyro_accel: n
 * rows of gyro xyz, accel xyz; bias6 = (gyro_bias, accel_bias). The window is every sample with stamp >= last - required, plus
 * the latest earlier one when the first of them lies more than 1e-6 s inside; means and variances in double; the three
 * stationarity tests unless bypass_stationarity != 0; R_world_imu the minimum rotation taking the bias-corrected mean specific
 * force onto -gravity (Quaternionf::FromTwoVectors; for opposite vectors the reference takes an axis from an SVD, here the cross
 * product with the coordinate axis least aligned with the force), roll = atan2(R21, R22), pitch = asin(-clamp(R20)). An early
 * return of the reference is SP_OK with success = 0 and its message. Null pointers (stamps / gyro_accel with n > 0, gravity3,
 * params, bias6, result_out) -> SP_ERR_INVALID_ARGUMENT. */
int sp_initial_alignment_host(const double* stamps_host, const float* gyro_accel_host, size_t n, const float* gravity3,
                              const sp_initial_alignment_params* params, const float* bias6, int bypass_stationarity,
                              sp_initial_alignment_result* result_out);
/* imu::detail::yaw_from_rotation (:211-218): atan2(R10, R00), 0 when R00^2 + R10^2 < 1e-12. */
float sp_yaw_from_rotation_host(const float* R9_colmajor);

/* ---- tightly coupled LiDAR-inertial alignment in 15 DoF (algorithms/imu/imu_factor.hpp = A, algorithms/lio/lio_registration.hpp
 * = B, algorithms/registration/dogleg_step.hpp). HOST memory only, no device is touched, no stream. The per-point work of LIO is
 * sp_gicp_linearize / sp_gicp_error; these are the 15x15 algebra and the control flow around them.
 * Every 15x15 matrix is COLUMN-major (as sp_imu_preint_reset takes its covariance); the 6x6 of sp_linearized stays row-major.
 * A state is 21 floats: position 3, rotation 9 (column-major), velocity 3, accelerometer bias 3, gyroscope bias 3. The
 * error-state order is [dp, dphi, dv, db_a, db_g] (indices 0, 3, 6, 9, 12; imu::State::kIdx*). LDL^T is Eigen's (diagonal pivoting,
 * left-looking, failure on a zero pivot under a non-zero column; "positive" = vectorD().minCoeff() > 0), the algorithm of
 * sp_ldlt6_solve_host for any size. A null argument not named optional -> SP_ERR_INVALID_ARGUMENT. */
/* compute_manifold_residual (A:71-85): r = x_op (-) x_pred, the rotation part so3_log(quat(R_pred^T R_op)). */
int sp_imu_manifold_residual_host(const float* x_pred21, const float* x_op21, float* r15_out);
/* compute_imu_hessian_gradient (A:116-141): H = P^-1, b = P^-1 r through one LDL^T of P. *valid_out = 0 with H = 0 and b = 0 when
 * the factorisation fails or its smallest D is <= 0. */
int sp_imu_hessian_gradient_host(const float* x_pred21, const float* x_op21, const float* P225, float* H225_out, float* b15_out,
                                 int* valid_out);
/* compute_imu_gradient (A:154-157): b = H r. */
int sp_imu_gradient_host(const float* x_pred21, const float* x_op21, const float* H225, float* b15_out);
typedef struct sp_lio_linearized { /* LIOLinearizedResult (lio_linearized_result.hpp) */
    float H[225]; /* column-major */
    float b[15];
    float error_icp, error_imu;
    uint32_t inlier;
    uint32_t pad;
} sp_lio_linearized; /* 976 bytes */
/* add_icp_factor (B:94-113): the ICP system ([d_omega, d_t], body frame) is added into the rotation / position blocks, the
 * translation blocks rotated into the world frame with R_world_lidar; error_icp += weight * error, inlier += inlier. */
int sp_lio_add_icp_factor_host(sp_lio_linearized* result, const sp_linearized* icp, const float* R_world_lidar9, float weight);
typedef struct sp_lio_directional_params { /* DirectionalIcpWeightingParams (lio_registration_params.hpp:28-38) */
    int enable;                            /* 1 */
    float trans_min_eigenvalue_per_inlier; /* 10 */
    float rot_min_eigenvalue_per_inlier;   /* 10 */
    float trans_weak_direction_scale;      /* 0.2 */
    float rot_weak_direction_scale;        /* 0.2 */
} sp_lio_directional_params;
/* apply_directional_icp_weighting (B:144-202) on a factor that holds the ICP contribution only: nothing when disabled or
 * inlier == 0; the pose blocks symmetrised; per 3x3 diagonal block a filter sum_i sqrt(clamp(scale_i)) q_i q_i^T with scale_i = 0
 * for an eigenvalue <= 0, else max(weak_scale, lambda_i / (min_per_inlier * inlier)) when that threshold is > 0, else 1; the pose
 * system becomes F H F and F F b. */
int sp_lio_directional_weighting_host(sp_lio_linearized* icp_factor, const sp_lio_directional_params* params);
/* solve_ldlt (B:224-238): H delta = -b; P_post225_opt (may be NULL) = H^-1. *ok_out = 0 with delta = 0 (and P_post = 0) when the
 * factorisation fails or is not positive. */
int sp_lio_solve_ldlt_host(const float* H225, const float* b15, float* delta15_out, float* P_post225_opt, int* ok_out);
/* retract (B:260-273): p + dp, R * quat_to_rot(so3_exp(dphi)), v + dv, b_a + db_a, b_g + db_g. */
int sp_lio_retract_host(const float* x21, const float* delta15, float* x_out21);
/* imu_to_lidar_jacobian (B:308-323): identity but J[phi, phi] = R_lidar_imu and J[p, phi] = -R_world_lidar R_lidar_imu
 * skew(t_lidar_in_imu), T_imu_to_lidar column-major 4x4. */
int sp_lio_imu_to_lidar_jacobian_host(const float* T_imu_to_lidar16, const float* R_world_lidar9, float* J225_out);
/* transform_covariance_imu_to_lidar (lidar_to_imu == 0: J P J^T) and transform_covariance_lidar_to_imu (lidar_to_imu != 0:
 * J^-1 P J^-T with the analytic inverse) (B:340-381). P_out225 must not be P225. */
int sp_lio_transform_covariance_host(const float* P225, const float* T_imu_to_lidar16, const float* R_world_lidar9, int lidar_to_imu,
                                     float* P_out225);
/* compute_dogleg_step<N> (dogleg_step.hpp:33-102) for n = 6 or 15 (any other n -> SP_ERR_INVALID_ARGUMENT): H n x n column-major
 * (it is symmetric), g[n]. For n = 6 the arithmetic is that of sp_dogleg_step_host, whose signature stays as it is. */
int sp_dogleg_step_n_host(int n, const float* H, const float* g, float trust_region_radius, float* p_out, float* step_norm_out,
                          float* predicted_reduction_out);
typedef struct sp_lio_params { /* LIORegistrationParams (lio_registration_params.hpp:41-49) */
    sp_opt_params opt; /* optimization + criteria; max_iterations = total_iterations, summed over all robust levels */
    int robust_auto_scale; /* LIORobustScheduleParams: 0 */
    float robust_init_scale, robust_min_scale;                   /* 10, 0.5 */
    float rotation_robust_init_scale, rotation_robust_min_scale; /* 10, 0.5 */
    int robust_auto_scaling_iter;                                /* 4 */
    float invalid_regularization_factor;                         /* 1e4 */
    sp_lio_directional_params directional;
} sp_lio_params;
typedef struct sp_lio_factor_facts { /* what the loop reads of RegistrationFactorParams */
    int residual_dim;    /* 1 for POINT_TO_PLANE / GENZ, 3 otherwise (B:412-415) */
    int robust_is_none;  /* robust.type == NONE: no auto scaling (B:444-445) */
    float robust_default_scale, rotation_robust_default_scale; /* the scales of the single level without auto scaling */
} sp_lio_factor_facts;
typedef struct sp_lio_request {
    int want;             /* SP_OPT_WANT_* */
    int level, iteration; /* robust level and its solver iteration */
    float robust_scale, rotation_robust_scale; /* of the level in force */
    float state[21];      /* LINEARIZE: the operating state; TRIAL: the state to evaluate; DONE: the final state */
    float T[16];          /* its pose, column-major */
    float T_lin[16];      /* pose of the latest linearisation */
    float damping;        /* lambda (GN, LM) / trust-region radius (dog-leg) in force */
    float icp_weight;     /* the chi-square weight of the latest linearisation (1 before the first) */
} sp_lio_request;
typedef struct sp_lio_result { /* LIORegistrationResult */
    float state[21];
    float posterior_covariance[225];
    uint32_t iterations; /* every outer iteration, rejected ones too */
    uint32_t inlier;     /* of the last ICP linearisation, unweighted */
    float error;
    uint32_t converged;  /* always 1 (B:643) */
} sp_lio_result;
/* LIORegistration::align (B:396-648) as a state machine in the shape of sp_opt_stepper_*: the caller linearises
 * (Registration::compute_linearized_result at T with initial_pose = the predicted pose and the request's two scales) and
 * evaluates trials (compute_error_frozen at T) and the stepper does everything else: the IMU prior from ONE factorisation at
 * (x_pred, x_pred), from the second iteration on its gradient only; icp_weight = 1 / max(1, 2 error / (dim inlier - 6));
 * directional weighting of the ICP-only factor; invalid_regularization_factor * I on velocity and biases when the prior is
 * invalid; GN (a failed solve ends the level), LM (a TRIAL at the operating state first, then up to max_inner trials; none
 * accepted ends the level), dog-leg (a TRIAL at the operating state first; step on the undamped H, the bias freeze before the
 * predicted reduction; predicted <= 0 or rho < eta1 shrinks the radius, counts the iteration and linearises again at the same
 * state); update_bias == 0 zeroes both bias segments of every candidate; convergence leaves the current level only; the robust
 * schedule of B:443-476 with its three messages on stderr; the posterior of B:663-685. total_iterations 0: done at once, state =
 * predicted, posterior = previous, iterations 0, inlier 0, error FLT_MAX. An answer of the kind that was not asked for is
 * SP_ERR_INVALID_ARGUMENT and changes nothing. */
typedef struct sp_lio_stepper sp_lio_stepper;
int sp_lio_stepper_create(const sp_lio_params* params, const sp_lio_factor_facts* facts, const float* predicted_state21,
                          const float* predicted_covariance225, const float* previous_posterior_covariance225, int update_bias,
                          sp_lio_stepper** out);
void sp_lio_stepper_destroy(sp_lio_stepper* stepper);
int sp_lio_stepper_next(const sp_lio_stepper* stepper, sp_lio_request* out);
int sp_lio_stepper_linearized(sp_lio_stepper* stepper, const sp_linearized* lin_host);
int sp_lio_stepper_trial(sp_lio_stepper* stepper, float error, uint32_t inlier);
int sp_lio_stepper_result(const sp_lio_stepper* stepper, sp_lio_result* out);

/* ---- the per-frame LiDAR-inertial odometry loop (pipeline/lidar_inertial_odometry.hpp = L): what LidarInertialOdometryPipeline
 * computes and decides between its stages. HOST memory only, no device is touched, no stream; the conventions above. */
/* imu_bias_observable (L:371-393) on the n samples of the IMU window, gyro and accel as n x 3. *observable_out = 1 when
 * freeze_on_low_excitation == 0 (nothing is read); else 0 for n < 2; else 1 when max_i |gyro_i - mean gyro| > the gyro threshold
 * or max_i |accel_i - mean accel| > the accel threshold (the norms of the full difference vectors, strict >), 0 otherwise. The
 * means are float32 sums in sample order divided by (float)n. */
int sp_lio_bias_observable_host(const float* gyro_host, const float* accel_host, size_t n, int freeze_on_low_excitation,
                                float gyro_excitation_threshold, float accel_excitation_threshold, int* observable_out);
/* clamp_bias_norm (L:396-400), in place: nothing for max_norm <= 0 or |bias| <= max_norm, else bias *= max_norm / |bias|. */
int sp_lio_clamp_bias_host(float* bias3, float max_norm);
/* predict_state (L:432-459) from what the integrator reports for the current bias: T_imu_rel16 = predict_relative_transform,
 * Delta_v3 and dt_total = get_corrected. T_pred = pose(x) * (T_imu_to_lidar * T_imu_rel * T_imu_to_lidar^-1) gives position and
 * rotation; velocity = v + gravity * dt_total + (R * R_imu_to_lidar) * Delta_v; both biases are copied. */
int sp_lio_predict_state_host(const float* x21, const float* T_imu_to_lidar16, const float* T_imu_rel16, const float* Delta_v3,
                              float dt_total, const float* gravity3, float* x_pred_out21);
/* the covariance and rotation reset_imu_preintegration (L:402-426) hands to the integrator: P_post + fd_velocity_sigma^2 I on the
 * velocity block + icp_rotation_sigma^2 I on the rotation block, then sp_lio_transform_covariance_host(..., lidar_to_imu = 1)
 * (the same code); R_world_imu = R_world_lidar * R_imu_to_lidar, column-major. P_initial_imu225_out must not be P_post225. */
int sp_lio_reset_covariance_host(const float* P_post225, float fd_velocity_sigma, float icp_rotation_sigma,
                                 const float* T_imu_to_lidar16, const float* R_world_lidar9, float* P_initial_imu225_out,
                                 float* R_world_imu9_out);

/* ----------------------------------------------------------------------------------------- multi-GPU */

/* One process per GPU; the source cloud is sharded over the ranks, the target (points, covariances, grid, prepared rows)
 * is replicated. The exchange is RCCL over xGMI, bound at run time (dlopen librccl.so.1): on a machine
 * without RCCL these entry points return SP_ERR_RUNTIME and everything else still works.
 *   sp_comm_unique_id   ncclGetUniqueId: SP_COMM_ID_BYTES bytes, made by ONE rank and handed to the others out of band
 *                       (MPI_Bcast, a torch.distributed broadcast, a file)
 *   sp_comm_create      ncclCommInitRank on the calling thread's current device; collective over the `world` callers
 *   sp_allreduce_rows   sum over the ranks, in place, of launch k's fan-in row (sp_gicp_align_row): 128 bytes
 *   sp_allreduce_f32    the same for any float buffer (e.g. the 192-byte system of the generic loop, 2 scalars of an LM step)
 *   sp_allgather        ncclAllGather of bytes_per_rank bytes per rank (target covariances of a pre-loop sharded by query)
 *   sp_gicp_align_sharded  sp_gicp_align_fused with the source sharded over `comm`: per iteration one launch
 *                       (sp_gicp_align_step, rows_all_reduced = 2) + one sp_allreduce_rows, then sp_gicp_align_finish; every
 *                       rank ends with the identical pose. Only enqueues (hipGraph-capturable). All ranks must pass the same
 *                       params, gn and max_iterations; a rank with an empty shard still calls it.
 * An error return on one rank (bad arguments, a HIP error) leaves the other ranks inside that iteration's collective: the
 * communicator cannot be used again — destroy it (sp_comm_destroy) on every rank and create a new one. Launches after
 * convergence contribute a zero row. */
#define SP_COMM_ID_BYTES 128
typedef struct sp_comm sp_comm;
int sp_comm_unique_id(void* id_out);
int sp_comm_create(const void* id, int rank, int world, sp_comm** out);
void sp_comm_destroy(sp_comm* comm);
int sp_comm_rank(const sp_comm* comm);
int sp_comm_world(const sp_comm* comm);
int sp_allreduce_rows(sp_comm* comm, void* workspace, int k, void* stream);
int sp_allreduce_f32(sp_comm* comm, float* buf, size_t n_floats, void* stream);
int sp_allgather(sp_comm* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int sp_gicp_align_sharded(const sp_gicp_target* target, const sp_gicp_source* source, float* transT_device,
                          const sp_factor_params* params, const sp_gn_params* gn, int max_iterations, sp_comm* comm,
                          int32_t* nn_idx_out, float* nn_d2_out, sp_linearized* lin_out, float* delta_out8,
                          uint32_t* iterations_out, void* workspace, size_t workspace_bytes, void* stream);

/* The same sharded loop WITHOUT a collective per iteration (direct exchange). An all-reduce of 128 bytes is pure latency — a
 * library launch between two kernels, 15-30 us on an 8-GPU node against ~30 us of compute per iteration. Here every rank owns
 * a small slot buffer in uncached device memory and maps its peers' (hipIpc handles, exchanged ONCE through the caller's own
 * channel); the streaming launch's last-arriving workgroup stores the rank's 128-byte row, tagged with the iteration's
 * sequence number, straight into every rank's buffer over xGMI, and the NEXT streaming launch's prologue (every workgroup
 * for itself) waits until all `world` rows carry the tag, adds them in rank order (identical sums, identical pose on every
 * rank) and solves: one launch per iteration, nothing in between.
 *   sp_xchg_create / sp_xchg_handle / sp_xchg_connect   every rank creates, all ranks gather the SP_XCHG_HANDLE_BYTES-byte
 *                       handles in rank order (MPI_Allgather, torch.distributed, a file ...) and connect; world <= 8
 *   sp_gicp_align_direct   arguments as sp_gicp_align_sharded; only enqueues; every rank must call it the same number of
 *                       times (the sequence numbers are counted per alignment); max_iterations <= 255
 *   sp_gicp_align_status   the wait is BOUNDED (sp_xchg_set_timeout_ms, default 2000): a row that does not arrive stops the
 *                       alignment and raises a flag in its state block instead of hanging the queue; this call reads the
 *                       flag back (it synchronises the stream) -> SP_OK, or SP_ERR_RUNTIME when a peer was missing.
 * Summation order differs from one GPU (per-rank sums first), so poses agree to rounding, as with sp_gicp_align_sharded. */
#define SP_XCHG_HANDLE_BYTES 64
typedef struct sp_xchg sp_xchg;
int sp_xchg_create(int rank, int world, sp_xchg** out);
int sp_xchg_handle(const sp_xchg* xchg, void* handle_out);
int sp_xchg_connect(sp_xchg* xchg, const void* handles_of_all_ranks);
int sp_xchg_set_timeout_ms(sp_xchg* xchg, unsigned milliseconds);
int sp_xchg_rank(const sp_xchg* xchg);
int sp_xchg_world(const sp_xchg* xchg);
void sp_xchg_destroy(sp_xchg* xchg);
int sp_gicp_align_direct(const sp_gicp_target* target, const sp_gicp_source* source, float* transT_device,
                         const sp_factor_params* params, const sp_gn_params* gn, int max_iterations, sp_xchg* xchg,
                         int32_t* nn_idx_out, float* nn_d2_out, sp_linearized* lin_out, float* delta_out8,
                         uint32_t* iterations_out, void* workspace, size_t workspace_bytes, void* stream);
int sp_gicp_align_status(const void* workspace, int last_k, void* stream);

/* ------------------------------------------------------------------------------------- voxel hash map */

/* VoxelHashMap (algorithms/mapping/voxel_hash_map.hpp:22-1072): submap accumulation keyed by compute_voxel_bit
 * (sp_voxel_keys' key). The table (double hashing, 100 probes, capacities from the reference's prime list, rehash when
 * voxel_num / capacity exceeds the threshold) lives in HBM and is owned by the object; per voxel it keeps the sums of the
 * map-frame points, of log(R C R^T) (log-Euclidean covariance mean), of rgb and of intensity, a count and the time stamp of
 * its last update.
 *   sp_vhm_create        constructor (:28-36); voxel_size <= 0 -> SP_ERR_INVALID_ARGUMENT (std::invalid_argument, :41-43)
 *   sp_vhm_set / _get    set_voxel_size / set_max_staleness / set_remove_old_data_cycle / set_rehash_threshold /
 *                        set_min_num_point and their getters (:38-80)
 *   sp_vhm_clear         clear (:83-113)
 *   sp_vhm_add_point_cloud  add_point_cloud (:117-141): [rehash] -> integrate the cloud (device points in the SENSOR frame,
 *                        optional covariances / rgb / intensities; sensor_pose_host16 = column-major 4x4 in the map frame)
 *                        -> [remove_old_data every remove_old_data_cycle calls] -> ++staleness counter. Accumulation uses
 *                        relaxed device-scope atomics, as the reference does: counts are exact, float sums agree to rounding.
 *   sp_vhm_downsampling  downsampling (:146-190): voxels with count >= min_num_point whose centroid lies in the axis-aligned
 *                        box center +- distance -> mean point (w = 1), exp of the mean log-covariance, mean rgb / intensity,
 *                        in table-slot order (deterministic for a given table; the reference's order is that of an atomic
 *                        counter). Attribute outputs are written only when the map holds that attribute (sp_vhm_info); out
 *                        arrays must hold sp_vhm_info(SP_VHM_INFO_VOXEL_NUM) entries. keys_out_opt: the voxel keys.
 *   sp_vhm_overlap_ratio compute_overlap_ratio (:196-246)
 *   sp_vhm_remove_old_data remove_old_data (:248, 788-843)
 * Like the reference's methods these calls wait for their kernels (voxel counts are read back by the host). */
typedef struct sp_voxel_hash_map sp_voxel_hash_map;
enum { SP_VHM_VOXEL_SIZE = 0, SP_VHM_MAX_STALENESS = 1, SP_VHM_REMOVE_OLD_DATA_CYCLE = 2, SP_VHM_REHASH_THRESHOLD = 3,
       SP_VHM_MIN_NUM_POINT = 4 };
enum { SP_VHM_INFO_VOXEL_NUM = 0, SP_VHM_INFO_CAPACITY = 1, SP_VHM_INFO_STALENESS_COUNTER = 2, SP_VHM_INFO_HAS_COV = 3,
       SP_VHM_INFO_HAS_RGB = 4, SP_VHM_INFO_HAS_INTENSITY = 5 };
int sp_vhm_create(float voxel_size, void* stream, sp_voxel_hash_map** out);
void sp_vhm_destroy(sp_voxel_hash_map* map);
int sp_vhm_set(sp_voxel_hash_map* map, int param, float value);
float sp_vhm_get(const sp_voxel_hash_map* map, int param);
size_t sp_vhm_info(const sp_voxel_hash_map* map, int what);
int sp_vhm_clear(sp_voxel_hash_map* map, void* stream);
int sp_vhm_add_point_cloud(sp_voxel_hash_map* map, const float* points, const float* covs, const float* rgb,
                           const float* intensities, size_t n, const float* sensor_pose_host16, void* stream);
int sp_vhm_downsampling(sp_voxel_hash_map* map, const float* center_host3, float distance, float* points_out,
                        float* covs_out, float* rgb_out, float* intensities_out, uint64_t* keys_out_opt,
                        size_t out_capacity, size_t* n_out_host, void* stream);
int sp_vhm_overlap_ratio(const sp_voxel_hash_map* map, const float* points, size_t n, const float* sensor_pose_host16,
                         float* ratio_out_host, void* stream);
int sp_vhm_remove_old_data(sp_voxel_hash_map* map, void* stream);

/* Voxelised GICP: a scan aligned against the map itself (MI355X extension; the reference exports the voxel means, builds a
 * KD-tree on them, estimates covariances and searches a neighbour per point per iteration, submapping.hpp). The target of a
 * source point is the Gaussian of a voxel (its mean, the exp of its mean log-covariance); the correspondence is a hash lookup.
 *   sp_vhm_prepare_registration  three float4 per table slot, indexed as the table's keys are, in an array the map owns
 *                        (allocated at the first call, again after a grow): row 0 = mean xyz, w = 1 when the voxel counts
 *                        (count >= min_num_point, count != 0) else 0; rows 1-2 = (xx, xy, xz, yy | yz, zz, 0, 0) of
 *                        SP_REG_GICP: V diag(1e-3, 1, 1) V^T of the voxel covariance; SP_REG_POINT_TO_DISTRIBUTION: its inverse
 *                        (zero when |det| < 1e-6). One launch, one lane per slot; enqueue only. The rows are valid for the map's
 *                        GENERATION, a counter that add_point_cloud, a rehash, remove_old_data, clear and setting voxel_size or
 *                        min_num_point advance. Any other reg_type, or a map without covariances: SP_ERR_INVALID_ARGUMENT,
 *                        nothing enqueued.
 *   sp_vhm_registration_ready    1 when the rows are those of the map's current generation and of reg_type, else 0.
 *   sp_vhm_registration_workspace_bytes / sp_vhm_prepare_source  the workspace of an alignment of n source points: partial rows
 *                        of the reduction | the frozen slot of every point (uint32, 0xFFFFFFFF: none) | two float4 per point,
 *                        the packed V diag(1e-3, 1, 1) V^T of its covariance, which prepare_source fills once per alignment
 *                        (SP_REG_POINT_TO_DISTRIBUTION reads no source covariance: nothing is enqueued, src_covs may be null).
 *   sp_vhm_neighbor_offsets_host  the cells a source point probes, in order, as neighbor_voxels int32 triples (dx, dy, dz):
 *                        1 = its own cell; 7 = that, then the six face neighbours; 27 = those seven, then the twelve edge and the
 *                        eight corner neighbours. HOST only. Any other count: SP_ERR_INVALID_ARGUMENT.
 *   sp_vhm_linearize     per source point q = T p -> the key of every probed cell (an invalid key is skipped) -> its slot (100
 *                        probes) -> among the slots whose row has w = 1 the one whose mean is nearest to q, an exact tie to the
 *                        earlier cell of the probing order -> rejected when |q - mean|^2 > max_correspondence_distance^2 -> else
 *                        linearised against the voxel's row (sp_gicp_iteration_fused's algebra) and summed into *out by the fixed
 *                        tree of sp_gicp_linearize: two runs give the same bits. The winner's slot is kept in the workspace (the
 *                        frozen correspondence); corr_keys_out_opt (device, n entries) receives its voxel key, or ~0.
 *   sp_vhm_error         the error of the factor at transT_trial over the slots the last sp_vhm_linearize of this map left in
 *                        this workspace (out->error, out->inlier; the inlier gate is that linearisation's, M uses the trial
 *                        pose's R): what an LM / dog-leg trial step asks for. SP_ERR_RUNTIME when that workspace holds no
 *                        linearisation of this map and n; SP_ERR_INVALID_ARGUMENT when the map's generation has moved since.
 * linearize and error only enqueue; both need sp_vhm_registration_ready(map, params->reg_type) (SP_ERR_INVALID_ARGUMENT
 * otherwise, as for an enabled rotation constraint, a reg_type other than the two above and a workspace that is too small), and
 * write nothing when they fail. n == 0: *out zeroed, SP_OK. All array pointers are device memory; transT as for sp_gicp_linearize. */
int sp_vhm_prepare_registration(sp_voxel_hash_map* map, int reg_type, void* stream);
int sp_vhm_registration_ready(const sp_voxel_hash_map* map, int reg_type);
size_t sp_vhm_registration_workspace_bytes(size_t n);
int sp_vhm_prepare_source(const float* src_covs, size_t n, int reg_type, void* workspace, size_t workspace_bytes, void* stream);
int sp_vhm_neighbor_offsets_host(int neighbor_voxels, int32_t* out);
int sp_vhm_linearize(const sp_voxel_hash_map* map, const float* src_points, size_t n, const float* transT,
                     int transT_on_device, const sp_factor_params* params, int neighbor_voxels, sp_linearized* out,
                     uint64_t* corr_keys_out_opt, void* workspace, size_t workspace_bytes, void* stream);
int sp_vhm_error(const sp_voxel_hash_map* map, const float* src_points, size_t n, const float* transT_trial,
                 int trial_on_device, const sp_factor_params* params, sp_linearized* out, void* workspace,
                 size_t workspace_bytes, void* stream);
/* The same alignment from `batch` initial guesses in ONE launch (relocalisation against the map: start-up without a pose, a yaw
 * sweep, a loop-closure check): sp_gicp_align_batch's launch shape around sp_vhm_linearize's and sp_vhm_error's per-point work.
 * Workgroup b of a plain grid of `batch` workgroups runs the whole alignment of hypothesis b (every OptimizationMethod, n_levels
 * robust scales): a step is a pass of its lanes over the source, the totals are summed in LDS, one lane runs the optimiser's
 * state machine. 256 lanes up to 256 source points, 512 beyond (no form of the kernel uses scratch memory). The workgroups
 * share nothing they write and none waits for another: no residency requirement, any batch on any stream (a capturing one too,
 * and beside another stream's persistent launch). The map is only read: its generation, its rows and what sp_vhm_linearize noted
 * for sp_vhm_error stay as they are — an sp_vhm_error after a batch behaves as if the batch had not run.
 *   src_covs        n x 16 floats; may be null for SP_REG_POINT_TO_DISTRIBUTION. SP_REG_GICP: the packed source rows are filled
 *                   on the same stream ahead of the optimiser (two launches; point-to-distribution one)
 *   T_init_device   batch x 16 floats, column-major poses            T_out_device  the final poses (may alias T_init_device)
 *   results_device  batch blocks, each as sp_gicp_align_batch writes its one (status 0, pad[0] = SP_ALIGN_RESULT_DONE last).
 *                   searched = n x linearizations: every linearisation looks every point up. T_lin: the pose of the last
 *                   linearisation, whose system H, b, error_raw are
 *   corr_keys_out_opt  device, batch x n, may be null: each point's voxel key of that last linearisation, or ~0
 *   workspace       sp_vhm_align_batch_workspace_bytes(n, batch) bytes: two float4 per source point | batch arrays of n uint32
 *                   slots, each 16-byte aligned; at least 32 n + 4 n batch. That function returns 0 for n == 0,
 *                   n > SP_VHM_ALIGN_BATCH_MAX_POINTS, batch == 0 or batch > SP_ALIGN_BATCH_MAX
 * Only enqueues. SP_ERR_INVALID_ARGUMENT with a message for a null argument, n_levels outside 1..SP_OPT_MAX_LEVELS, an unknown
 * method, max_iterations outside 1..65535, a reg_type other than the two above, an enabled rotation constraint, a map without
 * covariances, rows that are not sp_vhm_registration_ready for params->reg_type, neighbor_voxels not 1 / 7 / 27, n or batch
 * outside the ranges above and a workspace that is too small; SP_ERR_RUNTIME with the reference's message for SP_REG_GICP
 * without src_covs. On any failure nothing is enqueued and nothing is written. */
enum { SP_VHM_ALIGN_BATCH_MAX_POINTS = 16384 };   /* batch limit: SP_ALIGN_BATCH_MAX */
size_t sp_vhm_align_batch_workspace_bytes(size_t n, size_t batch);
int sp_vhm_align_batch(const sp_voxel_hash_map* map, const float* src_points, const float* src_covs, size_t n,
                       const float* T_init_device, float* T_out_device, size_t batch,
                       const sp_factor_params* params, const sp_opt_params* opt,
                       const float* robust_scales, int n_levels, int neighbor_voxels,
                       sp_align_result* results_device, uint64_t* corr_keys_out_opt,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- OccupancyGridMap (mapping/occupancy_grid_map.hpp:27-472)
 * The other submap of Submap::build_submap: the VoxelHashMap table (same key, same double hashing, same capacity ladder; 128
 * probes; removed slots keep a `deleted` key) whose voxels also carry a log-odds occupancy. Per voxel: sums of the map-frame hit
 * points, of log(R C R^T), of rgb and of intensity, hit_count, miss_count, log_odds, the frame of the last update.
 *   sp_ogm_create        constructor; voxel_size <= 0 -> SP_ERR_INVALID_ARGUMENT (std::invalid_argument, :73-76)
 *   sp_ogm_set / _get    the setters (:73-124) and rehash_threshold_; defaults :1658-1680. SP_OGM_LOG_ODDS_MIN above the maximum,
 *                        SP_OGM_LOG_ODDS_MAX below the minimum and an occupancy threshold outside (0, 1) are SP_ERR_INVALID_ARGUMENT.
 *                        SP_OGM_OCCUPANCY_THRESHOLD is given and returned as a probability and kept as log-odds.
 *   sp_ogm_set_log_odds_limits  set_log_odds_limits(minimum, maximum) in one call (:107-113)
 *   sp_ogm_add_point_cloud  add_point_cloud (:129-163): n == 0 returns at once; else [rehash] -> hits (centroid sums, hit_count,
 *                        covariance in the log-Euclidean encoding, rgb, intensity) -> [free-space carving: one miss for every
 *                        cell a ray crosses between the sensor's cell and the hit cell, the hit cell excluded, after growing the
 *                        table for the estimated number of visits] -> log_odds += hits * log_odds_hit + misses * log_odds_miss,
 *                        clamped -> [prune voxels not updated for more than stale_frame_threshold frames] -> ++frame.
 *                        The ray walk takes exactly |dix| + |diy| + |diz| steps; rays with a non-finite end point, an end point
 *                        outside the 21-bit cell range, or shorter than sqrt(FLT_EPSILON) post nothing, and nothing is carved
 *                        from a sensor position outside that range.
 *   sp_ogm_extract_occupied_points  extract_occupied_points (:169-181, 1530-1639): voxels with hit_count > 0, log_odds >= the
 *                        threshold and a centroid within max_distance (L-infinity) of sensor_xyz -> mean point (w = 1), exp of
 *                        the mean log-covariance, mean rgb / intensity, in table-slot order. Attribute outputs are written only
 *                        when the map holds that attribute; out arrays must hold sp_ogm_info(SP_OGM_INFO_VOXEL_NUM) entries.
 *   sp_ogm_extract_visible_points  extract_visible_points (:183-411): the occupied voxels whose centroid lies within max_distance
 *                        (L2) of the sensor and inside the frustum of horizontal_fov x vertical_fov around the sensor's x axis
 *                        (:197-198 clamps them to [1e-6, pi - 1e-6] and [1e-6, 2 pi - 1e-6]; at the horizontal limit the frustum
 *                        is mirrored behind the sensor, :248, 284), and that no other occupied voxel hides: the ray walk of the
 *                        carving runs from the sensor to the centroid and stops at the first occupied cell whose centroid is
 *                        nearer by more than 1e-6 in the squared distance (:313-361); a voxel within voxel_size of the sensor is
 *                        never hidden. Rows as for sp_ogm_extract_occupied_points, in table-slot order. Reads the map only. The
 *                        cosines of the frustum test are forward / sqrt(norm_sq), correctly rounded (the reference uses rsqrt); a
 *                        sensor at a non-finite position or outside the 21-bit cell range gives 0 rows; NaN max_distance (+inf is
 *                        allowed), a non-finite field of view or other pose entry is SP_ERR_INVALID_ARGUMENT.
 *   sp_ogm_overlap_ratio compute_overlap_ratio (:417-472)
 *   sp_ogm_voxel_probability  voxel_probability (:85-93): 0.5 where the map has no voxel
 *   sp_ogm_export        every live slot, in slot order, for tests and debugging: key, hit_count, miss_count, log_odds, the frame
 *                        of the last update, the sums (xyz 3 floats, covariance 6, rgb 4, intensity 1 per row). Each output may be
 *                        NULL; those given must hold sp_ogm_info(SP_OGM_INFO_VOXEL_NUM) rows.
 * Like the reference's methods these calls wait for their kernels. All array arguments are device pointers; *_host are host. */
typedef struct sp_occupancy_grid_map sp_occupancy_grid_map;
enum { SP_OGM_VOXEL_SIZE = 0, SP_OGM_LOG_ODDS_HIT = 1, SP_OGM_LOG_ODDS_MISS = 2, SP_OGM_LOG_ODDS_MIN = 3, SP_OGM_LOG_ODDS_MAX = 4,
       SP_OGM_OCCUPANCY_THRESHOLD = 5, SP_OGM_FREE_SPACE_UPDATES = 6, SP_OGM_VOXEL_PRUNING = 7, SP_OGM_STALE_FRAME_THRESHOLD = 8,
       SP_OGM_REHASH_THRESHOLD = 9 };
enum { SP_OGM_INFO_VOXEL_NUM = 0, SP_OGM_INFO_CAPACITY = 1, SP_OGM_INFO_FRAME_INDEX = 2, SP_OGM_INFO_HAS_COV = 3,
       SP_OGM_INFO_HAS_RGB = 4, SP_OGM_INFO_HAS_INTENSITY = 5 };
int sp_ogm_create(float voxel_size, void* stream, sp_occupancy_grid_map** out);
void sp_ogm_destroy(sp_occupancy_grid_map* map);
int sp_ogm_set(sp_occupancy_grid_map* map, int param, float value);
int sp_ogm_set_log_odds_limits(sp_occupancy_grid_map* map, float minimum, float maximum);
float sp_ogm_get(const sp_occupancy_grid_map* map, int param);
size_t sp_ogm_info(const sp_occupancy_grid_map* map, int what);
int sp_ogm_clear(sp_occupancy_grid_map* map, void* stream);
int sp_ogm_add_point_cloud(sp_occupancy_grid_map* map, const float* points, const float* covs, const float* rgb,
                           const float* intensities, size_t n, const float* sensor_pose_host16, void* stream);
int sp_ogm_extract_occupied_points(sp_occupancy_grid_map* map, const float* sensor_xyz_host3, float max_distance,
                                   float* points_out, float* covs_out, float* rgb_out, float* intensities_out,
                                   uint64_t* keys_out_opt, size_t out_capacity, size_t* n_out_host, void* stream);
int sp_ogm_extract_visible_points(sp_occupancy_grid_map* map, const float* sensor_pose_host16 /* column-major, map frame */,
                                  float max_distance, float horizontal_fov, float vertical_fov,
                                  float* points_out, float* covs_out, float* rgb_out, float* intensities_out,
                                  uint64_t* keys_out_opt, size_t out_capacity, size_t* n_out_host, void* stream);
int sp_ogm_overlap_ratio(const sp_occupancy_grid_map* map, const float* points, size_t n, const float* sensor_pose_host16,
                         float* ratio_out_host, void* stream);
int sp_ogm_voxel_probability(const sp_occupancy_grid_map* map, const float* xyz_host3, float* probability_out_host, void* stream);
int sp_ogm_export(sp_occupancy_grid_map* map, uint64_t* keys_out, uint32_t* hit_count_out, uint32_t* miss_count_out,
                  float* log_odds_out, uint32_t* last_updated_out, float* sum_xyz_out, float* cov_sums_out, float* rgb_sums_out,
                  float* intensity_sums_out, size_t out_capacity, size_t* n_out_host, void* stream);

/* ------------------------------------------------------- sensor_msgs/PointCloud2 ingestion (ros2/convert.hpp, ros2/enhanced_reflectivity.hpp)
 * A PointCloud2 is a byte buffer of n records of point_step bytes plus a list of named, typed fields. The reference unpacks the
 * coordinates, rgb and intensity in a kernel (convert.hpp:192-248) and leaves the time stamps (:144-190), the whole reflectivity
 * correction (enhanced_reflectivity.hpp:45-140) and the packing of toROS2msg (convert.hpp:376-426) as host loops over USM-shared
 * memory. Here all of it runs on the device. Field type codes are sensor_msgs/PointField's. */
enum { SP_PC2_INT8 = 1, SP_PC2_UINT8 = 2, SP_PC2_INT16 = 3, SP_PC2_UINT16 = 4, SP_PC2_INT32 = 5, SP_PC2_UINT32 = 6,
       SP_PC2_FLOAT32 = 7, SP_PC2_FLOAT64 = 8 };
#define SP_PC2_BLOCK_POINTS 256   /* records per workgroup of every kernel of this section */
#define SP_PC2_MAX_POINT_STEP 240 /* a workgroup's records are staged in LDS: 256 * 240 bytes and the sums' arrays fit 64 KiB */
#define SP_ER_MAX_RINGS 256       /* EnhancedReflectivityCorrector::MAX_RINGS */
#define SP_ER_STATE_BYTES (3 * 4 * SP_ER_MAX_RINGS) /* float ref_mean[256], float amb_mean[256], uint32 initialised[256] */
/* Where the fields of a record are: byte offsets inside the record, -1 = absent. */
typedef struct sp_pc2_layout {
    uint32_t point_step;
    int32_t x_offset, y_offset, z_offset, rgb_offset, intensity_offset, timestamp_offset;
    uint8_t xyz_type;       /* FLOAT32 / FLOAT64, the same for x, y and z */
    uint8_t rgb_type;       /* FLOAT32 / UINT32: four bytes either way */
    uint8_t intensity_type; /* FLOAT32 / UINT16 */
    uint8_t timestamp_type; /* FLOAT32 (s) / FLOAT64 (s, absolute when > 1e8) / UINT32 (ns) */
    double start_time_ms;   /* the header stamp (sec * 1000.0 + nanosec * 1e-6): FLOAT64 time stamps are taken relative to it */
} sp_pc2_layout;
/* fromROS2msg's field resolution (convert.hpp:38-136) over num_fields (name, offset, datatype) triples. Names: x, y, z; rgb / rgba;
 * intensity; reflectivity; t / time / timestamp / offset_time (a later field of the same role replaces an earlier one). With
 * convert_intensity and use_reflectivity_as_intensity a UINT16 reflectivity takes over the intensity (:112-121). An optional field
 * that is switched off or has a type the reference does not convert is dropped (offset -1, type 0). A missing x, y or z, a
 * coordinate type other than FLOAT32 / FLOAT64, or three types that are not equal -> SP_ERR_RUNTIME (the reference returns false).
 * A kept field whose offset + size exceeds point_step -> SP_ERR_INVALID_ARGUMENT (the reference would read past the record), as
 * are a null pointer and point_step == 0. start_time_ms is set to 0: the caller fills it in. Host only. */
int sp_pc2_resolve_fields_host(const char* const* names, const uint32_t* offsets, const uint8_t* datatypes, size_t num_fields,
                               uint32_t point_step, int convert_rgb, int convert_intensity, int use_reflectivity_as_intensity,
                               sp_pc2_layout* layout_out);
/* The conversion kernel of fromROS2msg (convert.hpp:192-248) and its host loop over the time stamps (:144-190) as one pass:
 *   points_out[i] = {float(x), float(y), float(z), 1} (FLOAT64 rounds to nearest);  rgb_out[i] = four bytes, each / 255.0f;
 *   intensities_out[i] = the float, or float(uint16);  timestamps_out[i] = float(offset_ms) with offset_ms, a double, from
 *     UINT32   float(u) * 1e-6f (a float, widened)
 *     FLOAT32  double(raw) * 1e3 if raw is finite and > 0, else 0
 *     FLOAT64  0 unless raw is finite and >= 0; raw > 1e8 ? raw * 1e3 - start_time_ms : raw * 1e3; a negative result becomes 0
 *   *max_offset_ms_dev = the largest offset_ms BEFORE the cast to float (what the reference adds to start_time_ms, :186-189).
 * Each workgroup pulls its SP_PC2_BLOCK_POINTS consecutive records into LDS with aligned 16-byte loads and picks the (unaligned)
 * fields from there; no load touches a byte at or beyond data_dev + data_bytes rounded up to 16. An attribute whose offset is -1
 * is not written and its pointer is ignored; max_offset_ms_dev is written, and workspace (sp_pc2_unpack_workspace_bytes(n) bytes
 * of device memory, 16-byte aligned: one value per workgroup, reduced by a second small launch) used, only with a time stamp field.
 * layout == NULL -> SP_ERR_INVALID_ARGUMENT; then n == 0 -> SP_OK, nothing enqueued. A null or not 16-byte aligned data_dev, a
 * null output of a present attribute, a null or not aligned workspace with a time stamp field, point_step == 0 or > SP_PC2_MAX_POINT_STEP, n * point_step > data_bytes, n >= 2^32, a type
 * outside the lists above, a field running past point_step, a start_time_ms that is not finite -> SP_ERR_INVALID_ARGUMENT
 * before any HIP call. Enqueue only. */
size_t sp_pc2_unpack_workspace_bytes(size_t n);
int sp_pc2_unpack(const void* data_dev, size_t data_bytes, size_t n, const sp_pc2_layout* layout, float* points_out,
                  float* rgb_out, float* intensities_out, float* timestamps_out, double* max_offset_ms_dev, void* workspace,
                  void* stream);
/* toROS2msg's packing loop (convert.hpp:394-426): record i = the 16 bytes of points[i], then, each only where its array is given,
 * four bytes uint8(clamp(c, 0, 1) * 255.0f) of rgb[i] (truncating; clamp = fminf(fmaxf(c, 0), 1), so NaN gives 0), the float
 * intensities[i], the double (start_time_ms + double(timestamps[i])) * 1e-3. data_out_dev: n * sp_pc2_pack_point_step(...) bytes,
 * 16-byte aligned. A null points or data_out_dev, a data_out_dev that is not aligned, n >= 2^32 -> SP_ERR_INVALID_ARGUMENT before
 * any HIP call. n == 0: SP_OK, nothing enqueued. Enqueue only. */
uint32_t sp_pc2_pack_point_step(int has_rgb, int has_intensity, int has_timestamp);
int sp_pc2_pack(const float* points, const float* rgb, const float* intensities, const float* timestamps, size_t n,
                double start_time_ms, void* data_out_dev, void* stream);
/* EnhancedReflectivityCorrector::apply (enhanced_reflectivity.hpp:45-140) as three launches and no read-back. Per point:
 * range_sq = x * x + y * y + z * z, ref = intensity * range_sq, amb = float(ambient) / range_sq, both 0 where range_sq < 1e-6f;
 * ring and ambient (UINT16) are read from the message's records (data_dev, 16-byte aligned, n * point_step bytes; loads reach
 * to the next 16-byte boundary at most).
 *   1. per ring < 256: sums of ref and amb and the count over the points with range_sq >= 1e-6f (:70-102)
 *   2. per ring with a count: mean = sum / float(count); state = mean on the first observation, else
 *      ema_alpha * mean + (1 - ema_alpha) * state (:107-123). state_dev: SP_ER_STATE_BYTES, zeroed by the caller once.
 *   3. intensity = clamp((ref / ref_mean if ref_mean > 0) + (amb / amb_mean if amb_mean > 0), 0, clip_max); 0 for a ring >= 256
 * The sums are deterministic: workgroup b sums its fixed span of consecutive points in index order, launch 2 adds the spans in
 * a fixed order (four slices of consecutive spans, each in span order, then the slices in order). No float atomics; the same bits from every call on the same input and state. workspace:
 * sp_enhanced_reflectivity_workspace_bytes(n) bytes of device memory, 16-byte aligned.
 * n == 0: SP_OK, nothing enqueued (no ring has points: the state stays). A null pointer, a data_dev that is not aligned,
 * point_step == 0 or > SP_PC2_MAX_POINT_STEP, a ring or ambient field running past point_step, n >= 2^32 ->
 * SP_ERR_INVALID_ARGUMENT before any HIP call. Enqueue only. */
size_t sp_enhanced_reflectivity_workspace_bytes(size_t n);
int sp_enhanced_reflectivity(const float* points, float* intensities_inout, size_t n, const void* data_dev, uint32_t point_step,
                             int32_t ring_offset, int ring_is_u8, int32_t ambient_offset, void* state_dev, float ema_alpha,
                             float clip_max, void* workspace, void* stream);

/* ---------------------------------------------------------------- global registration (MI355X extension)
 * Initial guesses for sp_gicp_align_batch / sp_vhm_align_batch from the data: FPFH descriptors, nearest neighbours in descriptor
 * space, and poses of matched triplets scored by how many matches they explain. The reference has nothing of the kind; the
 * definitions below are the specification. No float atomics anywhere: two calls on the same input give the same bits.
 *
 * sp_fpfh_compute: one descriptor row of SP_FPFH_STRIDE floats per point (33 bins, then 3 zeros: 144 bytes, 16-byte aligned).
 *   points, normals  n x float4. The normals must be of unit length and CONSISTENTLY ORIENTED (what sp_normals_from_knn gives a
 *                    scan whose sensor sits at the origin): the features are signed, a flipped normal is another descriptor.
 *   knn_idx, knn_d2  a kNN result of the cloud on itself, n x k, padding -1 / FLT_MAX, k <= SP_FPFH_MAX_K; a list may or may
 *                    not hold the point itself. Entries outside [0, n) are treated as padding.
 *   SPFH of point i  its neighbours are the entries j >= 0, j != i in list order, m of them. A pair (i, j) with d = p_j - p_i,
 *                    dist = |d| is skipped when dist == 0 or a value is not finite. The frame sits at the query point (no swap
 *                    of the two points): f3 = n_i.d / dist; v = d x n_i, skipped when |v| == 0, v /= |v|; w = n_i x v;
 *                    f2 = v.n_j; f1 = atan2(w.n_j, n_i.n_j). b1 = floor(11 (f1 + pi) / 2 pi), b2 = floor(11 (f2 + 1) / 2),
 *                    b3 = floor(11 (f3 + 1) / 2), each clamped to 0..10; the pair adds 1 to count[b1], count[11 + b2],
 *                    count[22 + b3]. SPFH_i[b] = float(count[b]) * (100.0f / float(m)); all zero for m == 0.
 *   FPFH of point i  F[b] = sum over the same neighbours, in ascending list position as an fmaf chain from 0, of
 *                    (1 / d2_ij) * SPFH_j[b] with the list's own d2 (entries with d2 == 0 skipped); then each of the three
 *                    groups of 11 bins is scaled to sum 100 (a group that sums to 0 stays 0).
 *   spfh_counts_out_opt / spfh_m_out_opt  n x 33 and n uint16, may be null: the counts and m, for tests and diagnosis.
 *   workspace        sp_fpfh_workspace_bytes(n) bytes (the SPFH rows, 144 n), 16-byte aligned.
 * Two launches (SPFH: a wave per point, a lane per neighbour, the histogram by ballots; FPFH: a wave per point, a lane per bin).
 * n == 0: SP_OK. k == 0 or > SP_FPFH_MAX_K, a null pointer, n >= 2^31, a workspace that is too small -> SP_ERR_INVALID_ARGUMENT.
 *
 * sp_feature_match: for every row of `a` (na x SP_FPFH_STRIDE) the row of `b` with the smallest squared L2 distance over the 33
 * bins, computed as |a|^2 + |b|^2 - 2 a.b (the norms summed in double and rounded once, the product on v_mfma_f32_32x32x2_f32:
 * exact f32, an fmaf chain), clamped at 0; ties in the computed distance go to the lowest index. idx_out na int32, d2_out_opt
 * na floats (may be null); nb == 0 gives -1 / FLT_MAX. na, nb <= SP_FEATURE_MATCH_MAX. The targets are split into chunks over
 * the grid and combined by a 64-bit integer atomicMin on (bits of d2) << 32 | index: order-independent.
 * workspace: sp_feature_match_workspace_bytes(na, nb), which is 0 beyond the limits.
 *
 * sp_feature_match_mutual: both directions, then the source rows i with match_t->s(match_s->t(i)) == i, as (i, j) int32 pairs in
 * ascending i (flags -> scan -> compaction: sp_compact_by_flags). corr_out: room for min(ns, nt) pairs. *count_out_host receives
 * the number of pairs by one read-back (the call synchronises the stream). workspace: sp_feature_match_mutual_workspace_bytes.
 *
 * sp_correspondence_points: cs_out[m] = src_points[corr[m][0]], ct_out[m] = tgt_points[corr[m][1]] (float4 rows). Enqueue only.
 *
 * sp_ransac_score: score_out[h] (uint32, device) for hypotheses h in [0, H), H <= SP_RANSAC_MAX_HYPOTHESES, from the matched
 * points cs, ct (M x float4, device). Hypothesis h draws r_j = splitmix64(seed + 3 h + j), index_j = ((r_j >> 32) * M) >> 32,
 * j = 0, 1, 2 (sp_ransac_triplets_host computes the same on the host), with splitmix64(z): z += 0x9E3779B97F4A7C15;
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31. It scores 0 unless the three
 * indices are distinct, every source edge is longer than min_edge, min(l_s, l_t) >= edge_ratio * max(l_s, l_t) for each of the
 * three edges, and both triangles satisfy |e x f|^2 >= 0.04 |e|^2 |f|^2 (e = p1 - p0, f = p2 - p0). Its pose aligns the triangle
 * frames e1 = e / |e|, e3 = (e1 x f) / |e1 x f|, e2 = e3 x e1: R = [e1 e2 e3]_t [e1 e2 e3]_s^T, t = centroid_t - R centroid_s;
 * its score is the number of m with |R cs_m + t - ct_m|^2 < inlier_distance^2. One lane per hypothesis, the matches pass through
 * LDS in tiles. M < 3: every score 0. Enqueue only.
 *
 * sp_ransac_select_host (host memory only): the `guesses` hypotheses with the highest nonzero scores, ties to the lower h, their
 * poses recomputed in double from the same triplets of host copies of cs, ct: poses_out[g] 16 doubles, column-major;
 * hyp_out_opt[g] the hypothesis. *count_out <= guesses poses are written (fewer when fewer scores are nonzero). */
enum { SP_FPFH_BINS = 33, SP_FPFH_STRIDE = 36, SP_FPFH_MAX_K = 64, SP_FEATURE_MATCH_MAX = 1 << 20,
       SP_RANSAC_MAX_HYPOTHESES = 1 << 20 };
size_t sp_fpfh_workspace_bytes(size_t n);
int sp_fpfh_compute(const float* points, const float* normals, size_t n, const int32_t* knn_idx, const float* knn_d2, size_t k,
                    float* fpfh_out, uint16_t* spfh_counts_out_opt, uint16_t* spfh_m_out_opt, void* workspace,
                    size_t workspace_bytes, void* stream);
size_t sp_feature_match_workspace_bytes(size_t na, size_t nb);
int sp_feature_match(const float* a, size_t na, const float* b, size_t nb, int32_t* idx_out, float* d2_out_opt, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t sp_feature_match_mutual_workspace_bytes(size_t ns, size_t nt);
int sp_feature_match_mutual(const float* src, size_t ns, const float* tgt, size_t nt, int32_t* corr_out,
                            uint32_t* count_out_host, void* workspace, size_t workspace_bytes, void* stream);
int sp_correspondence_points(const float* src_points, size_t ns, const float* tgt_points, size_t nt, const int32_t* corr, size_t m,
                             float* cs_out, float* ct_out, void* stream);
int sp_ransac_score(const float* cs, const float* ct, size_t m, size_t hypotheses, uint64_t seed, float inlier_distance,
                    float min_edge, float edge_ratio, uint32_t* score_out, void* stream);
int sp_ransac_triplets_host(uint64_t seed, size_t first_hypothesis, size_t count, size_t m, uint32_t* triplets_out);
int sp_ransac_select_host(const uint32_t* scores_host, size_t hypotheses, const float* cs_host, const float* ct_host, size_t m,
                          uint64_t seed, size_t guesses, double* poses_out, uint32_t* hyp_out_opt, size_t* count_out);

/* ---------------------------------------------------------------- place recognition (MI355X extension)
 * Scan Context: a polar height image per scan, compared with every earlier one under every column shift. It answers "have I been
 * here before, and at what heading?": the best shift is a yaw estimate, the initial guess sp_gicp_align_batch wants. The whole
 * range of the database is compared exactly (no ring-key pre-filter). The reference has nothing of the kind; the definitions
 * below are the specification. No float atomics anywhere: two calls on the same input give the same bits.
 *
 * sp_scan_context_params: rings in 1..SP_SCAN_CONTEXT_MAX_RINGS (default 20), sectors even and in 4..SP_SCAN_CONTEXT_MAX_SECTORS
 * (60), max_range finite and > 0 (80), sensor_height (2). Anything else: SP_ERR_INVALID_ARGUMENT, from every entry point.
 *
 * sp_scan_context_compute / sp_scan_context_compute_host (its twin on host memory): desc_out[rings x sectors] floats, ring-major,
 * from n points (float4 rows). All arithmetic is plain f32 without contraction, in the order written:
 *   skipped   a point (x, y, z, .) with x, y or z not finite; with r2 = x*x + y*y == 0; with r = sqrtf(r2) >= max_range.
 *   ring      min(rings - 1, (int)floorf(r * (float)(rings / max_range))), the quotient formed once in double and rounded to float.
 *   sector    without atan2. sp_scan_context_boundaries_host(sectors, cos_out, sin_out) gives c_k = (float)cos(phi_k),
 *             s_k = (float)sin(phi_k), phi_k = -pi + 2 pi k / sectors in double, k = 0 .. sectors - 1. With h = sectors / 2 and
 *             ge(k) = (c_k * y >= s_k * x): sector = h + #{k in h+1 .. sectors-1 : ge(k)} when y >= 0 (-0.0 included), else
 *             #{k in 1 .. h-1 : ge(k)}. A count: well defined even where rounding makes ge non-monotone in k.
 *   value     v = z + sensor_height if that is > 0, else 0. The bin holds the maximum v of its points; an empty bin holds 0.
 * The maximum does not depend on the order of the points: the device's descriptor equals the host twin's bit for bit (an integer
 * atomicMax on the bits of v >= 0, per workgroup in LDS, then one global atomicMax per bin the workgroup touched). n == 0: all
 * zeros, SP_OK. A null pointer, n >= 2^32: SP_ERR_INVALID_ARGUMENT. Enqueue only.
 *
 * The database (sp_scan_context_db_create .. _add): descriptors of one parameter set, at most SP_SCAN_CONTEXT_DB_MAX. Creating one
 * takes no device memory (capacity_hint entries are taken at the first add); growth past the capacity doubles the storage and
 * copies on the device, entries unchanged. add(db, desc_device, stream) appends the descriptor as, per column j: the normalised
 * column C^[i][j] = D[i][j] / n_j in f32 with n_j = (float)sqrt(sum_i (double)D[i][j]^2) (i ascending, rounded once), zeros when
 * n_j == 0; and bit j of a 64-bit mask of the columns with n_j != 0. (The norm itself is not kept: the search reads only these.)
 * An entry is K_pad x 32 or 64 floats (K_pad = rings rounded up to a multiple of 4; 64 columns when sectors > 32) in the order a
 * wave of the search loads its matrix-core operands. add and search only enqueue on the caller's stream; a database is used
 * from one host thread at a time and from ONE stream, or from streams the caller orders among themselves: growth copies the
 * entries on the stream of the add that triggers it and waits for no other stream. size: the entries added so far; clear: size 0, the storage kept.
 *
 * sp_scan_context_db_search: the query descriptor (device, normalised as in add: Q^) against the entries [first, first + count)
 * — the usual loop-closure call leaves out the most recent keyframes by its choice of count. For candidate C and shift s in
 * 0 .. sectors - 1: N_s = #{j : column (j + s) mod sectors of Q and column j of C are both non-empty},
 * d_s = 1 - (1 / N_s) sum_j Q^[:, (j + s) mod sectors] . C^[:, j] (the dot products on v_mfma_f32_32x32x2_f32: exact f32, an fmaf
 * chain over the rings; the sum over j ascending), clamped at 0; d_s = 1 when N_s == 0. The candidate's distance is min_s d_s, its
 * shift the lowest s that attains it in the computed values. Output: the k <= SP_SCAN_CONTEXT_MAX_K candidates with the smallest
 * key (bits of distance) << 32 | index, ascending by key (equal distances: the lower index first); idx_out (int32, ABSOLUTE index,
 * not relative to first), dist_out (float), shift_out (int32), k rows each, device; rows beyond count are -1 / FLT_MAX / 0.
 * Convention: a scan turned by +s sectors about z has its columns moved from j to j + s, so shift s says the query is the candidate
 * turned by s * 2 pi / sectors, and Rz(-s * 2 pi / sectors) takes query points into the candidate's frame.
 * workspace: sp_scan_context_db_search_workspace_bytes(db, count) bytes (0 for a null db or count > SP_SCAN_CONTEXT_DB_MAX),
 * 16-byte aligned. Every entry of the range is read once. k == 0: SP_OK, nothing written. A range outside [0, size), k too
 * large, a null pointer, a workspace that is too small: SP_ERR_INVALID_ARGUMENT before any HIP call.
 *
 * sp_scan_context_guesses_host (host only): `steps` poses Rz(-(shift + delta) * 2 pi / sectors) with zero translation, 16 doubles
 * each, column-major (as sp_ransac_select_host's); delta evenly spaced over [-1/2, +1/2] (delta_i = -1/2 + i / (steps - 1)),
 * steps == 1: delta = 0; an odd steps contains delta = 0. shift >= sectors: SP_ERR_INVALID_ARGUMENT. */
typedef struct sp_scan_context_params {
    uint32_t rings, sectors;
    float max_range, sensor_height;
} sp_scan_context_params;
typedef struct sp_scan_context_db sp_scan_context_db;
enum { SP_SCAN_CONTEXT_MAX_RINGS = 32, SP_SCAN_CONTEXT_MAX_SECTORS = 64, SP_SCAN_CONTEXT_MAX_K = 32,
       SP_SCAN_CONTEXT_DB_MAX = 1 << 20 };
int sp_scan_context_boundaries_host(uint32_t sectors, float* cos_out, float* sin_out);
int sp_scan_context_compute(const sp_scan_context_params* params, const float* points, size_t n, float* desc_out, void* stream);
int sp_scan_context_compute_host(const sp_scan_context_params* params, const float* points_host, size_t n, float* desc_out_host);
int sp_scan_context_db_create(const sp_scan_context_params* params, size_t capacity_hint, sp_scan_context_db** out);
void sp_scan_context_db_destroy(sp_scan_context_db* db);
size_t sp_scan_context_db_size(const sp_scan_context_db* db);
int sp_scan_context_db_clear(sp_scan_context_db* db);
int sp_scan_context_db_add(sp_scan_context_db* db, const float* desc_device, void* stream);
size_t sp_scan_context_db_search_workspace_bytes(const sp_scan_context_db* db, size_t count);
int sp_scan_context_db_search(sp_scan_context_db* db, const float* desc_device, size_t first, size_t count, size_t k,
                              int32_t* idx_out, float* dist_out, int32_t* shift_out, void* workspace, size_t workspace_bytes,
                              void* stream);
int sp_scan_context_guesses_host(const sp_scan_context_params* params, uint32_t shift, size_t steps, double* poses_out);

/* ---------------------------------------------------------------- compatibility-graph guesses (MI355X extension)
 * A second source of initial guesses for sp_gicp_align_batch / sp_vhm_align_batch, beside sp_ransac_score's triplets: a graph over
 * the matches whose edges say "a rigid motion would keep the distance between these two", its second-order form (common
 * neighbours), and least-squares poses of the densest neighbourhoods. It finds the pose where the inliers are a few per cent of
 * the matches, which random triplets do not. The reference has nothing of the kind; the definitions below are the specification.
 * Every quantity on the device is an integer or a fixed f32 expression: two calls on the same input give the same bits, and the
 * device equals the host twins (*_host, host memory only) bit for bit.
 *
 * Inputs: cs, ct  M x float4 matched points (sp_correspondence_points), 3 <= M <= SP_COMPAT_MAX_MATCHES; tau > 0 and min_edge >= 0.
 *
 * 1. C[a][b] (0 or 1), with t2 = tau * tau and e2 = min_edge * min_edge in f32, d = cs_a - cs_b and g = ct_a - ct_b componentwise,
 *    u = fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x)), v the same of g, q = (u + v) - t2:
 *      C[a][b] = 1  iff  a != b  and  u > e2  and  v > e2  and  (q < 0  or  q * q < (4 * u) * v).
 *    That is | |d| - |g| | < tau without a square root. No contraction: every operation above is one f32 rounding. A NaN anywhere
 *    gives 0. C is symmetric bit for bit (d and g only change sign). The device keeps C as bytes, rows padded with zeros to a
 *    multiple of 128; degree_a = sum_b C[a][b].
 * 2. S[a][b] = C[a][b] * sum_k C[a][k] C[b][k] (the common compatible neighbours of a compatible pair), on
 *    v_mfma_i32_32x32x32_i8: exact. s_a = sum_b S[a][b] (uint32; <= 2^26). S is never stored; the per-tile partial sums of s are
 *    combined by integer atomic adds: order-independent.
 * 3. Seeds: the `seeds` <= SP_COMPAT_MAX_SEEDS matches with the largest key (s_a descending, a ascending) among those with
 *    s_a > 0. seed_idx_out / seed_s_out: `seeds` entries, int32 / uint32, rank order, -1 / 0 beyond the last seed.
 * 4. Consensus lists: for the seed of rank r, row a of S is computed again (a second, small matrix-core launch) and the
 *    k <= SP_COMPAT_MAX_K matches b with the largest key (S[a][b] descending, b ascending) among those with S[a][b] > 0 are
 *    written to cons_out[r * k ..] (int32, -1 beyond the last; a row of -1 for seed_idx[r] < 0), cons_s_out_opt the S values.
 * 5. sp_compat_poses_host: for every rank r whose list holds at least 2 companions, the unweighted least-squares rigid pose
 *    (Horn's quaternion method, in double) of the set {a} + list from host copies of cs, ct. A set whose source or target points
 *    are collinear or coincident (middle eigenvalue of the 3x3 scatter matrix <= 1e-10 x the largest) or not finite yields
 *    nothing. Poses are written in rank order: poses_out[p] 16 doubles column-major (as sp_ransac_select_host's),
 *    rank_out_opt[p] the seed rank; *count_out of them.
 * 6. sp_pose_score: score_out[p] (uint32, device) = the number of m with |R cs_m + t - ct_m|^2 < inlier_distance^2 for each of P
 *    <= SP_RANSAC_MAX_HYPOTHESES poses (device, 16 floats each, column-major), the residual expression of sp_ransac_score:
 *    r.x = fmaf(R02, z, fmaf(R01, y, fmaf(R00, x, t.x))) - ct.x ..., fmaf(r.z, r.z, fmaf(r.y, r.y, r.x * r.x)) < tau2.
 * 7. sp_compat_select_host: the `guesses` poses with the highest nonzero score, ties to the earlier pose (the earlier seed rank);
 *    output as in 5.
 *
 * sp_compat_seeds runs 1 - 3 and leaves C in the workspace; sp_compat_consensus runs 4 from the SAME workspace and m, after it on
 * the same stream. degree_out_opt / s_out_opt (m uint32 each, device, may be null) are for tests. workspace:
 * sp_compat_workspace_bytes(m) bytes (0 beyond the limit), 16-byte aligned: Mp^2 + 12 Mp + 1024 Mp bytes, Mp = m rounded up to 128.
 * m < 3: every list empty (-1 / 0), SP_OK. m > SP_COMPAT_MAX_MATCHES, seeds or k over its limit, a null pointer, a tau that is
 * not > 0, a negative min_edge, a short or misaligned workspace: SP_ERR_INVALID_ARGUMENT before any HIP call. All enqueue only. */
enum { SP_COMPAT_MAX_MATCHES = 8192, SP_COMPAT_MAX_SEEDS = 256, SP_COMPAT_MAX_K = 64 };
size_t sp_compat_workspace_bytes(size_t m);
int sp_compat_seeds(const float* cs, const float* ct, size_t m, float tau, float min_edge, size_t seeds, int32_t* seed_idx_out,
                    uint32_t* seed_s_out, uint32_t* degree_out_opt, uint32_t* s_out_opt, void* workspace, size_t workspace_bytes,
                    void* stream);
int sp_compat_consensus(size_t m, const int32_t* seed_idx, size_t seeds, size_t k, int32_t* cons_out, uint32_t* cons_s_out_opt,
                        void* workspace, size_t workspace_bytes, void* stream);
int sp_compat_seeds_host(const float* cs_host, const float* ct_host, size_t m, float tau, float min_edge, size_t seeds,
                         int32_t* seed_idx_out, uint32_t* seed_s_out, uint32_t* degree_out_opt, uint32_t* s_out_opt);
int sp_compat_consensus_host(const float* cs_host, const float* ct_host, size_t m, float tau, float min_edge,
                             const int32_t* seed_idx, size_t seeds, size_t k, int32_t* cons_out, uint32_t* cons_s_out_opt);
int sp_compat_poses_host(const float* cs_host, const float* ct_host, size_t m, const int32_t* seed_idx, const int32_t* cons,
                         size_t seeds, size_t k, double* poses_out, uint32_t* rank_out_opt, size_t* count_out);
int sp_pose_score(const float* cs, const float* ct, size_t m, const float* poses, size_t count, float inlier_distance,
                  uint32_t* score_out, void* stream);
int sp_compat_select_host(const uint32_t* scores_host, const double* poses_in, const uint32_t* rank_in_opt, size_t count,
                          size_t guesses, double* poses_out, uint32_t* rank_out_opt, size_t* count_out);

/* ------------------------------------------------------------------------------------------- photometric (intensity) term
 * MI355X extension (the reference fetches intensities in its linearisation kernel and ignores them): the photometric objective of
 * Park, Zhou, Koltun, "Colored Point Cloud Registration Revisited" (ICCV 2017) on a cloud's scalar intensities.
 *
 * 1. sp_intensity_gradient: per point a with unit normal n and the neighbours j of its own kNN row (knn_idx: n x k, row-major),
 *      u_j = (p_j - p_a) - ((p_j - p_a) . n) n,  M = sum u_j u_j^T + m^2 n n^T,  g = sum u_j (I_j - I_a)   (m neighbours used)
 *      d = M^-1 g by the symmetric adjugate inverse, then d <- d - (d . n) n.
 *    A neighbour is skipped when its index is negative (or past the cloud), when it is the point itself, or when its intensity or
 *    point is not finite. rows_out: n float4 (d.x, d.y, d.z, I_a). (0, 0, 0, NaN): fewer than 3 neighbours used, I_a or n not
 *    finite, or |det M| < 1e-6; (0, 0, 0, I_a): d came out non-finite. The gradients are in the frame the cloud is in at the call.
 *    points / normals: n x 4 floats. One lane per point; the host twin runs the same function: the same bits.
 *    k < 2 or a null pointer: SP_ERR_INVALID_ARGUMENT before any HIP call. n == 0: SP_OK.
 * 2. sp_photometric_linearize: for source point s (intensity I_s) with q = T s and winner t = nn_idx[s] (target row (d_t, I_t)):
 *      r = (I_t + d_t . (q - t)) - I_s,   J = d_t^T [-R S | R], S = skew(s)   (the twist of sp_gicp_linearize: rotation first)
 *    and the point adds rho J^T J, rho J^T r and the robust error of |r| (robust_type / robust_scale: the SP_LOSS_* kernels) to
 *    *out. It adds nothing when nn_idx < 0, nn_d2 > max_correspondence_distance^2 (the rejection of sp_gicp_linearize), the target
 *    row's w is NaN, or I_s is not finite; out->inlier counts the points that add. `weight` is NOT applied here: the caller scales
 *    the system. rows_out_opt (may be null; device, 16-byte aligned): every point's 28 values (21 upper entries of H row-major, 6
 *    of b, the error), zeros for a point that adds nothing. The sums are a fixed tree without float atomics: two launches give the
 *    same bytes. transT: host or device, as for sp_gicp_linearize. workspace: sp_photometric_workspace_bytes(n), 16-byte aligned.
 *    sp_photometric_error: out->error and out->inlier alone.
 *    A null pointer, a short or misaligned workspace, a robust type out of range, a robust_scale that is not > 0 when a loss is
 *    set: SP_ERR_INVALID_ARGUMENT before any HIP call. n == 0: *out zeroed, SP_OK. All enqueue only.
 * The *_host twins take host memory and run the same per-point functions on the CPU: rows bit for bit under every loss (the Tukey
 * and Cauchy errors are evaluated without powf / logf, a few ulp from the values sp_gicp_linearize's robust kernel gives); their
 * sums are within the classical bound of any summation order. */
typedef struct sp_photometric_params {
    float weight;        /* what the caller multiplies the term's H, b and error by; 0: the term is off */
    int robust_type;     /* SP_LOSS_* */
    float robust_scale;
    float max_correspondence_distance;
} sp_photometric_params;
int sp_intensity_gradient(const float* points, const float* normals, const float* intensities, size_t n, const int32_t* knn_idx,
                          size_t k, float* rows_out, void* stream);
int sp_intensity_gradient_host(const float* points, const float* normals, const float* intensities, size_t n,
                               const int32_t* knn_idx, size_t k, float* rows_out);
size_t sp_photometric_workspace_bytes(size_t n);
int sp_photometric_linearize(const float* src_points, const float* src_intensities, size_t n, const float* tgt_points,
                             const float* tgt_rows, const int32_t* nn_idx, const float* nn_d2, const float* transT,
                             int transT_on_device, const sp_photometric_params* params, sp_linearized* out, float* rows_out_opt,
                             void* workspace, size_t workspace_bytes, void* stream);
int sp_photometric_error(const float* src_points, const float* src_intensities, size_t n, const float* tgt_points,
                         const float* tgt_rows, const int32_t* nn_idx, const float* nn_d2, const float* transT, int transT_on_device,
                         const sp_photometric_params* params, sp_linearized* out, void* workspace, size_t workspace_bytes,
                         void* stream);
int sp_photometric_linearize_host(const float* src_points, const float* src_intensities, size_t n, const float* tgt_points,
                                  const float* tgt_rows, const int32_t* nn_idx, const float* nn_d2, const float* transT,
                                  const sp_photometric_params* params, sp_linearized* out, float* rows_out_opt);
int sp_photometric_error_host(const float* src_points, const float* src_intensities, size_t n, const float* tgt_points,
                              const float* tgt_rows, const int32_t* nn_idx, const float* nn_d2, const float* transT,
                              const sp_photometric_params* params, sp_linearized* out);

#ifdef __cplusplus
}
#endif
#endif /* SYCL_POINTS_AMD_H */
