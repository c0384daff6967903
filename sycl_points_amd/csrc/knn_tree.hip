// sp_knn_tree: the accelerated KDTree behind the facade's KDTree (include/sycl_points/amd/knn.hpp) and
// sycl_points_amd.api.KDTree(accelerate=True) — its own copy of the points, the structures built from it on first need, and
// the rule that picks which one answers a search. Host code only. The rule, in order (backend_of):
//   * below 1024 points, k > 32 or the reference's tie order: the reference's tree (sp_kdtree_*). Below 1024 points it is
//     built at create (the host build takes microseconds and its balanced tree is the shallower one), else on first need;
//   * the tree's own cloud, untouched, 8 <= k <= 20, 32 k points or more of near-uniform density (the fullest cell of a
//     6-points-per-cell grid holds at most 48): that grid (1 M points, k = 20: 0.6 ms against 5.5 ms for the hierarchy);
//   * a small cloud (the reference example's 6 k-point scans): the exact brute-force search, tens of microseconds, where
//     building the hierarchy alone takes 0.17 ms;
//   * else the device-built hierarchy (sp_bvh_*; the own cloud is walked in tree order, 1.5x faster than in query order).
// The last three break distance ties by the lowest index: the same lists.
#include <vector>

#include "sp_common.h"

void sp_set_error(const char* msg);

namespace {
constexpr size_t kDeviceBuildMinPoints = 1024, kHierarchyMaxK = 32;
constexpr size_t kGridSelfMinPoints = 32768;
constexpr float kGridSelfPointsPerCell = 6.0f;
constexpr uint32_t kGridSelfMaxCell = 48;
constexpr size_t kBruteForceMaxTargets = 16384, kBruteForceMaxQueries = 65536;

struct Removal { std::vector<int32_t> indices; std::vector<uint8_t> flags; };
}  // namespace

struct sp_knn_tree {
    size_t n = 0, leaf_threshold = 16;
    float* pts = nullptr;           // the tree's copy of the points
    sp_bvh* bvh = nullptr;
    sp_grid* grid = nullptr;        // on the own cloud, kept if its density allows (grid_tried: decided)
    void* grid_ws = nullptr;
    bool grid_tried = false, pristine = true, reference_order = false;
    sp_kdtree* kd = nullptr;
    std::vector<Removal> removals;  // lazy deletes made before kd existed: replayed when it is built
    sp::StreamSet streams;
};

namespace {
int hip_fail(hipError_t e) {
    sp_set_error(hipGetErrorString(e));
    return SP_ERR_HIP;
}

bool on_hierarchy(const sp_knn_tree* t) { return t->n >= kDeviceBuildMinPoints && !t->reference_order; }

int build_hierarchy(sp_knn_tree* t, hipStream_t st) { return t->bvh ? SP_OK : sp_bvh_create(t->pts, t->n, st, &t->bvh); }

// The reference's tree from a host copy of the points (synchronises), with the lazy deletes it missed replayed in their order.
int build_host_tree(sp_knn_tree* t, hipStream_t st) {
    if (t->kd) return SP_OK;
    std::vector<float> host(4 * t->n + 4);
    hipError_t e = t->n ? hipMemcpyAsync(host.data(), t->pts, t->n * 16, hipMemcpyDeviceToHost, st) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    int rc = e == hipSuccess ? sp_kdtree_create(host.data(), t->n, t->leaf_threshold, st, &t->kd) : hip_fail(e);
    for (size_t i = 0; rc == SP_OK && i < t->removals.size(); ++i) {
        const Removal& r = t->removals[i];
        const size_t m = r.indices.size();
        int32_t* d = nullptr;  // m indices, then m flags
        e = sp::pooled_alloc(&d, m * 5, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d, r.indices.data(), m * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d + m, r.flags.data(), m, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) rc = sp_kdtree_remove_by_flags(t->kd, reinterpret_cast<const uint8_t*>(d + m), d, m, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        sp::pooled_free(d);
        if (e != hipSuccess) rc = hip_fail(e);
    }
    if (rc != SP_OK) {  // (the next attempt starts over)
        sp_kdtree_destroy(t->kd);
        t->kd = nullptr;
        return rc;
    }
    t->removals.clear();
    return SP_OK;
}

void drop_grid(sp_knn_tree* t) {
    sp_grid_destroy(t->grid);
    sp::pooled_free_after(t->grid_ws, t->streams);
    t->grid = nullptr;
    t->grid_ws = nullptr;
}

int try_grid(sp_knn_tree* t, hipStream_t st) {
    if (t->grid_tried || t->n < kGridSelfMinPoints) return SP_OK;
    t->grid_tried = true;
    int rc = sp_grid_create(t->pts, t->n, 0.0f, kGridSelfPointsPerCell, st, &t->grid);
    if (rc == SP_OK && sp_grid_max_cell_points(t->grid) <= kGridSelfMaxCell) {
        const hipError_t e = sp::pooled_alloc(&t->grid_ws, sp_grid_self_workspace_bytes(t->grid), st);
        if (e == hipSuccess) return SP_OK;
        rc = hip_fail(e);
    }
    drop_grid(t);  // (surfaces, clusters: the hierarchy's case)
    return rc;
}

// NULL or a host identity (Eigen's operator==): no transform. A device matrix always counts as one.
bool is_transform(const float* transT, int transT_on_device) {
    if (transT == nullptr) return false;
    if (transT_on_device) return true;
    for (int i = 0; i < 16; ++i)
        if (transT[i] != (i % 5 == 0 ? 1.0f : 0.0f)) return true;
    return false;
}

// `own`: own_cloud, checked against what the caller cannot see (nothing removed) and the transform.
int backend_of(sp_knn_tree* t, size_t nq, size_t k, bool transform, bool own, hipStream_t st, int* out) {
    *out = SP_KNN_HOST_TREE;
    if (!on_hierarchy(t) || k > kHierarchyMaxK) return SP_OK;
    if (own && k >= 8 && k <= 20) {
        const int rc = try_grid(t, st);
        if (rc != SP_OK) return rc;
        if (t->grid) {
            *out = SP_KNN_GRID;
            return SP_OK;
        }
    }
    // (sp_knn_bruteforce's one launch with the cloud in LDS, or from 2048 targets its bounded passes)
    const bool brute_force = t->pristine && k <= 20 && !transform && nq <= kBruteForceMaxQueries &&
                             (sp::small_applies(nq, t->n) || (t->n >= 2048 && t->n <= kBruteForceMaxTargets && t->n >= 256 * k));
    *out = brute_force ? SP_KNN_BRUTE_FORCE : SP_KNN_HIERARCHY;
    return SP_OK;
}

bool own_cloud_of(const sp_knn_tree* t, size_t nq, bool transform, int own_cloud) {
    return own_cloud && t->pristine && !transform && nq == t->n;
}
}  // namespace

extern "C" int sp_knn_tree_create(const float* points, size_t n, size_t leaf_threshold, void* stream, sp_knn_tree** out) {
    if (!out) return SP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (leaf_threshold == 0 || leaf_threshold > 4096) {  // (here, not when the reference's tree is first needed: as sp_kdtree_create)
        sp_set_error("[KDTree::build] leaf_threshold must be in [1, 4096]");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = sp::as_stream(stream);
    sp_knn_tree* t = new sp_knn_tree();
    t->n = n;
    t->leaf_threshold = leaf_threshold;
    t->streams.note(st);
    // (like the nodes of the reference's tree: the source cloud may be gone or changed by the time the tree is searched —
    // 16 MB per million points, a few microseconds on the device, no synchronisation)
    hipError_t e = sp::pooled_alloc(&t->pts, n * 16, st);
    if (e == hipSuccess && n) e = hipMemcpyAsync(t->pts, points, n * 16, hipMemcpyDeviceToDevice, st);
    int rc = e == hipSuccess ? SP_OK : hip_fail(e);
    if (rc == SP_OK && n < kDeviceBuildMinPoints) rc = build_host_tree(t, st);
    if (rc != SP_OK) {
        sp_knn_tree_destroy(t);
        t = nullptr;
    }
    *out = t;
    return rc;
}

extern "C" void sp_knn_tree_destroy(sp_knn_tree* t) {
    if (!t) return;
    sp_kdtree_destroy(t->kd);
    sp_bvh_destroy(t->bvh);
    drop_grid(t);
    sp::pooled_free_after(t->pts, t->streams);
    delete t;
}

extern "C" int sp_knn_tree_backend(sp_knn_tree* t, size_t nq, size_t k, const float* transT, int transT_on_device,
                                   int own_cloud, void* stream, int* backend_out) {
    if (!t || !backend_out) return SP_ERR_INVALID_ARGUMENT;
    hipStream_t st = sp::as_stream(stream);
    t->streams.note(st);
    const bool transform = is_transform(transT, transT_on_device);
    return backend_of(t, nq, k, transform, own_cloud_of(t, nq, transform, own_cloud), st, backend_out);
}

extern "C" int sp_knn_tree_search(sp_knn_tree* t, const float* queries, size_t nq, size_t k, const float* transT,
                                  int transT_on_device, int own_cloud, int32_t* idx_out, float* d2_out, void* stream) {
    if (!t) return SP_ERR_INVALID_ARGUMENT;
    if (k > 100) {
        sp_set_error("[KDTree::knn_search_async] `k` is too large. not support.");
        return SP_ERR_RUNTIME;
    }
    if (nq == 0) return SP_OK;
    hipStream_t st = sp::as_stream(stream);
    t->streams.note(st);
    const bool transform = is_transform(transT, transT_on_device);
    const bool own = own_cloud_of(t, nq, transform, own_cloud);
    int backend, rc = backend_of(t, nq, k, transform, own, st, &backend);
    if (rc != SP_OK) return rc;
    if (backend == SP_KNN_BRUTE_FORCE) {
        const size_t ws_bytes = sp_knn_bruteforce_workspace_bytes(nq, t->n, k);
        void* ws = nullptr;
        const hipError_t e = ws_bytes ? sp::pooled_alloc(&ws, ws_bytes, st) : hipSuccess;
        if (e != hipSuccess) return hip_fail(e);
        rc = sp_knn_bruteforce(queries, nq, t->pts, t->n, k, idx_out, d2_out, ws, ws_bytes, st);
        sp::StreamSet used;  // (back to the pool behind this stream's work: its next user on the stream does not wait)
        used.note(st);
        sp::pooled_free_after(ws, used);
        return rc;
    }
    if (backend == SP_KNN_GRID)
        return sp_grid_self_knn(t->grid, k, idx_out, d2_out, nullptr, nullptr, t->grid_ws, sp_grid_self_workspace_bytes(t->grid), st);
    if (backend == SP_KNN_HIERARCHY) {
        if ((rc = build_hierarchy(t, st)) != SP_OK) return rc;
        return own ? sp_bvh_self_knn(t->bvh, k, idx_out, d2_out, st)
                   : sp_bvh_search(t->bvh, queries, nq, k, transT, transT_on_device, idx_out, d2_out, st);
    }
    if ((rc = build_host_tree(t, st)) != SP_OK) return rc;
    return sp_kdtree_search(t->kd, queries, nq, k, transT, transT_on_device, idx_out, d2_out, st);
}

extern "C" int sp_knn_tree_radius_search(sp_knn_tree* t, const float* queries, size_t nq, size_t max_k, float radius,
                                         const float* transT, int transT_on_device, int32_t* idx_out, float* d2_out,
                                         void* stream) {
    if (!t) return SP_ERR_INVALID_ARGUMENT;
    if (max_k > 100) {
        sp_set_error("[KDTree::radius_search_async] `max_k` is too large. not support.");
        return SP_ERR_RUNTIME;
    }
    if (nq == 0 || max_k == 0) return SP_OK;
    hipStream_t st = sp::as_stream(stream);
    t->streams.note(st);
    int rc;
    if (on_hierarchy(t) && max_k <= kHierarchyMaxK) {
        if ((rc = build_hierarchy(t, st)) != SP_OK) return rc;
        return sp_bvh_radius_search(t->bvh, queries, nq, max_k, radius, transT, transT_on_device, idx_out, d2_out, st);
    }
    if ((rc = build_host_tree(t, st)) != SP_OK) return rc;
    return sp_kdtree_radius_search(t->kd, queries, nq, max_k, radius, transT, transT_on_device, idx_out, d2_out, st);
}

extern "C" int sp_knn_tree_remove_by_flags(sp_knn_tree* t, const uint8_t* flags, const int32_t* new_indices, size_t n,
                                           void* stream) {
    if (!t) return SP_ERR_INVALID_ARGUMENT;
    hipStream_t st = sp::as_stream(stream);
    t->streams.note(st);
    // every structure that exists, or will: from now on they must agree
    int rc = t->n >= kDeviceBuildMinPoints ? build_hierarchy(t, st) : SP_OK;
    if (rc == SP_OK && t->bvh) rc = sp_bvh_remove_by_flags(t->bvh, flags, new_indices, n, st);
    if (rc == SP_OK && t->kd) rc = sp_kdtree_remove_by_flags(t->kd, flags, new_indices, n, st);
    hipError_t e = hipSuccess;
    if (rc == SP_OK && !t->kd) {
        Removal r{std::vector<int32_t>(n), std::vector<uint8_t>(n)};
        e = hipMemcpyAsync(r.indices.data(), new_indices, n * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(r.flags.data(), flags, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) t->removals.push_back(std::move(r));
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (rc == SP_OK && e != hipSuccess) rc = hip_fail(e);
    if (rc != SP_OK) return rc;
    t->pristine = false;  // the points carry other indices now: no grid, no own-cloud or brute-force shortcut
    drop_grid(t);
    t->grid_tried = true;
    return SP_OK;
}

extern "C" int sp_knn_tree_set_reference_order(sp_knn_tree* t, int enable) {
    if (!t) return SP_ERR_INVALID_ARGUMENT;
    t->reference_order = enable != 0;
    return SP_OK;
}

extern "C" int sp_knn_tree_info(const sp_knn_tree* t, int what, uint64_t* out) {
    if (!t || !out || what < SP_KNN_TREE_SIZE || what > SP_KNN_TREE_GRID_BUILT) return SP_ERR_INVALID_ARGUMENT;
    const uint64_t v[] = {t->n, t->pristine, t->bvh != nullptr, t->grid != nullptr};
    *out = v[what];
    return SP_OK;
}
