// sycl_points facade for MI355X — KNN layer.
//   algorithms/knn/result.hpp     : KNNResult
//   algorithms/knn/knn.hpp        : KNNBase (the operator boundary Registration::align sits on)
//   algorithms/knn/bruteforce.hpp : knn_search_bruteforce
//   algorithms/knn/kdtree.hpp     : KDTree (host build with the reference's split rule, device search)
//   algorithms/knn/octree.hpp     : Octree (device build, device search, k <= 100)
//   + GridKNN: an MI355X-native KNNBase (device-built uniform grid), no counterpart file in the reference.
#pragma once
#include <atomic>
#include "core.hpp"

namespace sycl_points {
namespace algorithms {

namespace filter {
constexpr uint8_t REMOVE_FLAG = 0;   // common/filter_by_flags.hpp:11-12
constexpr uint8_t INCLUDE_FLAG = 1;
}  // namespace filter

namespace knn {

/// algorithms/knn/result.hpp:12-34
struct KNNResult {
    using Ptr = std::shared_ptr<KNNResult>;
    shared_vector_ptr<int32_t> indices = nullptr;
    shared_vector_ptr<float> distances = nullptr;
    size_t query_size = 0;
    size_t k = 0;

    /// result.hpp:20-27: query_size x k entries of -1 / FLT_MAX. They are put there by a device fill, not by a host vector
    /// (shared_vector::resize_on_device); `fill = false` when a search that writes every entry follows at once.
    void allocate(const sycl_utils::DeviceQueue& queue, size_t query_size_ = 0, size_t k_ = 0, bool fill = true) {
        query_size = query_size_;
        k = k_;
        indices = std::make_shared<shared_vector<int32_t>>(queue);
        distances = std::make_shared<shared_vector<float>>(queue);
        const uint32_t minus_one = 0xffffffffu, flt_max = 0x7f7fffffu;
        indices->resize_on_device(query_size * k, fill ? &minus_one : nullptr);
        distances->resize_on_device(query_size * k, fill ? &flt_max : nullptr);
    }
    void resize(size_t query_size_ = 0, size_t k_ = 0) {
        query_size = query_size_;
        k = k_;
        indices->resize(query_size * k);
        distances->resize(query_size * k);
    }
};

/// algorithms/knn/knn.hpp:14-61 — same virtual interface; `depends` is kept for source compatibility (all work is
/// enqueued in order on the cloud's stream, so dependencies are implicit).
class KNNBase {
public:
    virtual ~KNNBase() = default;
    virtual sycl_utils::events knn_search_async(const PointCloudShared& queries, const size_t k, KNNResult& result,
                                                const std::vector<sycl_utils::event>& depends = {},
                                                const TransformMatrix& transT = TransformMatrix::Identity()) const = 0;

    KNNResult knn_search(const PointCloudShared& queries, const size_t k, const std::vector<sycl_utils::event>& depends = {},
                         const TransformMatrix& transT = TransformMatrix::Identity()) const {
        KNNResult result;
        knn_search_async(queries, k, result, depends, transT).wait_and_throw();
        return result;
    }
    sycl_utils::events nearest_neighbor_search_async(const PointCloudShared& queries, KNNResult& result,
                                                     const std::vector<sycl_utils::event>& depends = {},
                                                     const TransformMatrix& transT = TransformMatrix::Identity()) const {
        return knn_search_async(queries, 1, result, depends, transT);
    }
    void nearest_neighbor_search(const PointCloudShared& queries, KNNResult& result,
                                 const std::vector<sycl_utils::event>& depends = {},
                                 const TransformMatrix& transT = TransformMatrix::Identity()) const {
        nearest_neighbor_search_async(queries, result, depends, transT).wait_and_throw();
    }
};

namespace detail {
inline void prepare_result(const sycl_utils::DeviceQueue& q, KNNResult& r, size_t nq, size_t k) {
    // kdtree.hpp:446-450; every search kernel writes all nq x k entries (padding included): no fill, no host storage
    if (r.indices == nullptr || r.distances == nullptr) {
        r.allocate(q, nq, k, false);
    } else {
        r.query_size = nq;
        r.k = k;
        r.indices->resize_on_device(nq * k);
        r.distances->resize_on_device(nq * k);
    }
}
}  // namespace detail

/// algorithms/knn/bruteforce.hpp:24-96 (synchronous, like the reference)
inline KNNResult knn_search_bruteforce(const sycl_utils::DeviceQueue& queue, const PointCloudShared& queries,
                                       const PointCloudShared& targets, const size_t k) {
    const size_t nq = queries.size(), nt = targets.size();
    KNNResult result;
    result.allocate(queue, nq, k);
    if (nq == 0) return result;
    const size_t ws_bytes = sp_knn_bruteforce_workspace_bytes(nq, nt, k);
    void* ws = nullptr;
    size_t ws_got = 0;
    if (ws_bytes) ws = sycl_points::detail::DeviceBufferCache::acquire(ws_bytes, &ws_got, queue.stream());  // (no hipMalloc / hipFree per call)
    const int rc = sp_knn_bruteforce(queries.points_device(), nq, targets.points_device(), nt, k,
                                     result.indices->device_data_for_write(nq * k),
                                     result.distances->device_data_for_write(nq * k), ws, ws_bytes, queue.stream());
    if (rc == SP_OK) queue.wait();
    if (ws) sycl_points::detail::DeviceBufferCache::release(ws, ws_got, queue.stream(), rc == SP_OK);
    throw_on_error(rc);
    return result;
}

/// MI355X-native KNNBase for clouds of any density profile: a bounding-volume hierarchy over the Morton-sorted points, built
/// entirely on the device (sp_bvh_*, csrc/bvh.hip). Exact kNN, k <= 32, bit-identical to knn_search_bruteforce.
class BVH : public KNNBase {
public:
    using Ptr = std::shared_ptr<BVH>;
    sycl_utils::DeviceQueue queue;

    explicit BVH(const sycl_utils::DeviceQueue& q) : queue(q) {}
    ~BVH() override { if (bvh_) sp_bvh_destroy(bvh_); }
    BVH(const BVH&) = delete;
    BVH& operator=(const BVH&) = delete;

    static Ptr build(const sycl_utils::DeviceQueue& q, const PointContainerShared& points) {
        auto t = std::make_shared<BVH>(q);
        throw_on_error(sp_bvh_create(reinterpret_cast<const float*>(points.device_data()), points.size(), q.stream(), &t->bvh_));
        return t;
    }
    static Ptr build(const sycl_utils::DeviceQueue& q, const PointCloudShared& cloud) { return build(q, *cloud.points); }
    const sp_bvh* handle() const { return bvh_; }
    size_t size() const { return sp_bvh_size(bvh_); }

    sycl_utils::events knn_search_async(const PointCloudShared& queries, const size_t k, KNNResult& result,
                                        const std::vector<sycl_utils::event>& = {},
                                        const TransformMatrix& transT = TransformMatrix::Identity()) const override {
        const size_t nq = queries.size();
        if (k > 32) throw std::runtime_error("[BVH::knn_search_async] `k` is too large (max 32).");
        detail::prepare_result(queue, result, nq, nq ? k : 0);
        if (nq == 0) return sycl_utils::events();
        throw_on_error(sp_bvh_search(bvh_, queries.points_device(), nq, k, transT.data(), 0,
                                     result.indices->device_data_for_write(nq * k),
                                     result.distances->device_data_for_write(nq * k), queue.stream()));
        return sycl_utils::events(queue.stream());
    }
    /// The cloud's own points as queries, walked in tree order (row i = neighbours of point i, itself first).
    KNNResult self_knn(const size_t k) const {
        const size_t n = size();
        if (k > 32) throw std::runtime_error("[BVH::self_knn] `k` is too large (max 32).");
        KNNResult result;
        result.allocate(queue, n, n ? k : 0);
        if (n == 0) return result;
        throw_on_error(sp_bvh_self_knn(bvh_, k, result.indices->device_data_for_write(n * k),
                                       result.distances->device_data_for_write(n * k), queue.stream()));
        queue.wait();
        return result;
    }

private:
    sp_bvh* bvh_ = nullptr;
};

/// algorithms/knn/kdtree.hpp:142-766, over the library's sp_knn_tree (csrc/knn_tree.hip), which is also
/// sycl_points_amd.api.KDTree(accelerate=True). The reference builds its tree on the host (nth_element: 30 ms per 1M points here,
/// 16 threads) and its callers rebuild it every frame (pipeline/submapping.hpp:197, pipeline/pointcloud_processing.hpp:64).
/// From 1024 points build() copies the points and knn_search answers from the device's own hierarchy (BVH above), a grid on the
/// tree's own cloud or the exact brute-force search — the same neighbours; only the order inside a group of exactly equal
/// distances differs (lowest index first instead of first visited). k > 32 and set_reference_tie_order(true) use the
/// reference-topology tree, built when first needed.
class KDTree : public KNNBase {
public:
    using Ptr = std::shared_ptr<KDTree>;
    sycl_utils::DeviceQueue queue;

    explicit KDTree(const sycl_utils::DeviceQueue& q) : queue(q) {}
    ~KDTree() override { sp_knn_tree_destroy(tree_); }
    KDTree(const KDTree&) = delete;
    KDTree& operator=(const KDTree&) = delete;

    static Ptr build(const sycl_utils::DeviceQueue& q, const PointContainerShared& points, size_t leaf_threshold = 16) {
        auto t = std::make_shared<KDTree>(q);
        throw_on_error(sp_knn_tree_create(reinterpret_cast<const float*>(points.device_data()), points.size(), leaf_threshold,
                                          q.stream(), &t->tree_));
        static std::atomic<uint64_t> next_id{1};
        t->id_ = next_id.fetch_add(1);
        return t;
    }
    static Ptr build(const sycl_utils::DeviceQueue& q, const PointCloudShared& cloud, size_t leaf_threshold = 16) {
        auto t = build(q, *cloud.points, leaf_threshold);
        t->built_on_ = cloud.points;  // (shared ownership: the address cannot be handed to another container meanwhile)
        t->built_generation_ = cloud.points->generation();
        return t;
    }
    /// MI355X extension: answer knn_search from the reference-topology tree (first-visited tie order, host build) always.
    void set_reference_tie_order(bool v) { throw_on_error(sp_knn_tree_set_reference_order(tree_, v)); }
    /// MI355X extension: which structure knn_search_async(queries, k, ..., transT) answers from — the library's decision itself
    /// (sp_knn_tree_backend), without searching.
    enum class Backend { HostTree = SP_KNN_HOST_TREE, Hierarchy = SP_KNN_HIERARCHY, Grid = SP_KNN_GRID, BruteForce = SP_KNN_BRUTE_FORCE };
    Backend backend_for(const PointCloudShared& queries, size_t k, const TransformMatrix& transT = TransformMatrix::Identity()) const {
        int b = SP_KNN_HOST_TREE;
        throw_on_error(sp_knn_tree_backend(tree_, queries.size(), k, transT.data(), 0, own_cloud(queries), queue.stream(), &b));
        return Backend(b);
    }

    sycl_utils::events knn_search_async(const PointCloudShared& queries, const size_t k, KNNResult& result,
                                        const std::vector<sycl_utils::event>& = {},
                                        const TransformMatrix& transT = TransformMatrix::Identity()) const override {
        const size_t nq = queries.size();
        detail::prepare_result(queue, result, nq, nq ? k : 0);
        throw_on_error(sp_knn_tree_search(tree_, queries.points_device(), nq, k, transT.data(), 0, own_cloud(queries),
                                          result.indices->device_data_for_write(nq * k),
                                          result.distances->device_data_for_write(nq * k), queue.stream()));
        return sycl_utils::events(queue.stream());
    }
    sycl_utils::events radius_search_async(const PointCloudShared& queries, const size_t max_k, const float radius,
                                           KNNResult& result, const std::vector<sycl_utils::event>& = {},
                                           const TransformMatrix& transT = TransformMatrix::Identity()) const {
        const size_t nq = max_k ? queries.size() : 0;
        detail::prepare_result(queue, result, nq, nq ? max_k : 0);
        throw_on_error(sp_knn_tree_radius_search(tree_, nq ? queries.points_device() : nullptr, nq, max_k, radius, transT.data(), 0,
                                                 result.indices->device_data_for_write(nq * max_k),
                                                 result.distances->device_data_for_write(nq * max_k), queue.stream()));
        return sycl_utils::events(queue.stream());
    }
    void remove_nodes_by_flags(const shared_vector<uint8_t>& flags, const shared_vector<int32_t>& indices) {
        if (flags.size() != indices.size())
            throw std::runtime_error("[KDTree::remove_nodes_by_flags_impl] flags and indices must have the same size.");
        throw_on_error(sp_knn_tree_remove_by_flags(tree_, flags.device_data(), indices.device_data(), flags.size(), queue.stream()));
    }
    /// Identity of the built tree (unique per build), its point count, and whether no node was ever removed — what
    /// Registration::align needs to decide that a GridKNN on the same cloud answers the same nearest-neighbour queries.
    uint64_t id() const { return id_; }
    size_t size() const { return size_t(info(SP_KNN_TREE_SIZE)); }
    bool pristine() const { return info(SP_KNN_TREE_PRISTINE) != 0; }

private:
    uint64_t info(int what) const { uint64_t v = 0; throw_on_error(sp_knn_tree_info(tree_, what, &v)); return v; }
    /// The queries are the cloud the tree was built on, unchanged since (the library adds: nothing removed, no transform).
    int own_cloud(const PointCloudShared& queries) const {
        return built_on_ != nullptr && queries.points == built_on_ && queries.points->generation() == built_generation_ &&
               queries.size() == size();
    }
    sp_knn_tree* tree_ = nullptr;
    uint64_t id_ = 0;
    std::shared_ptr<PointContainerShared> built_on_;  // the cloud's point container at build(), and its generation then
    uint64_t built_generation_ = 0;
};

/// algorithms/knn/octree.hpp:27-844 over the library's device-built octree (sp_octree_*, csrc/octree.hip): the reference's
/// constructor, build, knn_search_async, accessors and remove_nodes_by_flags. Exact kNN for k <= 100; rows are bit-identical to
/// knn_search_bruteforce (ties to the lowest index, where the reference's heap leaves them to its traversal).
class Octree : public KNNBase {
public:
    using Ptr = std::shared_ptr<Octree>;

    /// octree.hpp:193-210: an empty tree, ready to be built
    Octree(const sycl_utils::DeviceQueue& queue, float resolution, size_t max_points_per_node)
        : queue_(queue), resolution_(resolution), max_points_per_node_(max_points_per_node) {
        throw_on_error(sp_octree_create(nullptr, 0, resolution, max_points_per_node, queue.stream(), &tree_));
    }
    ~Octree() override { sp_octree_destroy(tree_); }
    Octree(const Octree&) = delete;
    Octree& operator=(const Octree&) = delete;

    /// octree.hpp:581-596
    static Ptr build(const sycl_utils::DeviceQueue& queue, const PointCloudShared& points, float resolution,
                     size_t max_points_per_node = 32) {
        auto t = std::make_shared<Octree>(queue, resolution, max_points_per_node);
        if (!points.points) throw std::runtime_error("[Octree::build_from_cloud] Point cloud is not initialised");
        sp_octree* built = nullptr;
        throw_on_error(sp_octree_create(points.points_device(), points.size(), resolution, max_points_per_node, queue.stream(), &built));
        sp_octree_destroy(t->tree_);
        t->tree_ = built;
        return t;
    }
    const sp_octree* handle() const { return tree_; }

    /// octree.hpp:599-630
    sycl_utils::events knn_search_async(const PointCloudShared& queries, const size_t k, KNNResult& result,
                                        const std::vector<sycl_utils::event>& = {},
                                        const TransformMatrix& transT = TransformMatrix::Identity()) const override {
        const size_t nq = queries.size();
        if (k > 100) throw std::runtime_error("[Octree::knn_search_async] Requested neighbor count exceeds the supported maximum");
        detail::prepare_result(queue_, result, nq, k);
        if (nq == 0 || k == 0) return sycl_utils::events();
        throw_on_error(sp_octree_search(tree_, queries.points_device(), nq, k, transT.data(), 0,
                                        result.indices->device_data_for_write(nq * k),
                                        result.distances->device_data_for_write(nq * k), queue_.stream()));
        return sycl_utils::events(queue_.stream());
    }

    [[nodiscard]] float resolution() const { return resolution_; }
    [[nodiscard]] size_t max_points_per_node() const { return max_points_per_node_; }
    [[nodiscard]] size_t size() const { return sp_octree_size(tree_); }

    /// octree.hpp:276-380
    void remove_nodes_by_flags(const shared_vector<uint8_t>& flags, const shared_vector<int32_t>& indices) {
        if (flags.size() != indices.size())
            throw std::runtime_error("[Octree::remove_nodes_by_flags] flags and indices must have the same size");
        throw_on_error(sp_octree_remove_by_flags(tree_, flags.device_data(), indices.device_data(), flags.size(), queue_.stream()));
    }

private:
    sycl_utils::DeviceQueue queue_;
    float resolution_;
    size_t max_points_per_node_;
    sp_octree* tree_ = nullptr;
};

/// MI355X-native KNNBase: exact kNN on a device-built uniform grid (sp_grid_*). Bit-identical to
/// knn_search_bruteforce. Registration::align recognises it and takes the fused NN + linearise path.
class GridKNN : public KNNBase {
public:
    using Ptr = std::shared_ptr<GridKNN>;
    sycl_utils::DeviceQueue queue;

    explicit GridKNN(const sycl_utils::DeviceQueue& q) : queue(q) {}
    ~GridKNN() override { if (grid_) sp_grid_destroy(grid_); }
    GridKNN(const GridKNN&) = delete;
    GridKNN& operator=(const GridKNN&) = delete;

    static Ptr build(const sycl_utils::DeviceQueue& q, const PointCloudShared& cloud, float points_per_cell = 0.5f,
                     float cell_size = 0.0f) {
        auto g = std::make_shared<GridKNN>(q);
        // (a cloud whose producer left a bounding box behind — voxel downsampling does: the build then needs no box of its own,
        // i.e. no kernel, no read-back and no wait before it can size its cell table)
        float box[6];
        const float* const pts = cloud.points_device();  // (before the look-up: an upload does not change the generation)
        if (sycl_points::detail::BoundsHints::get(cloud.points->generation(), box))
            throw_on_error(sp_grid_create_bounded(pts, cloud.size(), box, cell_size, points_per_cell, q.stream(), &g->grid_));
        else
            throw_on_error(sp_grid_create(pts, cloud.size(), cell_size, points_per_cell, q.stream(), &g->grid_));
        g->id_ = next_grid_id();
        return g;
    }
    static uint64_t next_grid_id() {
        static std::atomic<uint64_t> next_id{1};
        return next_id.fetch_add(1);
    }
    /// Cell size steered by the measured occupancy instead of the bounding-box volume (sp_grid_create_adaptive): for clouds of
    /// surfaces — what Registration::align builds when it stands in for the caller's KDTree.
    static Ptr build_adaptive(const sycl_utils::DeviceQueue& q, const PointCloudShared& cloud, float points_per_cell = 0.5f) {
        auto g = std::make_shared<GridKNN>(q);
        throw_on_error(sp_grid_create_adaptive(cloud.points_device(), cloud.size(), points_per_cell, q.stream(), &g->grid_));
        g->id_ = next_grid_id();
        return g;
    }
    const sp_grid* handle() const { return grid_; }
    uint64_t id() const { return id_; }  ///< unique per build (a handle address can be reused after destruction)
    size_t size() const { return sp_grid_size(grid_); }
    float cell_size() const { return sp_grid_cell_size(grid_); }

    sycl_utils::events knn_search_async(const PointCloudShared& queries, const size_t k, KNNResult& result,
                                        const std::vector<sycl_utils::event>& = {},
                                        const TransformMatrix& transT = TransformMatrix::Identity()) const override {
        const size_t nq = queries.size();
        if (k > 20) throw std::runtime_error("[GridKNN::knn_search_async] `k` is too large (max 20).");
        detail::prepare_result(queue, result, nq, nq ? k : 0);
        if (nq == 0) return sycl_utils::events();
        throw_on_error(sp_grid_search(grid_, queries.points_device(), nq, k, transT.data(), 0,
                                      result.indices->device_data_for_write(nq * k),
                                      result.distances->device_data_for_write(nq * k), queue.stream()));
        return sycl_utils::events(queue.stream());
    }

    /// The grid's counterpart of KDTree::radius_search_async (kdtree.hpp:251-280): the max_k nearest within `radius`.
    sycl_utils::events radius_search_async(const PointCloudShared& queries, const size_t max_k, const float radius,
                                           KNNResult& result, const std::vector<sycl_utils::event>& = {},
                                           const TransformMatrix& transT = TransformMatrix::Identity()) const {
        const size_t nq = queries.size();
        if (max_k > 20) throw std::runtime_error("[GridKNN::radius_search_async] `max_k` is too large (max 20).");
        detail::prepare_result(queue, result, (nq && max_k) ? nq : 0, (nq && max_k) ? max_k : 0);
        if (nq == 0 || max_k == 0) return sycl_utils::events();
        throw_on_error(sp_grid_radius_search(grid_, queries.points_device(), nq, max_k, radius, transT.data(), 0,
                                             result.indices->device_data_for_write(nq * max_k),
                                             result.distances->device_data_for_write(nq * max_k), queue.stream()));
        return sycl_utils::events(queue.stream());
    }

    /// The grid's counterpart of KDTree::remove_nodes_by_flags (kdtree.hpp:282-284): flags 1 = keep, kept point p is
    /// relabelled indices[p]. The grid gets a new identity (Registration re-prepares its target on the next align()).
    void remove_nodes_by_flags(const shared_vector<uint8_t>& flags, const shared_vector<int32_t>& indices) {
        if (flags.size() != indices.size())
            throw std::runtime_error("[GridKNN::remove_nodes_by_flags] flags and indices must have the same size.");
        throw_on_error(sp_grid_remove_by_flags(grid_, flags.device_data(), indices.device_data(), flags.size(), queue.stream()));
        static std::atomic<uint64_t> next_removed_id{1ull << 40};
        id_ = next_removed_id.fetch_add(1);
    }

private:
    sp_grid* grid_ = nullptr;
    uint64_t id_ = 0;
};

}  // namespace knn
}  // namespace algorithms
}  // namespace sycl_points
