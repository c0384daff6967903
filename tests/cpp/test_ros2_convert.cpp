// C++ tests of ros2::fromROS2msg / ros2::toROS2msg / ros2::EnhancedReflectivityCorrector, included through the reference's paths
// only and run on ros2::compat's stand-in message types (no ROS needed). Built and run by tests/test_gpu_pointcloud2.py on a GPU
// box: test_ros2_convert <golden dir>; exit code 0 = all checks passed.
//   1. both fromROS2msg overloads on an Ouster-like message against a host loop over the same bytes, bit for bit
//   2. a larger msg_buffer is reused as it is; a smaller one grows
//   3. the empty message; a big-endian message; a message without y
//   4. toROS2msg: field offsets where the data is, and fromROS2msg reads the message back
//   5. EnhancedReflectivityCorrector::apply with and without the shared buffer: identical intensities and ring means
//   6. a scan converted this way through LiDAROdometryPipeline::process with enhanced_reflectivity.enable set
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sycl_points/io/point_cloud_reader.hpp"
#include "sycl_points/pipeline/lidar_odometry.hpp"
#include "sycl_points/ros2/convert.hpp"
#include "sycl_points/ros2/enhanced_reflectivity.hpp"

using namespace sycl_points;
namespace lo = sycl_points::pipeline::lidar_odometry;
using Msg = ros2::compat::PointCloud2;
using Field = ros2::compat::PointField;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); std::fflush(stdout); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); std::fflush(stdout); } while (0)

static PointCloudCPU g_scan;

template <class T>
static void put(Msg& m, size_t i, uint32_t offset, T v) { std::memcpy(&m.data[i * m.point_step + offset], &v, sizeof(T)); }
template <class T>
static T get(const Msg& m, size_t i, uint32_t offset) { T v; std::memcpy(&v, &m.data[i * m.point_step + offset], sizeof(T)); return v; }
static bool same_bits(const float* a, const float* b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

/// An Ouster-like message of the golden scan's points: 37-byte records (unaligned everywhere), xyz f32 @0/4/8, intensity f32 @13,
/// t u32 @17 (ns), ring u16 @21, ambient u16 @23, reflectivity u16 @25, rgba u32 @27, six pad bytes
static Msg ouster_like(size_t n) {
    Msg m;
    m.header.stamp.sec = 1700000000;
    m.header.stamp.nanosec = 250000000u;
    m.height = 1;
    m.width = static_cast<uint32_t>(n);
    m.point_step = 37;
    m.row_step = static_cast<uint32_t>(37 * n);
    auto field = [&](const char* name, uint32_t offset, uint8_t type) {
        Field f;
        f.name = name; f.offset = offset; f.datatype = type; f.count = 1;
        m.fields.push_back(f);
    };
    field("x", 0, Field::FLOAT32); field("y", 4, Field::FLOAT32); field("z", 8, Field::FLOAT32);
    field("intensity", 13, Field::FLOAT32); field("t", 17, Field::UINT32); field("ring", 21, Field::UINT16);
    field("ambient", 23, Field::UINT16); field("reflectivity", 25, Field::UINT16); field("rgba", 27, Field::UINT32);
    m.data.assign(37 * n, 0xAB);
    for (size_t i = 0; i < n; ++i) {
        const PointType& p = (*g_scan.points)[i % g_scan.size()];
        put<float>(m, i, 0, p[0]); put<float>(m, i, 4, p[1]); put<float>(m, i, 8, p[2]);
        put<float>(m, i, 13, float(20 + (i * 7) % 180));
        put<uint32_t>(m, i, 17, uint32_t((i * 100000000ull) / n));  // 0 .. 100 ms
        put<uint16_t>(m, i, 21, uint16_t(i % 64));
        put<uint16_t>(m, i, 23, uint16_t(100 + (i * 13) % 900));
        put<uint16_t>(m, i, 25, uint16_t((i * 31) % 65536));
        put<uint32_t>(m, i, 27, uint32_t(i * 2654435761u));
    }
    return m;
}

static void test_from_overloads() {
    sycl_utils::DeviceQueue q(0);
    const size_t n = 3 * SP_PC2_BLOCK_POINTS + 7;
    const Msg m = ouster_like(n);
    shared_vector_ptr<uint8_t> buffer = std::make_shared<shared_vector<uint8_t>>(q);
    PointCloudShared::Ptr cloud;
    CHECK(ros2::fromROS2msg(q, m, cloud, buffer));
    CHECK(cloud != nullptr && cloud->size() == n && cloud->has_rgb() && cloud->has_intensity() && cloud->has_timestamps());
    CHECK(!cloud->has_cov() && !cloud->has_normal());
    CHECK(buffer->size() == m.data.size());
    bool pts_ok = true, rgb_ok = true, int_ok = true, ts_ok = true;
    double max_ms = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const float want[4] = {get<float>(m, i, 0), get<float>(m, i, 4), get<float>(m, i, 8), 1.0f};
        pts_ok = pts_ok && same_bits(std::as_const(*cloud->points)[i].data(), want, 4);
        const uint32_t c = get<uint32_t>(m, i, 27);
        const float col[4] = {float(c & 0xff) / 255.0f, float((c >> 8) & 0xff) / 255.0f, float((c >> 16) & 0xff) / 255.0f, float(c >> 24) / 255.0f};
        rgb_ok = rgb_ok && same_bits(std::as_const(*cloud->rgb)[i].data(), col, 4);
        int_ok = int_ok && std::as_const(*cloud->intensities)[i] == float(get<uint16_t>(m, i, 25));  // reflectivity takes over
        const float off = float(get<uint32_t>(m, i, 17)) * 1e-6f;
        ts_ok = ts_ok && std::as_const(*cloud->timestamp_offsets)[i] == off;
        max_ms = std::max(max_ms, double(off));
    }
    CHECK(pts_ok); CHECK(rgb_ok); CHECK(int_ok); CHECK(ts_ok);
    const double start = 1700000000.0 * 1000.0 + 250000000.0 * 1e-6;
    CHECK(cloud->start_time_ms == start && cloud->end_time_ms == start + max_ms);
    // the switches, and the overload that returns the cloud
    const auto plain = ros2::fromROS2msg(q, m, buffer, false, true, false);
    CHECK(plain != nullptr && !plain->has_rgb() && plain->has_intensity());
    CHECK(std::as_const(*plain->intensities)[5] == get<float>(m, 5, 13));
    const auto bare = ros2::fromROS2msg(q, m, buffer, false, false);
    CHECK(bare != nullptr && !bare->has_rgb() && !bare->has_intensity() && bare->has_timestamps());
    // a cloud bound to another queue is replaced, one bound to this queue is kept
    PointCloudShared* before = cloud.get();
    CHECK(ros2::fromROS2msg(q, m, cloud, buffer) && cloud.get() == before);
    sycl_utils::DeviceQueue q2(0);
    CHECK(ros2::fromROS2msg(q2, m, cloud, buffer) && cloud.get() != before && cloud->queue.ptr == q2.ptr);
}

static void test_buffer_reuse() {
    sycl_utils::DeviceQueue q(0);
    const Msg big = ouster_like(1000), small = ouster_like(100);
    shared_vector_ptr<uint8_t> buffer = std::make_shared<shared_vector<uint8_t>>(q);
    PointCloudShared::Ptr cloud;
    CHECK(ros2::fromROS2msg(q, small, cloud, buffer) && buffer->size() == small.data.size());
    CHECK(ros2::fromROS2msg(q, big, cloud, buffer) && buffer->size() == big.data.size() && cloud->size() == 1000);  // grows
    const uint8_t* dev = buffer->device_data();
    CHECK(ros2::fromROS2msg(q, small, cloud, buffer) && cloud->size() == 100);
    CHECK(buffer->size() == big.data.size() && buffer->device_data() == dev);  // the larger buffer as it is
    CHECK(std::as_const(*cloud->points)[99][0] == get<float>(small, 99, 0));
    shared_vector_ptr<uint8_t> none;  // a null buffer is created
    CHECK(ros2::fromROS2msg(q, small, cloud, none) && none != nullptr && none->size() == small.data.size());
}

static void test_refusals() {
    sycl_utils::DeviceQueue q(0);
    shared_vector_ptr<uint8_t> buffer = std::make_shared<shared_vector<uint8_t>>(q);
    PointCloudShared::Ptr cloud;
    CHECK(ros2::fromROS2msg(q, ouster_like(50), cloud, buffer) && cloud->size() == 50);
    Msg empty = ouster_like(0);
    CHECK(ros2::fromROS2msg(q, empty, cloud, buffer));  // clears the cloud, true
    CHECK(cloud->size() == 0 && !cloud->has_timestamps() && cloud->start_time_ms == 0.0);
    Msg be = ouster_like(50);
    be.is_bigendian = true;
    PointCloudShared::Ptr untouched;
    CHECK(!ros2::fromROS2msg(q, be, untouched, buffer) && untouched == nullptr);
    Msg no_y = ouster_like(50);
    no_y.fields.erase(no_y.fields.begin() + 1);
    CHECK(!ros2::fromROS2msg(q, no_y, untouched, buffer) && untouched == nullptr);
    Msg past = ouster_like(50);
    past.fields[4].offset = 35;  // a u32 at 35 of 37 bytes
    bool threw = false;
    try { ros2::fromROS2msg(q, past, untouched, buffer); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
}

static void test_to_msg() {
    sycl_utils::DeviceQueue q(0);
    shared_vector_ptr<uint8_t> buffer;
    const size_t n = SP_PC2_BLOCK_POINTS + 3;
    const Msg m = ouster_like(n);
    const auto cloud = ros2::fromROS2msg(q, m, buffer);
    const auto out = ros2::toROS2msg(*cloud, m.header);
    CHECK(out->point_step == 32 && out->width == n && out->height == 1 && out->row_step == 32 * n && out->data.size() == 32 * n);
    CHECK(!out->is_bigendian && out->is_dense && out->header.stamp.sec == m.header.stamp.sec);
    CHECK(out->fields.size() == 6);
    const char* names[6] = {"x", "y", "z", "rgb", "intensity", "timestamp"};
    const uint32_t offsets[6] = {0, 4, 8, 16, 20, 24};  // the reference declares the timestamp at 28 and writes it at 24
    const uint8_t types[6] = {Field::FLOAT32, Field::FLOAT32, Field::FLOAT32, Field::UINT32, Field::FLOAT32, Field::FLOAT64};
    for (size_t f = 0; f < 6 && f < out->fields.size(); ++f)
        CHECK(out->fields[f].name == names[f] && out->fields[f].offset == offsets[f] && out->fields[f].datatype == types[f] && out->fields[f].count == 1);
    bool data_ok = true;
    for (size_t i = 0; i < n; ++i) {
        data_ok = data_ok && same_bits(reinterpret_cast<const float*>(&out->data[32 * i]), std::as_const(*cloud->points)[i].data(), 4);
        data_ok = data_ok && get<uint32_t>(*out, i, 16) == get<uint32_t>(m, i, 27);  // byte / 255 * 255 truncates back to the byte
        data_ok = data_ok && get<float>(*out, i, 20) == std::as_const(*cloud->intensities)[i];
        data_ok = data_ok && get<double>(*out, i, 24) == (cloud->start_time_ms + double(std::as_const(*cloud->timestamp_offsets)[i])) * 1e-3;
    }
    CHECK(data_ok);
    const auto back = ros2::fromROS2msg(q, *out, buffer);  // works because of the offset
    CHECK(back != nullptr && back->size() == n && back->has_rgb() && back->has_intensity() && back->has_timestamps());
    bool back_ok = true;
    for (size_t i = 0; i < n; ++i) {
        back_ok = back_ok && same_bits(std::as_const(*back->points)[i].data(), std::as_const(*cloud->points)[i].data(), 4);
        back_ok = back_ok && same_bits(std::as_const(*back->rgb)[i].data(), std::as_const(*cloud->rgb)[i].data(), 4);
        back_ok = back_ok && std::as_const(*back->intensities)[i] == std::as_const(*cloud->intensities)[i];
        back_ok = back_ok && std::fabs(std::as_const(*back->timestamp_offsets)[i] - std::as_const(*cloud->timestamp_offsets)[i]) < 1e-3f;
    }
    CHECK(back_ok);
    PointCloudShared bare(q);
    bare.points->resize(5, PointType(1.0f, 2.0f, 3.0f, 1.0f));
    const auto small = ros2::toROS2msg(bare, m.header);
    CHECK(small->point_step == 16 && small->fields.size() == 3 && small->data.size() == 80 && get<float>(*small, 4, 8) == 3.0f);
    CHECK(ros2::toROS2msg(PointCloudShared(q), m.header)->data.empty());
}

static void test_reflectivity() {
    sycl_utils::DeviceQueue q(0);
    const size_t n = 5000;
    shared_vector_ptr<uint8_t> buffer;
    ros2::EnhancedReflectivityCorrector own(0.5f), shared(0.5f);
    for (int scan = 0; scan < 2; ++scan) {
        Msg m = ouster_like(n);
        for (size_t i = 0; i < n; ++i) put<uint16_t>(m, i, 23, uint16_t(100 + (i * (13 + scan)) % 900));
        const auto a = ros2::fromROS2msg(q, m, buffer, true, true, false);
        PointCloudShared b(*a);  // deep copy
        CHECK(own.apply(b, m));  // uploads the bytes itself
        CHECK(shared.apply(*a, m, buffer));
        bool same = true, changed = false, in_range = true;
        for (size_t i = 0; i < n; ++i) {
            const float va = std::as_const(*a->intensities)[i], vb = std::as_const(*b.intensities)[i];
            same = same && std::memcmp(&va, &vb, 4) == 0;
            changed = changed || va != get<float>(m, i, 13);
            in_range = in_range && va >= 0.0f && va <= 5.0f;
        }
        CHECK(same); CHECK(changed); CHECK(in_range);
        const auto ra = shared.ring_mean_ref(), rb = own.ring_mean_ref();
        const auto ia = shared.ring_initialized();
        CHECK(std::memcmp(ra.data(), rb.data(), sizeof(float) * ra.size()) == 0);
        CHECK(ra[0] > 0.0f && ra[63] > 0.0f && ra[64] == 0.0f && ia[63] == 1u && ia[64] == 0u);
        CHECK(shared.ring_mean_amb() == own.ring_mean_amb());
    }
    // what apply refuses leaves the cloud alone
    Msg m = ouster_like(100);
    const auto cloud = ros2::fromROS2msg(q, m, buffer, true, true, false);
    ros2::EnhancedReflectivityCorrector fresh;
    Msg no_ambient = m;
    no_ambient.fields.erase(no_ambient.fields.begin() + 6);
    CHECK(!fresh.apply(*cloud, no_ambient) && std::as_const(*cloud->intensities)[7] == get<float>(m, 7, 13));
    Msg ring_f32 = m;
    ring_f32.fields[5].datatype = Field::FLOAT32;
    CHECK(!fresh.apply(*cloud, ring_f32, buffer));
    const auto no_intensity = ros2::fromROS2msg(q, m, buffer, true, false);
    CHECK(!fresh.apply(*no_intensity, m));
    CHECK(fresh.apply(*cloud, m, 2.0f) && std::as_const(*cloud->intensities)[7] <= 2.0f);
}

static void test_pipeline() {
    lo::Parameters P;
    P.imu.enable = false;
    P.scan.enhanced_reflectivity.enable = true;  // (intensity_correction is skipped: the scan arrives corrected)
    lo::LiDAROdometryPipeline pipeline(P);
    const auto q = pipeline.get_device_queue();
    shared_vector_ptr<uint8_t> buffer;
    ros2::EnhancedReflectivityCorrector corrector(P.scan.enhanced_reflectivity.ring_mean_ema_alpha);
    for (int frame = 0; frame < 2; ++frame) {
        Msg m = ouster_like(g_scan.size());
        m.header.stamp.nanosec += 100000000u * frame;
        PointCloudShared::Ptr scan;
        CHECK(ros2::fromROS2msg(*q, m, scan, buffer, false, true, false));
        CHECK(corrector.apply(*scan, m, buffer, P.scan.enhanced_reflectivity.clip_max));
        const auto rc = pipeline.process(scan, 0.1 * frame);
        std::printf("  frame %d: result %d %s\n", frame, int(rc), pipeline.get_error_message().c_str());
        using RT = lo::LiDAROdometryPipeline::ResultType;
        CHECK(rc == (frame == 0 ? RT::first_frame : RT::success));
    }
    const auto odom = pipeline.get_odom();
    float drift = 0.0f;
    for (int r = 0; r < 3; ++r) drift = std::max(drift, std::fabs(odom.matrix()(r, 3)));
    std::printf("  the same scan twice: |translation| = %.3e\n", drift);
    CHECK(drift < 0.05f);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <golden dir>\n", argv[0]); return 2; }
    g_scan = PointCloudReader::readFile(std::string(argv[1]) + "/target.ply");
    if (g_scan.size() == 0) { std::printf("cannot read the golden files in %s\n", argv[1]); return 2; }
    RUN(test_from_overloads);
    RUN(test_buffer_reuse);
    RUN(test_refusals);
    RUN(test_to_msg);
    RUN(test_reflectivity);
    RUN(test_pipeline);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
