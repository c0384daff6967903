// What getting an Ouster-128 frame (131 072 points, 48-byte records) into a PointCloudShared costs, three ways:
//   1. sp_pc2_unpack on the uploaded bytes (device events around back-to-back calls)
//   2. sp_enhanced_reflectivity's three launches (the same)
//   3. ros2::fromROS2msg end to end: upload, unpack, the 8-byte read-back (host clock)
//   4. the baseline, what a caller had to do before ros2/convert.hpp existed: a host loop over the records into a PointCloudCPU,
//      the PointCloudShared constructor, and the upload of its attributes (host clock, ends in a synchronise)
// Prints microseconds per call and, for 1 and 2, the share of the bytes-per-point bound at 6.3 TB/s (the achievable HBM rate).
//
// build: g++ -O2 -std=c++20 -Iinclude -I$ROCM/include -D__HIP_PLATFORM_AMD__ examples/bench_pointcloud2.cpp -o bench_pointcloud2
//            -Lsycl_points_amd/lib -lsycl_points_amd -Wl,-rpath,$PWD/sycl_points_amd/lib -L$ROCM/lib -lamdhip64
// usage: bench_pointcloud2 [--n 131072] [--loops 200] [--warmup 20]
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>

#include "sycl_points/ros2/convert.hpp"
#include "sycl_points/ros2/enhanced_reflectivity.hpp"

using namespace sycl_points;
using Msg = ros2::compat::PointCloud2;
using Field = ros2::compat::PointField;
using Clock = std::chrono::steady_clock;

template <class T>
static void put(Msg& m, size_t i, uint32_t offset, T v) { std::memcpy(&m.data[i * m.point_step + offset], &v, sizeof(T)); }
template <class T>
static T get(const Msg& m, size_t i, uint32_t offset) { T v; std::memcpy(&v, &m.data[i * m.point_step + offset], sizeof(T)); return v; }

/// xyz f32 @0/4/8, intensity f32 @16, t u32 @20, reflectivity u16 @24, ring u16 @26, ambient u16 @28; 48-byte records
static Msg ouster_frame(size_t n) {
    Msg m;
    m.header.stamp.sec = 1700000000;
    m.height = 128;
    m.width = static_cast<uint32_t>(n / 128);
    m.point_step = 48;
    m.row_step = 48 * m.width;
    const char* names[8] = {"x", "y", "z", "intensity", "t", "reflectivity", "ring", "ambient"};
    const uint32_t offsets[8] = {0, 4, 8, 16, 20, 24, 26, 28};
    const uint8_t types[8] = {Field::FLOAT32, Field::FLOAT32, Field::FLOAT32, Field::FLOAT32, Field::UINT32, Field::UINT16, Field::UINT16, Field::UINT16};
    for (int f = 0; f < 8; ++f) {
        Field fd;
        fd.name = names[f]; fd.offset = offsets[f]; fd.datatype = types[f]; fd.count = 1;
        m.fields.push_back(fd);
    }
    m.data.assign(48 * n, 0);
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return float(s >> 8) / float(1 << 24); };
    for (size_t i = 0; i < n; ++i) {
        put<float>(m, i, 0, 60.0f * rnd() - 30.0f); put<float>(m, i, 4, 60.0f * rnd() - 30.0f); put<float>(m, i, 8, 6.0f * rnd() - 2.0f);
        put<float>(m, i, 16, 200.0f * rnd());
        put<uint32_t>(m, i, 20, uint32_t((i * 100000000ull) / n));
        put<uint16_t>(m, i, 24, uint16_t(65535.0f * rnd()));
        put<uint16_t>(m, i, 26, uint16_t(i % 128));
        put<uint16_t>(m, i, 28, uint16_t(100.0f + 900.0f * rnd()));
    }
    return m;
}

template <class F>
static double event_us(hipStream_t st, int warmup, int loops, F&& call) {
    hipEvent_t a, b;
    hip_check(hipEventCreate(&a), "event");
    hip_check(hipEventCreate(&b), "event");
    for (int i = 0; i < warmup; ++i) call();
    hip_check(hipEventRecord(a, st), "event");
    for (int i = 0; i < loops; ++i) call();
    hip_check(hipEventRecord(b, st), "event");
    hip_check(hipEventSynchronize(b), "event");
    float ms = 0.0f;
    hip_check(hipEventElapsedTime(&ms, a, b), "event");
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return 1e3 * double(ms) / loops;
}
template <class F>
static double host_us(int warmup, int loops, F&& call) {  // (call ends in a synchronise)
    for (int i = 0; i < warmup; ++i) call();
    const auto t0 = Clock::now();
    for (int i = 0; i < loops; ++i) call();
    return std::chrono::duration<double, std::micro>(Clock::now() - t0).count() / loops;
}

int main(int argc, char** argv) {
    size_t n = 131072;
    int loops = 200, warmup = 20;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--n") n = std::stoul(argv[i + 1]);
        else if (k == "--loops") loops = std::stoi(argv[i + 1]);
        else if (k == "--warmup") warmup = std::stoi(argv[i + 1]);
    }
    sycl_utils::DeviceQueue q(0);
    const Msg m = ouster_frame(n);
    shared_vector_ptr<uint8_t> buffer;
    PointCloudShared::Ptr cloud;
    if (!ros2::fromROS2msg(q, m, cloud, buffer, true, true, false)) return 1;
    const hipStream_t st = q.stream();

    // 1. the unpack alone, on the bytes already in HBM
    sp_pc2_layout L{};
    L.point_step = 48; L.x_offset = 0; L.y_offset = 4; L.z_offset = 8; L.rgb_offset = -1; L.intensity_offset = 16; L.timestamp_offset = 20;
    L.xyz_type = SP_PC2_FLOAT32; L.intensity_type = SP_PC2_FLOAT32; L.timestamp_type = SP_PC2_UINT32;
    L.start_time_ms = 1700000000.0 * 1000.0;
    shared_vector<double> max_ms(q);
    double* max_dev = max_ms.device_data_for_write(2 + sp_pc2_unpack_workspace_bytes(n) / sizeof(double));
    float* points = reinterpret_cast<float*>(cloud->points->device_data_rw());
    float* inten = cloud->intensities->device_data_rw();
    float* ts = cloud->timestamp_offsets->device_data_rw();
    const uint8_t* data = buffer->device_data();
    const double unpack_us = event_us(st, warmup, loops, [&]() {
        throw_on_error(sp_pc2_unpack(data, m.data.size(), n, &L, points, nullptr, inten, ts, max_dev, max_dev + 2, st));
    });
    const double unpack_bytes = double(n) * (48 + 16 + 4 + 4);

    // 2. the reflectivity correction's three launches
    shared_vector<uint32_t> state(3 * SP_ER_MAX_RINGS, 0u, q);
    shared_vector<uint8_t> ws(q);
    uint8_t* ws_dev = ws.device_data_for_write(sp_enhanced_reflectivity_workspace_bytes(n));
    uint32_t* state_dev = state.device_data_rw();
    const double er_us = event_us(st, warmup, loops, [&]() {
        throw_on_error(sp_enhanced_reflectivity(points, inten, n, data, 48, 26, 0, 28, state_dev, 0.5f, 5.0f, ws_dev, st));
    });
    // launch 1 reads the records, points and intensities; launch 3 reads them again and writes the intensities
    const double er_bytes = double(n) * (2 * (48 + 16 + 4) + 4);

    // 3. fromROS2msg end to end
    const double from_us = host_us(warmup, loops, [&]() { ros2::fromROS2msg(q, m, cloud, buffer, true, true, false); });

    // 4. the baseline: host unpack, PointCloudShared constructor, upload
    const double base_us = host_us(warmup / 2 + 1, loops / 4 + 1, [&]() {
        PointCloudCPU cpu;
        cpu.points->resize(n);
        cpu.intensities->resize(n);
        cpu.timestamp_offsets->resize(n);
        double max_offset = 0.0;
        for (size_t i = 0; i < n; ++i) {
            (*cpu.points)[i] = PointType(get<float>(m, i, 0), get<float>(m, i, 4), get<float>(m, i, 8), 1.0f);
            (*cpu.intensities)[i] = get<float>(m, i, 16);
            const float off = float(get<uint32_t>(m, i, 20)) * 1e-6f;
            (*cpu.timestamp_offsets)[i] = off;
            max_offset = std::max(max_offset, double(off));
        }
        cpu.start_time_ms = L.start_time_ms;
        cpu.end_time_ms = cpu.start_time_ms + max_offset;
        PointCloudShared shared(q, cpu);
        (void)shared.points_device();
        (void)shared.intensities->device_data();
        (void)shared.timestamp_offsets->device_data();
        q.wait();
    });

    const double peak = 6.3e12;  // achievable HBM bytes per second
    std::printf("{\"n\": %zu, \"loops\": %d, \"unpack_us\": %.2f, \"unpack_bound_us\": %.2f, \"unpack_fraction\": %.3f, "
                "\"reflectivity_us\": %.2f, \"reflectivity_bound_us\": %.2f, \"reflectivity_fraction\": %.3f, "
                "\"from_msg_end_to_end_us\": %.1f, \"host_unpack_and_upload_us\": %.1f}\n",
                n, loops, unpack_us, 1e6 * unpack_bytes / peak, 1e6 * unpack_bytes / peak / unpack_us, er_us, 1e6 * er_bytes / peak,
                1e6 * er_bytes / peak / er_us, from_us, base_us);
    return 0;
}
