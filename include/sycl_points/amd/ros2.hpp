// sycl_points facade for MI355X — sensor_msgs/PointCloud2 in and out of a PointCloudShared:
//   ros2::fromROS2msg / ros2::toROS2msg     (ros2/convert.hpp:34-429)
//   ros2::EnhancedReflectivityCorrector     (ros2/enhanced_reflectivity.hpp:32-194)
// ROS 2 is not needed: the functions are templates over the message type and use only the member names of
// sensor_msgs::msg::PointCloud2, sensor_msgs::msg::PointField and std_msgs::msg::Header. ros2::compat holds plain structs with
// those members for programs without ROS; where <sensor_msgs/msg/point_cloud2.hpp> can be included the real types deduce.
//
// The reference converts coordinates, rgb and intensity in a kernel and runs the time stamps, the whole reflectivity correction
// and the packing of toROS2msg as host loops over USM-shared memory. Here the message's bytes are copied to the device once
// (msg_buffer) and everything else is sp_pc2_unpack / sp_enhanced_reflectivity / sp_pc2_pack on them.
//
// Two deliberate deviations from the reference:
//   1. toROS2msg declares its `timestamp` field where the data is. The reference declares it sizeof(double) - sizeof(float) = 4
//      bytes further (convert.hpp:371 adds sizeof(double) to the offset of the 4-byte field before it), so its own fromROS2msg
//      cannot read its own message back.
//   2. A message with is_bigendian set is refused (false, a line on stderr). The reference ignores the flag and misreads it.
#pragma once
#include <iostream>
#include <type_traits>

#include "core.hpp"

#if __has_include(<sensor_msgs/msg/point_cloud2.hpp>)
#include <sensor_msgs/msg/point_cloud2.hpp>
#define SYCL_POINTS_AMD_HAS_SENSOR_MSGS 1
#endif

namespace sycl_points {
namespace ros2 {

namespace compat {
/// builtin_interfaces/Time, std_msgs/Header, sensor_msgs/PointField, sensor_msgs/PointCloud2: the members the conversions use
struct Time {
    int32_t sec = 0;
    uint32_t nanosec = 0;
};
struct Header {
    Time stamp;
    std::string frame_id;
};
struct PointField {
    static constexpr uint8_t INT8 = 1, UINT8 = 2, INT16 = 3, UINT16 = 4, INT32 = 5, UINT32 = 6, FLOAT32 = 7, FLOAT64 = 8;
    std::string name;
    uint32_t offset = 0;
    uint8_t datatype = 0;
    uint32_t count = 0;
};
struct PointCloud2 {
    using SharedPtr = std::shared_ptr<PointCloud2>;
    Header header;
    uint32_t height = 0, width = 0;
    std::vector<PointField> fields;
    bool is_bigendian = false;
    uint32_t point_step = 0, row_step = 0;
    std::vector<uint8_t> data;
    bool is_dense = false;
};
}  // namespace compat

namespace detail {
/// the message type that goes with a header type (toROS2msg is given the header only)
template <class Header> struct message_of;
template <> struct message_of<compat::Header> { using type = compat::PointCloud2; };
#ifdef SYCL_POINTS_AMD_HAS_SENSOR_MSGS
template <> struct message_of<std_msgs::msg::Header> { using type = sensor_msgs::msg::PointCloud2; };
#endif

/// msg.data on the device: copied into msg_buffer, which only ever grows (convert.hpp:195-199)
template <class Msg>
inline const uint8_t* upload_message(const sycl_utils::DeviceQueue& queue, const Msg& msg, shared_vector_ptr<uint8_t>& msg_buffer) {
    if (msg_buffer == nullptr) msg_buffer = std::make_shared<shared_vector<uint8_t>>(queue);
    const size_t bytes = msg.data.size();
    uint8_t* dev = msg_buffer->size() < bytes ? msg_buffer->device_data_for_write(bytes) : msg_buffer->device_data_rw();
    if (bytes) sycl_points::detail::StagedCopy::h2d(dev, msg.data.data(), bytes, queue.stream());
    return dev;
}
}  // namespace detail

/// ros2/convert.hpp:34-320. The cloud is (re)created on `queue` when it is null or bound to another queue; its attributes are
/// written by one sp_pc2_unpack and stay on the device. start_time_ms is the header stamp, end_time_ms = start_time_ms + the largest
/// time offset before its cast to float, which is the call's one read-back (8 bytes). False, with the reference's line on
/// stderr, for a message without x / y / z of one type FLOAT32 or FLOAT64, and for a big-endian one (deviation 2). A field that
/// runs past point_step, or data shorter than width * height records, throws std::invalid_argument.
template <class Msg>
inline bool fromROS2msg(const sycl_utils::DeviceQueue& queue, const Msg& msg, PointCloudShared::Ptr& cloud,
                        shared_vector_ptr<uint8_t>& msg_buffer, bool convert_rgb = true, bool convert_intensity = true,
                        bool use_reflectivity_as_intensity = true) {
    if (msg.is_bigendian) {
        std::cerr << "Not supported big-endian point cloud" << std::endl;
        return false;
    }
    std::vector<const char*> names;
    std::vector<uint32_t> offsets;
    std::vector<uint8_t> types;
    for (const auto& field : msg.fields) {
        names.push_back(field.name.c_str());
        offsets.push_back(field.offset);
        types.push_back(field.datatype);
    }
    sp_pc2_layout layout;
    const int rc = sp_pc2_resolve_fields_host(names.data(), offsets.data(), types.data(), names.size(), msg.point_step, convert_rgb,
                                              convert_intensity, use_reflectivity_as_intensity, &layout);
    if (rc == SP_ERR_RUNTIME) {
        std::cerr << sp_last_error() << std::endl;
        return false;
    }
    throw_on_error(rc);
    if (cloud == nullptr || cloud->queue.ptr != queue.ptr) cloud = std::make_shared<PointCloudShared>(queue);
    const size_t point_size = size_t(msg.width) * size_t(msg.height);
    cloud->clear();
    if (point_size == 0) return true;

    const uint8_t* data = detail::upload_message(queue, msg, msg_buffer);
    layout.start_time_ms = static_cast<double>(msg.header.stamp.sec) * 1000.0 + static_cast<double>(msg.header.stamp.nanosec) * 1e-6;
    const bool has_rgb = layout.rgb_offset >= 0, has_intensity = layout.intensity_offset >= 0, has_timestamp = layout.timestamp_offset >= 0;
    float* points = reinterpret_cast<float*>(cloud->points->device_data_for_write(point_size));
    float* rgb = has_rgb ? reinterpret_cast<float*>(cloud->rgb->device_data_for_write(point_size)) : nullptr;
    float* intensities = has_intensity ? cloud->intensities->device_data_for_write(point_size) : nullptr;
    float* timestamps = has_timestamp ? cloud->timestamp_offsets->device_data_for_write(point_size) : nullptr;
    shared_vector<double> max_offset_ms(queue);  // [0]: the maximum; from [2] on: sp_pc2_unpack's workspace (16-byte aligned)
    double* max_dev = has_timestamp ? max_offset_ms.device_data_for_write(2 + sp_pc2_unpack_workspace_bytes(point_size) / sizeof(double)) : nullptr;
    throw_on_error(sp_pc2_unpack(data, msg.data.size(), point_size, &layout, points, rgb, intensities, timestamps, max_dev,
                                 has_timestamp ? max_dev + 2 : nullptr, queue.stream()));
    if (has_timestamp) {
        cloud->start_time_ms = layout.start_time_ms;
        cloud->end_time_ms = cloud->start_time_ms + std::as_const(max_offset_ms)[0];  // (waits for the kernel: the read-back)
    }
    return true;
}

/// ros2/convert.hpp:322-329
template <class Msg>
inline PointCloudShared::Ptr fromROS2msg(const sycl_utils::DeviceQueue& queue, const Msg& msg, shared_vector_ptr<uint8_t>& msg_buffer,
                                         bool convert_rgb = true, bool convert_intensity = true,
                                         bool use_reflectivity_as_intensity = true) {
    PointCloudShared::Ptr ret = nullptr;
    fromROS2msg(queue, msg, ret, msg_buffer, convert_rgb, convert_intensity, use_reflectivity_as_intensity);
    return ret;
}

/// ros2/convert.hpp:331-429: x, y, z (FLOAT32 at 0, 4, 8; the record keeps the point's w), then rgb (UINT32), intensity
/// (FLOAT32) and timestamp (FLOAT64, seconds) where the cloud has them. The records are packed by sp_pc2_pack and come back in
/// one device-to-host copy. The timestamp field's offset is where the data is (deviation 1).
template <class Header>
inline std::shared_ptr<typename detail::message_of<Header>::type> toROS2msg(const PointCloudShared& cloud, const Header& header) {
    using Msg = typename detail::message_of<Header>::type;
    auto msg = std::make_shared<Msg>();
    msg->header = header;
    const bool has_rgb = cloud.has_rgb(), has_intensity = cloud.has_intensity(), has_timestamp = cloud.has_timestamps();
    typename std::decay_t<decltype(msg->fields)>::value_type field;
    field.count = 1;
    uint32_t offset = 0;
    auto add = [&](const char* name, uint8_t datatype, uint32_t size) {
        field.name = name;
        field.datatype = datatype;
        field.offset = offset;
        msg->fields.push_back(field);
        offset += size;
    };
    add("x", SP_PC2_FLOAT32, 4);
    add("y", SP_PC2_FLOAT32, 4);
    add("z", SP_PC2_FLOAT32, 8);  // (the point's w follows z)
    if (has_rgb) add("rgb", SP_PC2_UINT32, 4);
    if (has_intensity) add("intensity", SP_PC2_FLOAT32, 4);
    if (has_timestamp) add("timestamp", SP_PC2_FLOAT64, 8);

    const size_t n = cloud.size();
    msg->width = static_cast<uint32_t>(n);
    msg->height = 1;
    msg->point_step = sp_pc2_pack_point_step(has_rgb, has_intensity, has_timestamp);
    msg->row_step = static_cast<uint32_t>(msg->point_step * n);
    msg->is_bigendian = false;
    msg->is_dense = true;
    const size_t bytes = size_t(msg->point_step) * n;
    msg->data.resize(bytes);
    if (n == 0) return msg;
    const hipStream_t stream = cloud.queue.stream();
    shared_vector<uint8_t> packed(cloud.queue);
    uint8_t* dev = packed.device_data_for_write(bytes);
    throw_on_error(sp_pc2_pack(cloud.points_device(), has_rgb ? reinterpret_cast<const float*>(cloud.rgb->device_data()) : nullptr,
                               has_intensity ? cloud.intensities->device_data() : nullptr,
                               has_timestamp ? cloud.timestamp_offsets->device_data() : nullptr, n, cloud.start_time_ms, dev, stream));
    hip_check(hipStreamSynchronize(stream), "toROS2msg");
    sycl_points::detail::StagedCopy::d2h(msg->data.data(), dev, bytes, stream);
    return msg;
}

/// ros2/enhanced_reflectivity.hpp:32-194. Made for Ouster scans, whose messages carry `ambient` (UINT16) and `ring` (UINT8 or
/// UINT16) beside the intensity: intensity * range^2 and ambient / range^2, each divided by its ring's mean, summed and clipped.
/// The ring means are kept across calls (EMA) in device memory, and a call is three launches of sp_enhanced_reflectivity with no
/// read-back. The field offsets are parsed on the first message that has them and kept (:145-175).
class EnhancedReflectivityCorrector {
public:
    static constexpr size_t MAX_RINGS = SP_ER_MAX_RINGS;

    explicit EnhancedReflectivityCorrector(float ema_alpha = 0.5f) : ema_alpha_(ema_alpha) {}
    void set_ema_alpha(float alpha) { ema_alpha_ = alpha; }

    /// :45-140. Uploads msg.data itself. False, the cloud untouched, when the cloud has no intensity or the message no ambient /
    /// ring field of the types above.
    template <class Msg>
    bool apply(PointCloudShared& cloud, const Msg& msg, float clip_max = 5.0f) {
        if (!cloud.has_intensity()) return false;
        if (!parse_fields(msg)) return false;
        return run(cloud, msg.point_step, detail::upload_message(cloud.queue, msg, own_buffer_), msg.data.size(), clip_max);
    }
    /// The same on the bytes fromROS2msg has just put into `msg_buffer` for this message: nothing is uploaded.
    template <class Msg>
    bool apply(PointCloudShared& cloud, const Msg& msg, const shared_vector_ptr<uint8_t>& msg_buffer, float clip_max = 5.0f) {
        if (!cloud.has_intensity()) return false;
        if (!parse_fields(msg)) return false;
        if (msg_buffer == nullptr) throw std::invalid_argument("[EnhancedReflectivityCorrector::apply] null msg_buffer");
        return run(cloud, msg.point_step, msg_buffer->device_data(), msg_buffer->size(), clip_max);
    }

    /// the per-ring state as the host sees it (one small read-back; for tests and diagnostics)
    std::array<float, MAX_RINGS> ring_mean_ref() const { return state_slice<float>(0); }
    std::array<float, MAX_RINGS> ring_mean_amb() const { return state_slice<float>(1); }
    std::array<uint32_t, MAX_RINGS> ring_initialized() const { return state_slice<uint32_t>(2); }

private:
    bool run(PointCloudShared& cloud, size_t point_step, const uint8_t* data, size_t data_bytes, float clip_max) {
        const size_t N = cloud.size();
        if (N * point_step > data_bytes)
            throw std::invalid_argument("[EnhancedReflectivityCorrector::apply] the message holds fewer records than the cloud has points");
        if (state_ == nullptr) state_ = std::make_shared<shared_vector<uint32_t>>(3 * MAX_RINGS, 0u, cloud.queue);
        if (workspace_ == nullptr) workspace_ = std::make_shared<shared_vector<uint8_t>>(cloud.queue);
        const size_t ws_bytes = std::max<size_t>(sp_enhanced_reflectivity_workspace_bytes(N), 16);
        uint8_t* ws = workspace_->size() < ws_bytes ? workspace_->device_data_for_write(ws_bytes) : workspace_->device_data_rw();
        throw_on_error(sp_enhanced_reflectivity(cloud.points_device(), cloud.intensities->device_data_rw(), N, data,
                                                static_cast<uint32_t>(point_step), ring_offset_, ring_is_uint8_, ambient_offset_,
                                                state_->device_data_rw(), ema_alpha_, clip_max, ws, cloud.queue.stream()));
        return true;
    }
    /// :145-175
    template <class Msg>
    bool parse_fields(const Msg& msg) {
        if (fields_parsed_) return true;
        int32_t ambient_offset = -1, ring_offset = -1;
        uint8_t ambient_type = 0, ring_type = 0;
        for (const auto& field : msg.fields) {
            if (field.name == "ambient") {
                ambient_offset = static_cast<int32_t>(field.offset);
                ambient_type = field.datatype;
            } else if (field.name == "ring") {
                ring_offset = static_cast<int32_t>(field.offset);
                ring_type = field.datatype;
            }
        }
        if (ambient_offset < 0 || ring_offset < 0) return false;
        if (ambient_type != SP_PC2_UINT16) return false;
        if (ring_type != SP_PC2_UINT8 && ring_type != SP_PC2_UINT16) return false;
        ambient_offset_ = ambient_offset;
        ring_offset_ = ring_offset;
        ring_is_uint8_ = ring_type == SP_PC2_UINT8;
        fields_parsed_ = true;
        return true;
    }
    template <class T>
    std::array<T, MAX_RINGS> state_slice(size_t which) const {
        std::array<T, MAX_RINGS> out{};
        if (state_ != nullptr) std::memcpy(out.data(), std::as_const(*state_).data() + which * MAX_RINGS, sizeof(T) * MAX_RINGS);
        return out;
    }

    float ema_alpha_;
    bool fields_parsed_ = false;
    int32_t ambient_offset_ = -1, ring_offset_ = -1;
    bool ring_is_uint8_ = false;
    std::shared_ptr<shared_vector<uint32_t>> state_;  // 256 ref means, 256 amb means, 256 initialised flags: on the device
    shared_vector_ptr<uint8_t> workspace_, own_buffer_;
};

}  // namespace ros2
}  // namespace sycl_points
