// Reference-path forwarding header: pipeline/lidar_inertial_odometry_params.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../amd/pipeline.hpp"
