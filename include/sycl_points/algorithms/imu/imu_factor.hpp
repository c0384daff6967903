// Reference-path forwarding header: algorithms/imu/imu_factor.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../../amd/lio.hpp"
