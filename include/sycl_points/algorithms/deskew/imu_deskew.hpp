// Reference-path forwarding header: algorithms/deskew/imu_deskew.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../../amd/imu.hpp"
