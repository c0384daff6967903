// Reference-path forwarding header: ros2/enhanced_reflectivity.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../amd/ros2.hpp"
