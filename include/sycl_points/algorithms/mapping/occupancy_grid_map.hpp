// Reference-path forwarding header: algorithms/mapping/occupancy_grid_map.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../../amd/mapping.hpp"
