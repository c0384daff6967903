// Reference-path forwarding header: algorithms/filter/polar_downsampling.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../../amd/features.hpp"
