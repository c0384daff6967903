// Reference-path forwarding header: utils/time_utils.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../amd/pipeline.hpp"
