// Reference-path forwarding header: pipeline/adaptive_motion_predictor.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../amd/pipeline.hpp"
