// Reference-path forwarding header: pipeline/motion_predictor.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../amd/pipeline.hpp"
