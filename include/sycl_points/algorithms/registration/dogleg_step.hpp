// Reference-path forwarding header: algorithms/registration/dogleg_step.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../../amd/lio.hpp"
