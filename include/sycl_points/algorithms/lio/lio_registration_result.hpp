// Reference-path forwarding header: algorithms/lio/lio_registration_result.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../../amd/lio.hpp"
