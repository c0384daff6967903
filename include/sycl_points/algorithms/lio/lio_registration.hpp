// Reference-path forwarding header: algorithms/lio/lio_registration.hpp of fateshelled/sycl_points maps onto the MI355X facade.
#pragma once
#include "../../amd/lio.hpp"
