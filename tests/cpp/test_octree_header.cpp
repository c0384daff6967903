// knn::Octree through the reference's include path alone: the header needs nothing included before it.
#include "sycl_points/algorithms/knn/octree.hpp"

int main() {
    return sizeof(sycl_points::algorithms::knn::Octree) != 0 ? 0 : 1;
}
