// Kernel instantiations compiled as a separate translation unit (parallel build).
// Max-product bucket kernels (maxout.cuh).
#include <vector>

#include "maxout.cuh"

namespace bnpp {

hipError_t dispatch_max_level_f32(int key, const LevelArgs &a, int max_grid, hipStream_t stream) {
    switch (key) { BNPP_MAX_ALL(BNPP_CASE_MAX_LEVEL, float) default: break; }
    return hipErrorInvalidValue;
}
hipError_t dispatch_max_single_f32(int key, const SingleArgs &a, int max_grid, hipStream_t stream) {
    switch (key) { BNPP_MAX_ALL(BNPP_CASE_MAX_SINGLE, float) default: break; }
    return hipErrorInvalidValue;
}
void keys_max_f32(std::vector<int> &keys) {
    static const int k[] = {BNPP_MAX_ALL(BNPP_LIST_MAX, float)};
    keys.insert(keys.end(), k, k + sizeof k / sizeof *k);
}
}  // namespace bnpp
