// Kernel instantiations compiled as a separate translation unit (parallel build).
// Generic gather kernels, tiles along one output dim; two-dim tiles are in
// k_generic2_f64.hip.
#include <vector>

#include "kernels.cuh"

namespace bnpp {

hipError_t dispatch_level_f64_2d(int key, const LevelArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_single_f64_2d(int key, const SingleArgs &a, int max_grid, hipStream_t stream);

hipError_t dispatch_level_f64(int key, const LevelArgs &a, int max_grid, hipStream_t stream) {
    switch (key) { BNPP_ALL(BNPP_CASE_LEVEL, BNPP_TILES_1D, double) default: break; }
    return dispatch_level_f64_2d(key, a, max_grid, stream);
}
hipError_t dispatch_single_f64(int key, const SingleArgs &a, int max_grid, hipStream_t stream) {
    switch (key) { BNPP_ALL(BNPP_CASE_SINGLE, BNPP_TILES_1D, double) default: break; }
    return dispatch_single_f64_2d(key, a, max_grid, stream);
}
void keys_generic_f64_2d(std::vector<int> &keys);
void keys_generic_f64(std::vector<int> &keys) {
    static const int k[] = {BNPP_ALL(BNPP_LIST_GENERIC, BNPP_TILES_1D, double)};
    keys.insert(keys.end(), k, k + sizeof k / sizeof *k);
    keys_generic_f64_2d(keys);
}
}  // namespace bnpp
