// Kernel instantiations compiled as a separate translation unit (parallel build).
// Generic gather kernels, tiles along two output dims.  Built with
// -mllvm -sink-common-insts=false (Makefile): SimplifyCFG otherwise merges the
// stores load_tile's stride cases have in common into one store whose tile
// slot is selected at run time, and the whole tile then lives in scratch
// memory (80-272 B per lane, each load waited for at once).  The one-dim
// tiles measured slower without the sinking and keep the default.
#include <vector>

#include "kernels.cuh"

namespace bnpp {

hipError_t dispatch_level_f32_2d(int key, const LevelArgs &a, int max_grid, hipStream_t stream) {
    switch (key) { BNPP_ALL(BNPP_CASE_LEVEL, BNPP_TILES_F32_2D, float) default: break; }
    return hipErrorInvalidValue;
}
hipError_t dispatch_single_f32_2d(int key, const SingleArgs &a, int max_grid, hipStream_t stream) {
    switch (key) { BNPP_ALL(BNPP_CASE_SINGLE, BNPP_TILES_F32_2D, float) default: break; }
    return hipErrorInvalidValue;
}
void keys_generic_f32_2d(std::vector<int> &keys) {
    static const int k[] = {BNPP_ALL(BNPP_LIST_GENERIC, BNPP_TILES_F32_2D, float)};
    keys.insert(keys.end(), k, k + sizeof k / sizeof *k);
}
}  // namespace bnpp
