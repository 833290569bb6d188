// Kernel instantiations compiled as a separate translation unit (parallel build).
// Expected-counts accumulate kernels (counts.cuh).
#include "counts.cuh"

namespace bnpp {

hipError_t dispatch_counts_f32(const CountsArgs &a, int max_grid, hipStream_t stream) {
    return go_counts<float>(a, max_grid, stream);
}
hipError_t dispatch_counts_list_f32(const CountsArgs *list, int n, int64_t rows_max, int64_t rest_max, int max_grid,
                                    hipStream_t stream) {
    return go_counts_list<float>(list, n, rows_max, rest_max, max_grid, stream);
}
}  // namespace bnpp
