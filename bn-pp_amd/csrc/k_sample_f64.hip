// Kernel instantiations compiled as a separate translation unit (parallel build).
// Posterior sampling kernels (sample.cuh).
#include "sample.cuh"

namespace bnpp {

hipError_t dispatch_sample_rows_f64(const int64_t *pool, const TableMeta *meta, uint8_t *x, int64_t n, int64_t first,
                                    uint64_t seed, unsigned long long *n_degenerate, int max_grid, hipStream_t stream) {
    return go_sample_rows<double>(pool, meta, x, n, first, seed, n_degenerate, max_grid, stream);
}
hipError_t dispatch_sample_rows_batch_f64(const int64_t *pool, const TableMeta *meta, uint8_t *x, unsigned long long *deg_rows,
                                          int64_t lanes, const SampleBatchLaunch &a, int max_grid, hipStream_t stream) {
    return go_sample_rows_batch<double>(pool, meta, x, deg_rows, lanes, a, max_grid, stream);
}
hipError_t dispatch_sample_single_f64(const SampleSingleArgs &a, int max_grid, hipStream_t stream) {
    return go_sample_single<double>(a, max_grid, stream);
}
}  // namespace bnpp
