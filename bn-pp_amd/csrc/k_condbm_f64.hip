// Kernel instantiations compiled as a separate translation unit (parallel build).
// Masked batched conditioning kernels (condbatch.cuh, Masked = true): missing values.
#include "condbatch.cuh"

namespace bnpp {

hipError_t dispatch_cond_batch_masked_f64(const int64_t *pool, int64_t rest, TableMeta *meta, int out_table,
                                          const void *out_ptr, const int32_t *ev, int64_t n_rows, int max_grid,
                                          hipStream_t stream) {
    return go_cond_batch_masked<double>(pool, rest, meta, out_table, out_ptr, ev, n_rows, max_grid, stream);
}
hipError_t dispatch_cond_batch_masked_single_f64(const CondBatchMaskedArgs &a, int max_grid, hipStream_t stream) {
    return go_cond_batch_masked_single<double>(a, max_grid, stream);
}
}  // namespace bnpp
