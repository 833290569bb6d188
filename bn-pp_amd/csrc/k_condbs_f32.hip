// Kernel instantiations compiled as a separate translation unit (parallel build).
// Weighted batched conditioning kernels (condbatch.cuh, cond_batch_soft): soft evidence.
#include "condbatch.cuh"

namespace bnpp {

hipError_t dispatch_cond_batch_soft_f32(const int64_t *pool, int64_t rest, TableMeta *meta, int out_table,
                                        const void *out_ptr, const int32_t *ev, const void *lam, int64_t n_rows,
                                        int max_grid, hipStream_t stream) {
    return go_cond_batch_soft<float>(pool, rest, meta, out_table, out_ptr, ev, lam, n_rows, max_grid, stream);
}
hipError_t dispatch_cond_batch_soft_single_f32(const CondBatchSoftArgs &a, int max_grid, hipStream_t stream) {
    return go_cond_batch_soft_single<float>(a, max_grid, stream);
}
}  // namespace bnpp
