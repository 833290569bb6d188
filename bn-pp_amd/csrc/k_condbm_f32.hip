// Kernel instantiations compiled as a separate translation unit (parallel build).
// Masked batched conditioning kernels (condbatch.cuh, kCondMasked): missing values.
#include "condbatch.cuh"

namespace bnpp {

template hipError_t go_cond_batch<float, kCondMasked>(const int64_t *, int64_t, TableMeta *, int, const void *, const int32_t *,
                                                     const void *, int64_t, int, hipStream_t);
template hipError_t go_cond_batch_single<float, kCondMasked>(const CondBatchArgs &, int, hipStream_t);
}  // namespace bnpp
