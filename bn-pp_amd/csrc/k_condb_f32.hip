// Kernel instantiations compiled as a separate translation unit (parallel build).
// Batched conditioning kernels (condbatch.cuh): the plain gather.
#include "condbatch.cuh"

namespace bnpp {

template hipError_t go_cond_batch<float, kCondPlain>(const int64_t *, int64_t, TableMeta *, int, const void *, const int32_t *,
                                                    const void *, int64_t, int, hipStream_t);
template hipError_t go_cond_batch_single<float, kCondPlain>(const CondBatchArgs &, int, hipStream_t);
}  // namespace bnpp
