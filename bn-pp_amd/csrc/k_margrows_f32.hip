// Kernel instantiations compiled as a separate translation unit (parallel build).
// Batched-marginals emit kernels (margrows.cuh).
#include "margrows.cuh"

namespace bnpp {

hipError_t dispatch_marg_rows_f32(const int64_t *pool, const TableMeta *meta, const int32_t *ev, double *out,
                                  int64_t rows_live, int max_grid, hipStream_t stream) {
    return go_marg_rows<float>(pool, meta, ev, out, rows_live, max_grid, stream);
}
hipError_t dispatch_marg_rows_single_f32(const MargRowsSingleArgs &a, int max_grid, hipStream_t stream) {
    return go_marg_rows_single<float>(a, max_grid, stream);
}
}  // namespace bnpp
