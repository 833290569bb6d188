// Kernel instantiations compiled as a separate translation unit (parallel build).
// Max-product bucket kernels (maxout.cuh), the MPE decode and the batched decode (maxbatch.cuh).
#include <vector>

#include "maxout.cuh"
#include "maxbatch.cuh"

namespace bnpp {

hipError_t dispatch_max_level_f64(int key, const LevelArgs &a, int max_grid, hipStream_t stream) {
    switch (key) { BNPP_MAX_ALL(BNPP_CASE_MAX_LEVEL, double) default: break; }
    return hipErrorInvalidValue;
}
hipError_t dispatch_max_single_f64(int key, const SingleArgs &a, int max_grid, hipStream_t stream) {
    switch (key) { BNPP_MAX_ALL(BNPP_CASE_MAX_SINGLE, double) default: break; }
    return hipErrorInvalidValue;
}
void keys_max_f64(std::vector<int> &keys) {
    static const int k[] = {BNPP_MAX_ALL(BNPP_LIST_MAX, double)};
    keys.insert(keys.end(), k, k + sizeof k / sizeof *k);
}

hipError_t launch_mpe_decode(const int64_t *pool, const TableMeta *meta, int32_t *x, hipStream_t stream) {
    hipLaunchKernelGGL(mpe_decode_kernel<kBlock>, dim3(1), dim3(kBlock), 0, stream, pool, meta, x);
    return hipGetLastError();
}

hipError_t launch_mpe_decode_batch(const int64_t *pool, const TableMeta *meta, uint8_t *x, int64_t n_rows, int max_grid,
                                   hipStream_t stream) {
    if (n_rows <= 0) return hipSuccess;
    return go_mpe_decode_batch(pool, meta, x, n_rows, max_grid, stream);
}
}  // namespace bnpp
