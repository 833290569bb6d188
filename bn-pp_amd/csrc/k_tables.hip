// Kernel instantiations compiled as a separate translation unit (parallel build).
// Device-resident model tables (tables.cuh).
#include "tables.cuh"

namespace bnpp {

// the tables, then the shift in a one-wave launch of its own
hipError_t launch_stage_tables(const StageTablesSingle &a, bool log_form, int max_grid, hipStream_t stream) {
    if (a.a.n_factors > 0) {
        const dim3 grid(rowio_grid(a.a.n_factors, 1, max_grid));
        if (log_form) hipLaunchKernelGGL(stage_tables_log_kernel, grid, dim3(kBlock), 0, stream, a);
        else hipLaunchKernelGGL(stage_tables_kernel, grid, dim3(kBlock), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(tables_shift_kernel, dim3(1), dim3(64), 0, stream, a.a.out_shift, a.a.n_factors, log_form ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_mstep(const MstepArgs &a, int64_t n_cfg, int max_grid, hipStream_t stream) {
    if (n_cfg <= 0) return hipSuccess;
    hipLaunchKernelGGL(mstep_kernel, dim3(rowio_grid(n_cfg, kBlock, max_grid)), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace bnpp
