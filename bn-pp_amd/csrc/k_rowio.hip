// Kernel instantiations compiled as a separate translation unit (parallel build).
// Device-resident row input and output of the batched calls (rowio.cuh).
#include "rowio.cuh"

namespace bnpp {

hipError_t launch_stage_rows(const RowioSingle<StageRowsArgs> &a, int max_grid, hipStream_t stream) {
    if (a.a.R <= 0 || a.a.n_ev <= 0) return hipSuccess;
    hipLaunchKernelGGL(stage_rows_kernel, dim3(rowio_grid(a.a.R, 64, max_grid)), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_stage_lik(const RowioSingle<StageLikArgs> &a, int max_grid, hipStream_t stream) {
    if (a.a.R <= 0 || a.a.n_soft <= 0) return hipSuccess;
    hipLaunchKernelGGL(stage_lik_kernel, dim3(rowio_grid(a.a.R, 64, max_grid)), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_stage_loglik(const RowioSingle<StageLikArgs> &a, int max_grid, hipStream_t stream) {
    if (a.a.R <= 0 || a.a.n_soft <= 0) return hipSuccess;
    hipLaunchKernelGGL(stage_loglik_kernel, dim3(rowio_grid(a.a.R, 64, max_grid)), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_stage_weights(const StageWeightsArgs &a, int max_grid, hipStream_t stream) {
    if (a.R <= 0) return hipSuccess;
    hipLaunchKernelGGL(stage_weights_kernel, dim3(rowio_grid(a.R, 64, max_grid)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_emit_scalars(const EmitScalarsArgs &a, int max_grid, hipStream_t stream) {
    if (a.rows_live <= 0) return hipSuccess;
    hipLaunchKernelGGL(emit_scalars_kernel, dim3(rowio_grid(a.rows_live, 64, max_grid)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_emit_logs(const EmitScalarsArgs &a, int max_grid, hipStream_t stream) {
    if (a.rows_live <= 0) return hipSuccess;
    hipLaunchKernelGGL(emit_logs_kernel, dim3(rowio_grid(a.rows_live, 64, max_grid)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_emit_states(const RowioSingle<EmitStatesArgs> &a, int max_grid, hipStream_t stream) {
    if (a.a.rows_live <= 0) return hipSuccess;
    const dim3 grid(rowio_grid(a.a.rows_live, 64, max_grid));
    if (a.a.sampling) hipLaunchKernelGGL(emit_states_sample_kernel, grid, dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL(emit_states_mpe_kernel, grid, dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace bnpp
