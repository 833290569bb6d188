// Device helpers shared by the row input and output steps (rowio.cuh) and the model-table steps (tables.cuh): the
// kernel-argument segment as a constant-address-space struct, the status words, a table's entry as a double, the
// two forms of a staged entry, the grid of a persistent launch.  No kernel is defined here, so any number of
// translation units may include it.
#pragma once
#include "kernels.cuh"

namespace bnpp {

// a kernel's one argument struct, read where it lies in the kernel-argument segment (the scalar cache)
template <typename A>
__device__ __forceinline__ cst_t<A> &kernarg_of(const A &args) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)args;
    return *(cst_t<A> *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    return *(cst_t<A> *)&args;
#endif
}

__device__ __forceinline__ void rowio_flag(int64_t *status, int word, int64_t cell) {
    __hip_atomic_fetch_min(status + word, cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the value a table of floats or doubles holds at entry i, as a double; no table: the empty product
__device__ __forceinline__ double rowio_elem(const void *table, int is_f32, int64_t i) {
    if (!table) return 1.0;
    return is_f32 ? (double)gload(static_cast<const float *>(table) + i) : gload(static_cast<const double *>(table) + i);
}

// an entry that is NaN, infinite or negative counts as 0
__device__ __forceinline__ bool lik_bad(double v) { return !(v >= 0) || v == __builtin_inf(); }

// (float)v, rounded once to nearest even, subnormal results included without relying on the conversion
// instruction's denormal mode: below 2^-126 the sum with 2^-97 (whose ulp is 2^-149, the subnormal floats'
// spacing) rounds v to a multiple of 2^-149, and that multiple is the float's bit pattern
__device__ __forceinline__ float lik_to_float(double v) {
    if (v >= 0x1p-126) return (float)v;
    const double m = __dsub_rn(__dadd_rn(v, 0x1p-97), 0x1p-97);
    return __uint_as_float((unsigned)__dmul_rn(m, 0x1p149));
}

// The two forms of a likelihood block.  Linear: the entries are likelihoods, the block is scaled by the power of two
// that brings its top into [0.5, 1).  Log: the entries are natural logs (-inf: the likelihood 0; NaN and +inf are
// invalid and count as -inf), the block is E = exp(l - top) scaled by 2^-1, which is what the linear form makes of
// E (its top is 1.0 = 0.5 * 2^1); a block of nothing but -inf is all zero and adds no exponent
template <bool kLog>
__device__ __forceinline__ bool lik_invalid(double v) {
    if (kLog) return v != v || v == __builtin_inf();
    return lik_bad(v);
}
template <bool kLog>
__device__ __forceinline__ int lik_exponent(double top) {
    if (kLog) return top == -__builtin_inf() ? 0 : 1;
    int e = 0;
    if (top > 0) (void)frexp(top, &e);
    return e;
}
template <bool kLog>
__device__ __forceinline__ double lik_scaled(double v, double top, int e) {
    if (kLog) return lik_invalid<true>(v) || top == -__builtin_inf() ? 0.0 : ldexp(exp(__dsub_rn(v, top)), -1);
    return ldexp(lik_bad(v) ? 0.0 : v, -e);
}

// persistent: a workgroup per tile of 64 rows, capped like the other persistent launches
inline unsigned rowio_grid(int64_t rows, int64_t per, int max_grid) {
    const int64_t g = (rows + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : g < max_grid ? g : max_grid);
}

}  // namespace bnpp
