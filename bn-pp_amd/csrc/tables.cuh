// Device-resident model tables (gfx950): the steps that rewrite a model's
// tables in place on the device and refit them, so that a training loop never
// takes a table through the host.
//
//   stage_tables   values = flat [sum of sizes]  ->  every factor's pre-scaled table in the layout of
//                  upload_sources (runtime.cpp), its TableMeta, its top; then the shift in a launch of its own
//   mstep          counts, old values            ->  new values, per parent configuration (learn.m_step)
//
// include/bnpp.h states each step's arithmetic with its entry (bnpp_stage_tables, bnpp_mstep_dv).
//
// stage_tables: a workgroup owns a factor and a persistent grid walks the factors.  Pass one reads the factor
// once, lane t entries t, t + 256, ... (a wave's loads are 64 consecutive entries: coalesced), flags an invalid
// entry in the status word (a 64-bit atomic minimum over flat indices, which only an invalid entry touches) and
// reduces the maximum: within a wave by lane exchanges, across the four waves through four doubles of LDS.  max
// is exact in any order, so neither the grid nor the lane split shows in a bit.  Pass two reads the factor again
// and stores the scaled entries the same way.  The two forms of an entry are the two forms of a likelihood block
// (rowio_dev.cuh lik_exponent / lik_scaled): linear, scaled by the power of two that brings the top into [0.5, 1);
// log, exp(l - top) / 2.  The largest stored entry is the top's own, because scaling and rounding are monotone.
//
// The shift (log form: the sum of the factors' tops in factor order, from 0.0) is one lane of a second launch, so
// it does not depend on the grid either.
//
// mstep: a lane owns a parent configuration, k contiguous entries; the lanes of all factors run in one launch
// and find their factor by bisection of the configurations' prefix sums.
#pragma once
#include "rowio_dev.cuh"

namespace bnpp {

// the maximum of v over the workgroup, in every lane; red: kBlock / 64 doubles of LDS
__device__ __forceinline__ double tables_block_max(double v, double *red) {
    for (int d = 32; d > 0; d >>= 1) {
        const double o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();                                    // the previous factor's readers are done with red
    if (lane == 0) red[wv] = v;
    __syncthreads();
    double m = red[0];
    for (int q = 1; q < kBlock / 64; ++q) m = red[q] > m ? red[q] : m;
    return m;
}

template <bool kLog>
__device__ __forceinline__ void stage_tables_body(cst_t<StageTablesSingle> &s) {
    __shared__ double red[kBlock / 64];
    cst_t<StageTablesArgs> &a = s.a;
    cst_t<int64_t> *w = a.words ? as_const(a.words) : s.single;
    constexpr double kFloor = kLog ? -__builtin_inf() : 0.0;
    for (int64_t f = blockIdx.x; f < a.n_factors; f += gridDim.x) {
        const int64_t in0 = w[3 * f], size = w[3 * f + 1], out_off = w[3 * f + 2];
        double top = kFloor;
        for (int64_t j = threadIdx.x; j < size; j += kBlock) {
            double v = rowio_elem(a.values, a.values_f32, in0 + j);
            if (lik_invalid<kLog>(v)) {
                rowio_flag(a.status, 0, in0 + j);
                v = kFloor;
            }
            top = v > top ? v : top;
        }
        top = tables_block_max(top, red);
        const int e = lik_exponent<kLog>(top);
        char *out = static_cast<char *>(a.out_buf) + out_off;
        for (int64_t j = threadIdx.x; j < size; j += kBlock) {
            const double v = lik_scaled<kLog>(rowio_elem(a.values, a.values_f32, in0 + j), top, e);
            if (a.out_f32) *((gbl_t<float> *)out + j) = lik_to_float(v);
            else *((gbl_t<double> *)out + j) = v;
        }
        if (threadIdx.x == 0) {
            const double big = lik_scaled<kLog>(top, top, e);
            gbl_t<TableMeta> *m = (gbl_t<TableMeta> *)a.out_meta + f;
            m->ptr = out;
            m->maxbits = a.out_f32 ? (uint64_t)__float_as_uint(lik_to_float(big)) : (uint64_t)__double_as_longlong(big);
            m->exp2 = e;
            m->size = size;
            *((gbl_t<double> *)a.out_shift + 1 + f) = top;
        }
    }
}

__global__ __launch_bounds__(kBlock) void stage_tables_kernel(const StageTablesSingle args) {
    stage_tables_body<false>(kernarg_of(args));
}
__global__ __launch_bounds__(kBlock) void stage_tables_log_kernel(const StageTablesSingle args) {
    stage_tables_body<true>(kernarg_of(args));
}

// shift[0] = the log form's shift: the tops shift[1 + f] added in factor order from 0.0, a factor of nothing but
// -inf left out; the linear form's is 0.  One lane
__global__ __launch_bounds__(64) void tables_shift_kernel(double *shift, int64_t n_factors, int log_form) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int64_t f = 0; log_form && f < n_factors; ++f) {
        const double t = gload(shift + 1 + f);
        if (t != -__builtin_inf()) s = __dadd_rn(s, t);
    }
    *((gbl_t<double> *)shift) = s;
}

// ---- mstep ---------------------------------------------------------------------------------------------------
// words, per factor: its first entry, k, its first configuration; then the number of configurations in all
__global__ __launch_bounds__(kBlock) void mstep_kernel(const MstepArgs args) {
    cst_t<MstepArgs> &a = kernarg_of(args);
    cst_t<int64_t> *w = as_const(a.words);
    const int64_t n_cfg = w[3 * a.n_factors];
    for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_cfg; c += (int64_t)gridDim.x * kBlock) {
        int64_t lo = 0, hi = a.n_factors - 1;           // the last factor whose first configuration is <= c
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (w[3 * mid + 2] <= c) lo = mid;
            else hi = mid - 1;
        }
        const int64_t k = w[3 * lo + 1], at = w[3 * lo] + (c - w[3 * lo + 2]) * k;
        double tot = 0.0;
        for (int64_t i = 0; i < k; ++i) tot = __dadd_rn(tot, __dadd_rn(gload(a.counts + at + i), a.prior));
        for (int64_t i = 0; i < k; ++i) {
            const double v = tot > 0 ? __ddiv_rn(__dadd_rn(gload(a.counts + at + i), a.prior), tot) : gload(a.old_values + at + i);
            *((gbl_t<double> *)a.new_values + at + i) = v;
        }
    }
}

}  // namespace bnpp
