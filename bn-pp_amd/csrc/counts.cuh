// Expected counts (gfx950): one factor's belief folded into its accumulator,
// normalised row by row.
//
//   c[b]  = sum over rest, ascending, sequentially from 0.0, of (double)T[rest][b]
//   acc[offset(rest, evidence values of row b)] += w[b] * ((double)T[rest][b] / c[b])
//
// T is the belief over (rest dims, b), b fastest, R rows per launch (row
// stride 0: a belief no evidence reaches); acc the factor's fp64 accumulator in
// its natural layout over its whole scope, evidence variables included.  A row
// is skipped when b >= rows_live, w[b] == 0, c[b] is 0 or NaN, or its validity
// entry is 0.  All arithmetic is fp64, every operation rounded once (no
// contraction), and the contributions to one accumulator entry are added in
// ascending row order one at a time, so the result depends on neither the
// grid nor R nor how the rows split over launches.
//
// Pass 1 (counts_rows_kernel): one thread per b walks rest (loads coalesced in
// b) and writes c[b], w[b] and the row's evidence key to the scratch -- key -1
// marks a skipped row.  An evidence value is clamped into its variable's
// range, so no value can send a write outside acc.
// Pass 2 (counts_fold_kernel): one wave per rest entry, walked grid-stride by
// a persistent grid.  The wave loads 64 rows coalesced, every lane forms its
// row's term w * (t / c), and the terms are added in lane order (uniform reads
// of lane l, l = 0..63).  Key spaces of at most 64 keys: lane k owns the
// accumulator entry of key k in a register, loaded from acc before the first
// row and stored after the last, so a launch continues the chain the previous
// launch left.  Larger key spaces: the key is the entry's offset and lane 0
// adds straight into acc.  An entry (rest, key) belongs to one wave, so there
// is no atomic and no race.
// A plan's steps run together: blockIdx.y picks the step from a device array
// of their arguments (each step has scratch of its own), so the serial chains
// of different factors overlap; bnpp_bucket_counts launches one step with its
// arguments in the kernel-argument segment.
#pragma once
#include "kernels.cuh"

namespace bnpp {

constexpr int kCountsRegKeys = 64;     // key spaces up to this many keys accumulate in registers

__device__ __forceinline__ double counts_lane(double x, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}

// offset in acc of rest entry r (T's rest dims, fastest first)
__device__ __forceinline__ int64_t counts_rest_offset(cst_t<CountsArgs> &a, int64_t r) {
    int64_t off = 0;
    for (int d = 0; d < a.n_rest; ++d) {
        const int64_t c = a.r_card[d];
        off += (r % c) * a.r_stride[d];
        r /= c;
    }
    return off;
}

template <typename T>
__device__ __forceinline__ void counts_rows(cst_t<CountsArgs> &a) {
    const T *tab = static_cast<const T *>(a.table);
    const T *valid = static_cast<const T *>(a.valid);
    const int64_t R = a.n_rows;
    double *cs = static_cast<double *>(a.scratch), *ws = cs + R;
    int64_t *ks = reinterpret_cast<int64_t *>(ws + R);
    const bool dense = a.n_keys <= kCountsRegKeys;
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < a.rows_live; b += (int64_t)gridDim.x * kBlock) {
        double c = 0.0;
        for (int64_t r = 0; r < a.n_rest_entries; ++r) c = __dadd_rn(c, (double)gload(tab + (a.has_b ? r * R + b : r)));
        const double w = a.weights ? a.weights[b] : 1.0;
        bool skip = w == 0.0 || c == 0.0 || c != c;
        if (valid && (double)gload(valid + (a.valid_b ? b : 0)) == 0.0) skip = true;
        int64_t key = 0, radix = 1;
        for (int e = 0; e < a.n_e; ++e) {
            const int32_t x = a.ev[a.e_row[e] * R + b];
            const int64_t top = a.e_card[e] - 1;
            const int64_t v = x < 0 ? 0 : x > top ? top : x;
            key += v * (dense ? radix : a.e_stride[e]);
            radix *= a.e_card[e];
        }
        cs[b] = c;
        ws[b] = w;
        ks[b] = skip ? -1 : key;
    }
}

template <typename T>
__device__ __forceinline__ void counts_fold(cst_t<CountsArgs> &a) {
    const T *tab = static_cast<const T *>(a.table);
    const int64_t R = a.n_rows;
    const double *cs = static_cast<const double *>(a.scratch), *ws = cs + R;
    const int64_t *ks = reinterpret_cast<const int64_t *>(ws + R);
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (kBlock / 64);
    const bool dense = a.n_keys <= kCountsRegKeys;
    // dense keys: lane k's entry of key k (its digits in the order pass 1 packed them)
    int64_t koff = 0;
    if (dense) {
        int64_t q = lane;
        for (int e = 0; e < a.n_e; ++e) {
            koff += (q % a.e_card[e]) * a.e_stride[e];
            q /= a.e_card[e];
        }
    }
    const bool own = dense && lane < a.n_keys;
    for (int64_t r = wave; r < a.n_rest_entries; r += n_waves) {
        double *dst = a.acc + counts_rest_offset(a, r);
        double sum = own ? dst[koff] : 0.0;
        for (int64_t b0 = 0; b0 < a.rows_live; b0 += 64) {
            const int64_t b = b0 + lane;
            const bool in = b < a.rows_live;
            const int64_t key = in ? ks[b] : -1;
            double term = 0.0;
            if (key >= 0) term = __dmul_rn(ws[b], __ddiv_rn((double)gload(tab + (a.has_b ? r * R + b : r)), cs[b]));
            const int n = a.rows_live - b0 < 64 ? (int)(a.rows_live - b0) : 64;
            if (dense) {
                // straight-line: constant lane ids, a select instead of a branch (a lane past the
                // last row holds key -1, which no lane owns)
                const int k32 = (int)key;
#pragma unroll
                for (int l = 0; l < 64; ++l) {
                    const int kl = __builtin_amdgcn_readlane(k32, l);
                    const double next = __dadd_rn(sum, counts_lane(term, l));
                    sum = lane == kl ? next : sum;
                }
            } else {
                const int klo = (int)(key & 0xffffffff), khi = (int)(key >> 32);
                for (int l = 0; l < n; ++l) {
                    const int64_t kl = ((int64_t)__builtin_amdgcn_readlane(khi, l) << 32) |
                                       (uint32_t)__builtin_amdgcn_readlane(klo, l);
                    const double tl = counts_lane(term, l);
                    if (kl >= 0 && lane == 0) dst[kl] = __dadd_rn(dst[kl], tl);
                }
            }
        }
        if (own) dst[koff] = sum;
    }
}

// One step with its arguments in the kernel-argument segment (bnpp_bucket_counts).
template <typename T>
__global__ __launch_bounds__(kBlock) void counts_rows_kernel(const CountsArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)args;
    counts_rows<T>(*(cst_t<CountsArgs> *)__builtin_amdgcn_kernarg_segment_ptr());
#else
    counts_rows<T>(*(cst_t<CountsArgs> *)&args);
#endif
}
template <typename T>
__global__ __launch_bounds__(kBlock) void counts_fold_kernel(const CountsArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)args;
    counts_fold<T>(*(cst_t<CountsArgs> *)__builtin_amdgcn_kernarg_segment_ptr());
#else
    counts_fold<T>(*(cst_t<CountsArgs> *)&args);
#endif
}
// The accumulate steps of one level of a counts plan in one launch: step
// blockIdx.y of `list` (device), each with scratch of its own.  The steps'
// chains are independent, so they overlap instead of running one after another.
template <typename T>
__global__ __launch_bounds__(kBlock) void counts_rows_list_kernel(const CountsArgs *list) {
    counts_rows<T>(*as_const(list + blockIdx.y));
}
template <typename T>
__global__ __launch_bounds__(kBlock) void counts_fold_list_kernel(const CountsArgs *list) {
    counts_fold<T>(*as_const(list + blockIdx.y));
}

// persistent: the grids capped like the other persistent launches
template <typename T>
static hipError_t go_counts(const CountsArgs &a, int max_grid, hipStream_t stream) {
    const int64_t g1 = (a.rows_live + kBlock - 1) / kBlock, g2 = (a.n_rest_entries + kBlock / 64 - 1) / (kBlock / 64);
    auto cap = [&](int64_t g) { return (unsigned)(g < 1 ? 1 : g < max_grid ? g : max_grid); };
    hipLaunchKernelGGL((counts_rows_kernel<T>), dim3(cap(g1)), dim3(kBlock), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((counts_fold_kernel<T>), dim3(cap(g2)), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

// n steps (at most 65535) whose largest row and rest-entry counts are rows_max, rest_max
template <typename T>
static hipError_t go_counts_list(const CountsArgs *list, int n, int64_t rows_max, int64_t rest_max, int max_grid,
                                 hipStream_t stream) {
    const int64_t g1 = (rows_max + kBlock - 1) / kBlock, g2 = (rest_max + kBlock / 64 - 1) / (kBlock / 64);
    auto cap = [&](int64_t g) { return (unsigned)(g < 1 ? 1 : g < max_grid ? g : max_grid); };
    hipLaunchKernelGGL((counts_rows_list_kernel<T>), dim3(cap(g1), (unsigned)n), dim3(kBlock), 0, stream, list);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((counts_fold_list_kernel<T>), dim3(cap(g2), (unsigned)n), dim3(kBlock), 0, stream, list);
    return hipGetLastError();
}

}  // namespace bnpp
