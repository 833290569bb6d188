// Batched conditioning (gfx950): a source table gathered into a table over its
// non-evidence variables and the virtual variable B = "which evidence row".
//
//   out[rest][b] = src[ sum_e ev[row_e][b] * stride_e + offset(rest) ]
//
// src is a source table in its natural layout, rest its non-evidence variables
// (row-major, adjacent ones merged on the host), b the fastest output dim of
// R rows.  ev is int32[n_ev_rows][R], variable-major: a wave reads 64 rows of
// one evidence variable as 256 contiguous bytes.  A thread owns V consecutive
// b (V = 16 bytes of T when R is a multiple of it and the tables are 16-byte
// aligned, else 1), computes its V base offsets once and walks a chunk of
// rest: stores are contiguous in b (a wave writes 64 * V consecutive
// entries), reads are per-lane gathers at 64-bit offsets from a table that is
// usually cache-resident.  An evidence value is clamped into its variable's
// range, so no value can send a read outside src.
//
// Work: virtual blocks of (kBlock * V rows) x (kCondRestChunk rest entries),
// row blocks fastest, walked grid-stride by a persistent grid.  The rest
// offset is an odometer over the (wave-uniform) rest dims: scalar registers.
//
// One body, cond_batch<T, V, Form>, in three instantiations (plan.hpp CondForm):
//
// kCondPlain: the gather above.  It moves values and does no arithmetic on them.
//
// kCondMasked (missing values): some rest dims are PARTIAL evidence variables.
// Row b keeps an entry only where, for every partial dim, its evidence value
// is negative (missing) or equals the dim's digit:
//
//   out[rest][b] = src[...]  if for every partial dim p: ev[row_p][b] < 0 or ev[row_p][b] == digit_p(rest)
//                  0         otherwise
//
// A masked-out entry issues no load; a value >= the card equals no digit.  The
// digits are the (wave-uniform) odometer's, so the test is one compare of a
// lane's value against a scalar per partial dim.
//
// kCondWeighted (soft evidence): some rest dims are SOFT variables, masks
// beside them.  Row b scales an entry by its likelihood of each soft dim's
// digit, in the order of the source's scope, left to right, each product
// rounded once:
//
//   out[rest][b] = mask_b(rest) ? ((src[...] * lam[row0_d1 + digit_d1][b]) * lam[row0_d2 + digit_d2][b]) ... : 0
//
// lam is T[Ws][R], (variable, value)-major, rows fastest: the digits are the
// odometer's, so a wave reads the weights of one rest entry and one soft dim
// as one contiguous run of 64 * V entries -- a uniform base plus the lane's b
// -- through the V-wide path of the stores.  A dim's weights are folded into
// the running product before the next dim's are loaded.  lam is unused, and
// may be null, in the other two forms.
//
// A partial or a soft dim is never merged with a neighbour.
//
// pool (int64 words, plan.cpp build_condb_desc):
//   [0] source table  [1] n_e  [2] n_rest  [3] rest entries
//   n_e x (row of ev, stride in src, card)     evidence variables in the scope
//   n_rest x (card, stride in src)             fastest first, at most kCondMaxRest
//   n_p, then n_p x (row of ev, index of the rest dim)            masked and weighted (n_p may be 0 there)
//   n_s, then n_s x (first row of lam, index of the rest dim)     weighted
#pragma once
#include "kernels.cuh"

namespace bnpp {

constexpr int kCondRestChunk = 32;     // rest entries per virtual block
constexpr int kCondBatchU = 4;         // rest entries whose gathers are in flight together

template <typename T, int V, int Form>
__device__ __forceinline__ void cond_batch(cst_t<int64_t> *pool, const T *src, T *out, const int32_t *ev, const T *lam,
                                           int64_t R) {
    constexpr bool kMask = Form >= kCondMasked, kWeigh = Form == kCondWeighted;
    const int n_e = (int)pool[1], n_rest = (int)pool[2];
    const int64_t n_r = pool[3];
    cst_t<int64_t> *ew = pool + 4, *rw = ew + 3 * n_e;
    // the mask and weight words: the weighted form reads its two counts here, once; the masked form reads its one
    // count per virtual block, next to its use (with the SGPR file full, either form allocates registers worse
    // the other way round: measured 1 to 3 % slower)
    int n_p = 0, n_s = 0;
    if constexpr (kWeigh) {
        n_p = (int)rw[2 * n_rest];
        n_s = (int)rw[2 * n_rest + 1 + 2 * n_p];
    }
    const int64_t nbb = (R / V + kBlock - 1) / kBlock;
    const int64_t nrc = (n_r + kCondRestChunk - 1) / kCondRestChunk;
    for (int64_t vb = blockIdx.x; vb < nbb * nrc; vb += gridDim.x) {
        const int64_t rc = vb / nbb, bb = vb - rc * nbb;
        const int64_t b = (bb * kBlock + threadIdx.x) * V;
        const bool live = b < R;
        int64_t base[V];
#pragma unroll
        for (int j = 0; j < V; ++j) base[j] = 0;
        if (live) {
            for (int e = 0; e < n_e; ++e) {
                int32_t x[V];
                load_n<int32_t, V, false, true>(ev + ew[3 * e] * R + b, x);
                const int32_t top = (int32_t)ew[3 * e + 2] - 1;
                const int64_t st = ew[3 * e + 1];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int32_t c = x[j] < 0 ? 0 : x[j] > top ? top : x[j];
                    base[j] += (int64_t)c * st;
                }
            }
        }
        // per rest dim, resolved once: a partial dim's values of the lane (-1, "missing", for every other dim and a
        // dead lane), a soft dim's first row of lam (uniform)
        int32_t pv[kMask ? kCondMaxRest : 1][V];
        bool pd[kMask ? kCondMaxRest : 1];
        int32_t srow[kWeigh ? kCondMaxRest : 1];            // -1: not a soft dim
        if constexpr (kMask) {
            if constexpr (!kWeigh) n_p = (int)rw[2 * n_rest];
            cst_t<int64_t> *pw = rw + 2 * n_rest + 1, *sw = pw + 2 * n_p + 1;
#pragma unroll
            for (int d = 0; d < kCondMaxRest; ++d) {
                int64_t row = -1;
                for (int k = 0; k < n_p; ++k)
                    if (pw[2 * k + 1] == d) row = pw[2 * k];
                if constexpr (kWeigh) {
                    int64_t lrow = -1;
                    for (int k = 0; k < n_s; ++k)
                        if (sw[2 * k + 1] == d) lrow = sw[2 * k];
                    srow[d] = (int32_t)lrow;
                }
                pd[d] = row >= 0;
#pragma unroll
                for (int j = 0; j < V; ++j) pv[d][j] = -1;
                if (pd[d] && live) load_n<int32_t, V, false, true>(ev + row * R + b, pv[d]);
            }
        }
        // the odometer at the chunk's first rest entry (uniform)
        const int64_t r0 = rc * kCondRestChunk;
        const int64_t r1 = r0 + kCondRestChunk < n_r ? r0 + kCondRestChunk : n_r;
        int64_t dig[kCondMaxRest];
        int64_t off = 0, q = r0;
#pragma unroll
        for (int d = 0; d < kCondMaxRest; ++d) {
            dig[d] = 0;
            if (d < n_rest) {
                const int64_t c = rw[2 * d];
                dig[d] = q % c;
                q /= c;
                off += dig[d] * rw[2 * d + 1];
            }
        }
        for (int64_t r = r0; r < r1; r += kCondBatchU) {
            int64_t offs[kCondBatchU];
            int32_t lr[kCondBatchU][kWeigh ? kCondMaxRest : 1];    // per entry (uniform): a soft dim's row of lam
            bool hit[kCondBatchU][V];
#pragma unroll
            for (int u = 0; u < kCondBatchU; ++u) {
                offs[u] = off;
#pragma unroll
                for (int j = 0; j < V; ++j) hit[u][j] = true;
                if constexpr (kMask) {
#pragma unroll
                    for (int d = 0; d < kCondMaxRest; ++d) {
                        if constexpr (kWeigh) lr[u][d] = srow[d] + (int32_t)dig[d];
                        if (pd[d]) {
                            const int32_t digit = (int32_t)dig[d];
#pragma unroll
                            for (int j = 0; j < V; ++j) hit[u][j] = hit[u][j] && (pv[d][j] < 0 || pv[d][j] == digit);
                        }
                    }
                }
                bool carry = true;
#pragma unroll
                for (int d = 0; d < kCondMaxRest; ++d) {
                    if (carry && d < n_rest) {
                        const int64_t c = rw[2 * d], st = rw[2 * d + 1];
                        ++dig[d];
                        off += st;
                        if (dig[d] == c) {
                            dig[d] = 0;
                            off -= c * st;
                        } else {
                            carry = false;
                        }
                    }
                }
            }
            T x[kCondBatchU][V];
#pragma unroll
            for (int u = 0; u < kCondBatchU; ++u)
                if (live && r + u < r1) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        if constexpr (kMask) x[u][j] = hit[u][j] ? gload(src + base[j] + offs[u]) : T(0);
                        else x[u][j] = gload(src + base[j] + offs[u]);
                    }
                }
            // the scope's order, left to right: the slowest rest dim first; one dim's weights live at a time
            if constexpr (kWeigh) {
#pragma unroll
                for (int d = kCondMaxRest - 1; d >= 0; --d)
                    if (srow[d] >= 0) {
                        T w[kCondBatchU][V];
#pragma unroll
                        for (int u = 0; u < kCondBatchU; ++u)
                            if (live && r + u < r1) load_n<T, V, false, true>(lam + (int64_t)lr[u][d] * R + b, w[u]);
#pragma unroll
                        for (int u = 0; u < kCondBatchU; ++u)
                            if (live && r + u < r1) {
#pragma unroll
                                for (int j = 0; j < V; ++j) x[u][j] = x[u][j] * w[u][j];
                            }
                    }
            }
#pragma unroll
            for (int u = 0; u < kCondBatchU; ++u)
                if (live && r + u < r1) store_n<T, V, false, true>(out + (r + u) * R + b, x[u]);
        }
    }
}

// The gather step of a batch plan: tables and their metadata from `meta`.  The
// gathered table carries the source's exp2 and maxbits -- the bound the single
// call's conditioned view of the same table carries; a mask zeroes entries and
// the weights are at most 1, so it stays a valid bound in every form.  Lam is
// `const void *` in the weighted form and empty in the others: lam is an argument
// of the form that reads it alone, and the arguments of each form stay one
// contiguous run of the kernel-argument segment.
template <typename T, int V, int Form, typename... Lam>
__global__ __launch_bounds__(kBlock) void cond_batch_kernel(const int64_t *pool_, TableMeta *meta, int out_table,
                                                            const int32_t *ev, Lam... lam_, int64_t R) {
    static_assert(sizeof...(Lam) == (Form == kCondWeighted ? 1 : 0), "lam is the weighted form's argument");
    const void *lam = nullptr;
    if constexpr (sizeof...(Lam) > 0) lam = (lam_, ...);
    cst_t<int64_t> *pool = as_const(pool_);
    const int src_table = (int)pool[0];
    cst_t<TableMeta> &ms = *as_const(meta + src_table);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        meta[out_table].exp2 = ms.exp2;
        meta[out_table].maxbits = ms.maxbits;
    }
    cond_batch<T, V, Form>(pool, static_cast<const T *>(ms.ptr), static_cast<T *>(as_const(meta + out_table)->ptr), ev,
                           static_cast<const T *>(lam), R);
}

// One gather with its metadata in the kernel-argument segment (bnpp_condition_batch, _mv, _sv).  The weighted
// kernels take CondBatchArgs as it is, the others the same without lam, for the same reason as above
struct CondBatchArgsNoLam {
    int64_t pool[cond_single_pool_words(kCondWeighted)];
    const void *src;
    void *out;
    const int32_t *ev;
    int64_t n_rows;
    static constexpr const void *lam = nullptr;
    explicit CondBatchArgsNoLam(const CondBatchArgs &a) : src(a.src), out(a.out), ev(a.ev), n_rows(a.n_rows) {
        for (int i = 0; i < cond_single_pool_words(kCondWeighted); ++i) pool[i] = a.pool[i];
    }
};
template <int Form>
using cond_single_args_t = std::conditional_t<Form == kCondWeighted, CondBatchArgs, CondBatchArgsNoLam>;
template <typename T, int V, int Form>
__global__ __launch_bounds__(kBlock) void cond_batch_single_kernel(const cond_single_args_t<Form> args) {
    using Args = cond_single_args_t<Form>;
#if defined(__HIP_DEVICE_COMPILE__)
    (void)args;
    cst_t<Args> &a = *(cst_t<Args> *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    cst_t<Args> &a = *(cst_t<Args> *)&args;
#endif
    cond_batch<T, V, Form>(a.pool, static_cast<const T *>(a.src), static_cast<T *>(a.out), a.ev,
                           static_cast<const T *>(a.lam), a.n_rows);
}

// persistent: the grid capped like the other persistent launches
template <int V>
static inline int64_t cond_batch_grid(int64_t rest, int64_t R, int max_grid) {
    const int64_t nbb = (R / V + kBlock - 1) / kBlock, nrc = (rest + kCondRestChunk - 1) / kCondRestChunk;
    const int64_t blocks = nbb * nrc;
    return blocks < 1 ? 1 : blocks < max_grid ? blocks : max_grid;
}
// wide accesses: R a multiple of 16 bytes of T, every address 16-byte aligned
template <typename T>
static inline bool cond_batch_wide(int64_t R, const void *a, const void *b) {
    constexpr int V = 16 / (int)sizeof(T);
    return R % V == 0 && (reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 16 == 0;
}

// the launchers, one instantiation per translation unit (k_condb*_f32/f64.hip); the weighted form's wide accesses
// need lam 16-byte aligned too
template <typename T, int V, int Form>
static void cond_batch_launch(const int64_t *pool, int64_t rest, TableMeta *meta, int out_table, const int32_t *ev,
                              const void *lam, int64_t R, int max_grid, hipStream_t stream) {
    const dim3 grid((unsigned)cond_batch_grid<V>(rest, R, max_grid));
    if constexpr (Form == kCondWeighted)
        hipLaunchKernelGGL((cond_batch_kernel<T, V, Form, const void *>), grid, dim3(kBlock), 0, stream, pool, meta, out_table,
                           ev, lam, R);
    else
        hipLaunchKernelGGL((cond_batch_kernel<T, V, Form>), grid, dim3(kBlock), 0, stream, pool, meta, out_table, ev, R);
}
template <typename T, int Form>
hipError_t go_cond_batch(const int64_t *pool, int64_t rest, TableMeta *meta, int out_table, const void *out_ptr,
                         const int32_t *ev, const void *lam, int64_t R, int max_grid, hipStream_t stream) {
    constexpr int V = 16 / (int)sizeof(T);
    if (cond_batch_wide<T>(R, out_ptr, ev) && (Form != kCondWeighted || cond_batch_wide<T>(R, lam, lam)))
        cond_batch_launch<T, V, Form>(pool, rest, meta, out_table, ev, lam, R, max_grid, stream);
    else
        cond_batch_launch<T, 1, Form>(pool, rest, meta, out_table, ev, lam, R, max_grid, stream);
    return hipGetLastError();
}
template <typename T, int Form>
hipError_t go_cond_batch_single(const CondBatchArgs &a, int max_grid, hipStream_t stream) {
    constexpr int V = 16 / (int)sizeof(T);
    const cond_single_args_t<Form> k(a);
    if (cond_batch_wide<T>(a.n_rows, a.out, a.ev) && (Form != kCondWeighted || cond_batch_wide<T>(a.n_rows, a.lam, a.lam)))
        hipLaunchKernelGGL((cond_batch_single_kernel<T, V, Form>),
                           dim3((unsigned)cond_batch_grid<V>(a.pool[3], a.n_rows, max_grid)), dim3(kBlock), 0, stream, k);
    else
        hipLaunchKernelGGL((cond_batch_single_kernel<T, 1, Form>),
                           dim3((unsigned)cond_batch_grid<1>(a.pool[3], a.n_rows, max_grid)), dim3(kBlock), 0, stream, k);
    return hipGetLastError();
}

}  // namespace bnpp
