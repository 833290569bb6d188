// Posterior sampling from the messages of a forward elimination pass (gfx950).
//
// After plan_ve's forward pass the inputs of x_i's bucket are P(x_i | separator)
// up to a constant, so drawing every variable from its bucket in REVERSE
// elimination order gives one exact joint sample of P(x | evidence).  One
// thread owns one sample and walks all rows for it: the dependent chain is per
// thread, no synchronisation between rows.  State: x = uint8[n_vars][n_samples],
// variable-major (a wave's read of one variable is 64 contiguous bytes).
//
// One draw, for variable X of k values with inputs in_0 .. in_{n-1} (include/bnpp.h):
//   p_v = ((1 * in_0[..]) * in_1[..]) ...     dtype T, each product rounded
//   c_v = c_{v-1} + (double)p_v               fp64, in order of v
//   t   = u * c_{k-1};   value = the lowest v with c_v > t   (none: 0, counted)
// The sums run twice (the total, then the walk): recomputation gives identical
// bits, and k can be 256.  Rows of k <= VB values keep their p_v in registers
// between the two (BNPP_SAMPLE_KEEP, on by default).  Loads of all inputs for
// VB consecutive v are issued before the first product uses one.
// Messages are stored scaled by exact powers of two; every p_v of one draw
// shares the scale and c_v > u * c_{k-1} is invariant under it: exp2 is never read.
//
// u: Philox4x32-10, key (seed lo, seed hi), counter (g lo, g hi, X, 0) with
// g = first_sample + s the global sample index: a sample depends on (seed, g) only.
//
// Row metadata is wave-uniform and read through the scalar cache (cst_t).  pool
// (int64 words, plan.cpp build_sample_desc):
//   [0] n_vars  [1] n_rows  [2] n_ev  [3] 0
//   n_ev x (variable, evidence value): rows of x filled before the walk
//   then per row, in reverse elimination order:
//     X, k, n_in, then per input: table, base offset, stride of X (0: absent),
//     n, n x (variable, stride) -- the eliminating bucket's view as emitted
// Table reads are per-lane gathers at 64-bit offsets.
#pragma once
#include "kernels.cuh"

#ifndef BNPP_SAMPLE_KEEP
#define BNPP_SAMPLE_KEEP 1
#endif

namespace bnpp {

__device__ __forceinline__ double philox_u01(uint64_t seed, uint64_t g, uint32_t var) {
    uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = var, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (double)((((uint64_t)c0 << 32) | c1) >> 11) * 0x1p-53;
}

// One row for one sample: NIN input slots (n_in <= NIN, uniform), VB values of
// X per batch of loads.  w: the row's first input; returns past the row.
// BATCH: an input has one more word, the stride of the row variable B, and the
// lane's row b enters its offset (sample_rows_batch_kernel below).
template <typename T, int NIN, int VB, bool BATCH = false>
__device__ __forceinline__ cst_t<int64_t> *draw_row(cst_t<int64_t> *w, cst_t<TableMeta> *meta, const gbl_t<uint8_t> *x,
                                                    int64_t n, int64_t s, int k, int n_in, double u, int &val,
                                                    int64_t b = 0) {
    constexpr int H = BATCH ? 5 : 4;                       // words before an input's (variable, stride) pairs
    const T *ptr[NIN];
    int64_t es[NIN], pos[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        ptr[i] = nullptr;
        es[i] = 0;
        pos[i] = 0;
        if (i < n_in) {                                    // uniform
            ptr[i] = static_cast<const T *>(meta[w[0]].ptr);
            es[i] = w[2];
            const int nd = (int)w[H - 1];
            int64_t off = w[1];
            if (BATCH) off += b * w[3];
            w += H;
#pragma unroll 4
            for (int j = 0; j < nd; ++j) off += (int64_t)x[w[2 * j] * n + s] * w[2 * j + 1];
            w += 2 * nd;
            pos[i] = off;
        }
    }
    auto batch = [&](int v0, T(&p)[VB]) {
        T xv[VB][NIN];
#pragma unroll
        for (int vv = 0; vv < VB; ++vv)
#pragma unroll
            for (int i = 0; i < NIN; ++i)
                if (i < n_in && v0 + vv < k) xv[vv][i] = gload(ptr[i] + pos[i] + (int64_t)(v0 + vv) * es[i]);   // uniform
#pragma unroll
        for (int vv = 0; vv < VB; ++vv) {
            T q = T(1);
#pragma unroll
            for (int i = 0; i < NIN; ++i)
                if (i < n_in && v0 + vv < k) q = q * xv[vv][i];
            p[vv] = q;
        }
    };
    T p[VB];
    double c = 0.0;
    for (int v0 = 0; v0 < k; v0 += VB) {
        batch(v0, p);
#pragma unroll
        for (int vv = 0; vv < VB; ++vv)
            if (v0 + vv < k) c = c + (double)p[vv];
    }
    const double t = u * c;
    val = -1;
    double a = 0.0;
    if (BNPP_SAMPLE_KEEP != 0 && k <= VB) {                // the one batch is still in registers
#pragma unroll
        for (int vv = 0; vv < VB; ++vv)
            if (vv < k) {
                a = a + (double)p[vv];
                val = val < 0 && a > t ? vv : val;
            }
    } else {
        for (int v0 = 0; v0 < k; v0 += VB) {
            batch(v0, p);
#pragma unroll
            for (int vv = 0; vv < VB; ++vv)
                if (v0 + vv < k) {
                    a = a + (double)p[vv];
                    val = val < 0 && a > t ? v0 + vv : val;
                }
        }
    }
    return w;
}

// All rows of `pool` for the samples [0, n) of this launch, 256 per workgroup
// and pass; x rows of other variables are read as this thread wrote them.
template <typename T>
__device__ __forceinline__ void sample_rows(cst_t<int64_t> *pool, cst_t<TableMeta> *meta, uint8_t *x_, int64_t n,
                                            int64_t first, uint64_t seed, unsigned long long *n_degenerate) {
    const int n_rows = (int)pool[1], n_ev = (int)pool[2];
    gbl_t<uint8_t> *x = (gbl_t<uint8_t> *)x_;
    unsigned deg = 0;
    for (int64_t s0 = (int64_t)blockIdx.x * kBlock; s0 < n; s0 += (int64_t)gridDim.x * kBlock) {
        const int64_t s = s0 + threadIdx.x;
        if (s >= n) continue;
        cst_t<int64_t> *w = pool + 4;
        for (int e = 0; e < n_ev; ++e, w += 2) x[w[0] * n + s] = (uint8_t)w[1];
        for (int r = 0; r < n_rows; ++r) {
            const int64_t X = w[0];
            const int k = (int)w[1], n_in = (int)w[2];
            w += 3;
            const double u = philox_u01(seed, (uint64_t)(first + s), (uint32_t)X);
            int val;
            if (n_in <= 2) w = draw_row<T, 2, 8>(w, meta, x, n, s, k, n_in, u, val);      // uniform
            else w = draw_row<T, kMaxIn, 2>(w, meta, x, n, s, k, n_in, u, val);
            if (val < 0) {                                 // c_{k-1} == 0 or NaN
                val = 0;
                ++deg;
            }
            x[X * n + s] = (uint8_t)val;
        }
    }
    if (deg && n_degenerate) atomicAdd(n_degenerate, (unsigned long long)deg);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void sample_rows_kernel(const int64_t *pool, const TableMeta *meta, uint8_t *x,
                                                             int64_t n, int64_t first, uint64_t seed,
                                                             unsigned long long *n_degenerate) {
    sample_rows<T>(as_const(pool), as_const(meta), x, n, first, seed, n_degenerate);
}

// ---- batched draws (bnpp_sample_batch): K samples for each of R evidence rows ----
// The messages of a batched plan carry the row variable B as their fastest
// dimension exactly where evidence reaches them.  Lane t in [0, R*K) owns
// (b, s) = (t % R, t / R): b fastest, as in the messages, so a wave reads 64
// consecutive B entries of a message wherever its separator values agree, and
// index t of each variable's row of x = uint8[n_vars][K][R] (64 contiguous
// bytes per wave).  The draw is draw_row's with b * (stride of B) added to each
// input's offset; u = philox_u01(seed, first + (row0 + b) * row_stride + s, X),
// so sample (b, s) has the bytes the single call draws for row b at that global
// index.  A lane of a padding row (b >= n_valid) reads and writes nothing.
// Degenerate draws are counted per row: one atomicAdd per lane that saw any,
// into deg_rows = int64[R], cleared by the launch.  No barrier, no LDS: a lane
// reads only what it wrote.  The kernel writes the sampled variables only
// (evidence variables never appear in a separator; the host fills them in).
// t % R is computed once per lane and pass of the persistent loop, one 64-bit
// division beside tens of draws; a 2-D loop over (s, b) would leave lanes idle
// whenever R is no multiple of the block, so it was not built.
// pool (plan.cpp build_sample_batch_desc):
//   [0] n_vars  [1] n_rows  [2] R  [3] K
//   per row: X, k, n_in, then per input: table, base offset, stride of X (0:
//   absent), stride of B (0: absent), n, n x (variable, stride)
template <typename T>
__global__ __launch_bounds__(kBlock) void sample_rows_batch_kernel(const int64_t *pool_, const TableMeta *meta_, uint8_t *x_,
                                                                   unsigned long long *deg_rows,
                                                                   const SampleBatchLaunch a) {
    cst_t<int64_t> *pool = as_const(pool_);
    cst_t<TableMeta> *meta = as_const(meta_);
    gbl_t<uint8_t> *x = (gbl_t<uint8_t> *)x_;
    const int n_rows = (int)pool[1];
    const int64_t R = pool[2], n = R * pool[3];
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t t = t0 + threadIdx.x;
        if (t >= n) continue;
        const int64_t s = t / R, b = t - s * R;
        if (b >= a.n_valid) continue;                      // a padding row
        const uint64_t g = (uint64_t)(a.first + (a.row0 + b) * a.row_stride + s);
        unsigned deg = 0;
        cst_t<int64_t> *w = pool + 4;
        for (int r = 0; r < n_rows; ++r) {
            const int64_t X = w[0];
            const int k = (int)w[1], n_in = (int)w[2];
            w += 3;
            const double u = philox_u01(a.seed, g, (uint32_t)X);
            int val;
            if (n_in <= 2) w = draw_row<T, 2, 8, true>(w, meta, x, n, t, k, n_in, u, val, b);   // uniform
            else w = draw_row<T, kMaxIn, 2, true>(w, meta, x, n, t, k, n_in, u, val, b);
            if (val < 0) {                                 // c_{k-1} == 0 or NaN
                val = 0;
                ++deg;
            }
            x[X * n + t] = (uint8_t)val;
        }
        if (deg) atomicAdd(deg_rows + b, (unsigned long long)deg);
    }
}

// One row with its metadata in the kernel-argument segment (bnpp_bucket_sample).
template <typename T>
__global__ __launch_bounds__(kBlock) void sample_single_kernel(const SampleSingleArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)args;
    cst_t<SampleSingleArgs> &a = *(cst_t<SampleSingleArgs> *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    cst_t<SampleSingleArgs> &a = *(cst_t<SampleSingleArgs> *)&args;
#endif
    sample_rows<T>(a.pool, a.meta, a.x, a.n, a.first, a.seed, a.n_degenerate);
}

// persistent: blocks of kBlock samples, capped like the other persistent launches
template <typename T>
static hipError_t go_sample_rows(const int64_t *pool, const TableMeta *meta, uint8_t *x, int64_t n, int64_t first,
                                 uint64_t seed, unsigned long long *n_degenerate, int max_grid, hipStream_t stream) {
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    const int64_t grid = blocks < max_grid ? blocks : max_grid;
    hipLaunchKernelGGL((sample_rows_kernel<T>), dim3((unsigned)grid), dim3(kBlock), 0, stream, pool, meta, x, n, first,
                       seed, n_degenerate);
    return hipGetLastError();
}
template <typename T>
static hipError_t go_sample_rows_batch(const int64_t *pool, const TableMeta *meta, uint8_t *x, unsigned long long *deg_rows,
                                       int64_t lanes, const SampleBatchLaunch &a, int max_grid, hipStream_t stream) {
    const int64_t blocks = (lanes + kBlock - 1) / kBlock;
    const int64_t grid = blocks < 1 ? 1 : blocks < max_grid ? blocks : max_grid;
    hipLaunchKernelGGL((sample_rows_batch_kernel<T>), dim3((unsigned)grid), dim3(kBlock), 0, stream, pool, meta, x, deg_rows,
                       a);
    return hipGetLastError();
}
template <typename T>
static hipError_t go_sample_single(const SampleSingleArgs &a, int max_grid, hipStream_t stream) {
    const int64_t blocks = (a.n + kBlock - 1) / kBlock;
    const int64_t grid = blocks < max_grid ? blocks : max_grid;
    hipLaunchKernelGGL((sample_single_kernel<T>), dim3((unsigned)grid), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace bnpp
