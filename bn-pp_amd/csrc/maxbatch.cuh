// The traceback of a batched max-product run (gfx950): R assignments at once.
//
// mpe_decode_kernel (maxout.cuh) is one workgroup walking one assignment, a
// barrier per tree depth.  Here a lane owns one evidence row b and walks the
// decode rows in reverse elimination order -- a bucket after every bucket
// that maximises one of its separator variables -- so a lane reads only what
// it wrote itself: no barrier, no atomics, no LDS.
//
//   for each decode row (arg table A, variable v, separator (u_j, stride_j)):
//       off = sum_j x[u_j][b] * stride_j   (+ b when A carries the row variable)
//       x[v][b] = A[off]
//
// x = uint8[n_vars][R], variable-major: a wave reads and writes 64 consecutive
// rows of one variable as one 64-byte run.  The arg read is one contiguous run
// of 64 bytes when the separator is empty apart from B, a per-lane gather from
// a table that is usually cache-resident otherwise, and one broadcast byte
// where the table carries no B and has no separator.  The kernel writes the
// rows of the maximised variables only: evidence variables never appear in a
// separator (the gather steps removed them), the host fills them in.
//
// The row words are wave-uniform: they stay in the dims pool and are read
// through the scalar path (as cond_batch_kernel reads its words), so the
// per-row cost in vector instructions is n byte loads, n multiply-adds, one
// byte load and one byte store.  An arg byte is below its variable's card, so
// every offset stays inside its table by construction of the strides.
//
// Work: virtual blocks of BLOCK rows, walked grid-stride by a persistent grid.
//
// pool (int64 words, plan.cpp build_decode_batch_desc):
//   [0] n_vars  [1] n_rows  [2] R  [3] 0
//   per row: arg table, eliminated variable, carries B (0 / 1), n, n x (variable, stride)
#pragma once
#include "kernels.cuh"

namespace bnpp {

template <int BLOCK>   // a template so that the header defines no symbol: instantiated in k_max_f64.hip
__global__ __launch_bounds__(BLOCK) void mpe_decode_batch_kernel(const int64_t *pool_, const TableMeta *meta, uint8_t *x,
                                                                  int64_t R) {
    cst_t<int64_t> *pool = as_const(pool_);
    const int n_rows = (int)pool[1];
    const int64_t n_vb = (R + BLOCK - 1) / BLOCK;
    for (int64_t vb = blockIdx.x; vb < n_vb; vb += gridDim.x) {
        const int64_t b = vb * BLOCK + threadIdx.x;
        const bool live = b < R;
        uint8_t *xb = x + b;
        cst_t<int64_t> *row = pool + 4;                    // uniform: the walk is the same in every lane
        for (int r = 0; r < n_rows; ++r) {
            const int n = (int)row[3];
            if (live) {                                    // a lane past R reads and writes nothing
                const uint8_t *arg = static_cast<const uint8_t *>(as_const(meta + row[0])->ptr);
                int64_t off = row[2] ? b : 0;
                for (int j = 0; j < n; ++j) off += (int64_t)gload(xb + row[4 + 2 * j] * R) * row[5 + 2 * j];
                *(gbl_t<uint8_t> *)(xb + row[1] * R) = gload(arg + off);
            }
            row += 4 + 2 * n;
        }
    }
}

// persistent: the grid capped like the other persistent launches
static inline hipError_t go_mpe_decode_batch(const int64_t *pool, const TableMeta *meta, uint8_t *x, int64_t R, int max_grid,
                                             hipStream_t stream) {
    const int64_t blocks = (R + kBlock - 1) / kBlock;
    const int64_t grid = blocks < 1 ? 1 : blocks < max_grid ? blocks : max_grid;
    hipLaunchKernelGGL(mpe_decode_batch_kernel<kBlock>, dim3((unsigned)grid), dim3(kBlock), 0, stream, pool, meta, x, R);
    return hipGetLastError();
}

}  // namespace bnpp
