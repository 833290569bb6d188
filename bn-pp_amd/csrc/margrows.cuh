// Batched marginals (gfx950): every target's table normalised row by row and
// laid out row-major, out = double[R][W].
//
//   c                 = sum over x, ascending, sequentially from 0.0, of (double)T_j[x][b]
//   out[b][off_j + x] = (double)T_j[x][b] / c              (c == 0: 0/0 = NaN, nothing special-cased)
//   evidence block    : 1.0 at the row's value (clamped into range), 0.0 elsewhere
//   free block        : 1.0 / card
//   rows b >= rows_live are not written
//
// T_j is target j's table over (x, b), b fastest, R rows per launch: entry
// x * R + b (a table no evidence reaches has no b: entry x, the same for every
// row).  All arithmetic is fp64 on values converted
// from the table, every operation rounded once (no contraction): run_batch's
// host normalisation, moved to the device (include/bnpp.h,
// bnpp_bucket_marginal_rows, states it).
//
// A workgroup owns a tile of 64 rows (a persistent grid walks the tiles); its
// four waves split the targets into contiguous runs, so each wave owns a
// contiguous range of output columns.  A lane owns a row: the loads of
// T_j[x][b] coalesce along b.  The normalised values go into the wave's LDS
// tile [64 rows][kMargCols columns], filled with one target after another, and
// whenever the tile is full (and after the wave's last target) it is flushed:
// 16 consecutive lanes store 16 consecutive columns (128 bytes) of one output
// row.  A target wider than the tile passes through it in chunks, c computed
// first.  The row pitch is kMargPitch = 17 doubles: the fill's 8-byte stores of
// 16 consecutive lanes (rows l, column fixed) fall on dwords 34 l + 2 x, 16
// distinct bank pairs of the 32 banks a store sees; the flush reads rows r,
// r + 16, r + 32, r + 48 in the four 16-lane quarters, and 34 * 16 = 32 (mod
// 64) puts the two rows of a 32-lane half on opposite halves of the 64 banks a
// load sees: neither phase has a bank conflict.  The tile is private to its
// wave, so the waves never meet at a barrier and a wave's trip counts may
// differ from its neighbours'.  No atomics, nothing shared between workgroups:
// the result does not depend on the grid.
//
// The column blocks are words read through the scalar cache: the emit step's
// rows of the dims pool (plan.cpp build_marg_rows_desc; tables by id, their
// addresses from the table metadata), or the kernel-argument segment
// (bnpp_bucket_marginal_rows; tables by address).
//   [0] n_targets  [1] R  [2] W  [3] evidence table (unused here)
//   per block: table (id, or address; none: -1, or 0), card, carries B, row of ev (-1: none), first column
#pragma once
#include "kernels.cuh"

namespace bnpp {

constexpr int kMargCols = 16;                   // columns of a wave's tile
constexpr int kMargPitch = kMargCols + 1;       // its row pitch, in doubles
constexpr int kMargWaves = kBlock / 64;

// the wave's LDS stores are visible to its own later loads (and the other way round)
__device__ __forceinline__ void marg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// columns [col0, col0 + n) of rows [b0, b0 + n_live) from the wave's tile
__device__ __forceinline__ void marg_flush(double *tile, gbl_t<double> *out, int64_t W, int64_t b0, int n_live,
                                           int64_t col0, int n, int lane) {
    marg_wave_sync();
    const int cc = lane & (kMargCols - 1), q = lane >> 4;
    for (int r = 0; r < 16; ++r) {
        const int rr = r + 16 * q;
        if (cc < n && rr < n_live) out[(b0 + rr) * W + col0 + cc] = tile[rr * kMargPitch + cc];
    }
    marg_wave_sync();
}

template <typename T>
__device__ __forceinline__ void marg_rows(cst_t<int64_t> *w, cst_t<TableMeta> *meta, const int32_t *ev_, double *out_,
                                          int64_t rows_live) {
    __shared__ double tiles[kMargWaves][64 * kMargPitch];
    static_assert(kMargCols == 16, "marg_flush maps 16 lanes to a row");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *tile = tiles[wv];
    gbl_t<double> *out = (gbl_t<double> *)out_;
    const gbl_t<int32_t> *ev = (const gbl_t<int32_t> *)ev_;
    const int64_t n_targets = w[0], R = w[1], W = w[2];
    const int64_t j0 = n_targets * wv / kMargWaves, j1 = n_targets * (wv + 1) / kMargWaves;
    if (j0 >= j1) return;
    cst_t<int64_t> *blocks = w + kMargRowsPoolHead;
    const int64_t n_tiles = (rows_live + 63) / 64;
    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t b0 = tl * 64, b = b0 + lane;
        const bool live = b < rows_live;
        const int n_live = rows_live - b0 < 64 ? (int)(rows_live - b0) : 64;
        int fill = 0;
        int64_t col0 = blocks[kMargRowsColWords * j0 + 4];
        for (int64_t j = j0; j < j1; ++j) {
            cst_t<int64_t> *t = blocks + kMargRowsColWords * j;
            const int64_t card = t[1], ev_row = t[3];
            const bool belief = meta ? t[0] >= 0 : t[0] != 0;
            const T *tab = nullptr;
            if (belief) tab = meta ? static_cast<const T *>(meta[t[0]].ptr) : reinterpret_cast<const T *>(t[0]);
            const int64_t xs = t[2] ? R : 1, bo = t[2] ? b : 0;      // T_j[x][b] at x * R + b; without b at x
            double c = 0.0;
            int64_t val = -1;
            if (belief && live) {
                for (int64_t x = 0; x < card; ++x) c = __dadd_rn(c, (double)gload(tab + x * xs + bo));
            } else if (!belief && ev_row >= 0 && live) {
                const int64_t v = ev[ev_row * R + b];
                val = v < 0 ? 0 : v > card - 1 ? card - 1 : v;
            }
            const double u = __ddiv_rn(1.0, (double)card);
            for (int64_t x = 0; x < card; ++x) {
                double v = u;
                if (belief) v = live ? __ddiv_rn((double)gload(tab + x * xs + bo), c) : 0.0;
                else if (ev_row >= 0) v = x == val ? 1.0 : 0.0;
                tile[lane * kMargPitch + fill] = v;
                if (++fill == kMargCols) {
                    marg_flush(tile, out, W, b0, n_live, col0, kMargCols, lane);
                    col0 += kMargCols;
                    fill = 0;
                }
            }
        }
        if (fill) marg_flush(tile, out, W, b0, n_live, col0, fill, lane);
    }
}

// The emit step of a batched-marginals plan: its words in the dims pool.
template <typename T>
__global__ __launch_bounds__(kBlock) void marg_rows_kernel(const int64_t *pool, const TableMeta *meta, const int32_t *ev,
                                                            double *out, int64_t rows_live) {
    marg_rows<T>(as_const(pool), as_const(meta), ev, out, rows_live);
}
// One call with its words in the kernel-argument segment (bnpp_bucket_marginal_rows).
template <typename T>
__global__ __launch_bounds__(kBlock) void marg_rows_single_kernel(const MargRowsSingleArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)args;
    cst_t<MargRowsSingleArgs> &a = *(cst_t<MargRowsSingleArgs> *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    cst_t<MargRowsSingleArgs> &a = *(cst_t<MargRowsSingleArgs> *)&args;
#endif
    marg_rows<T>(a.words, (cst_t<TableMeta> *)nullptr, a.ev, a.out, a.rows_live);
}

// persistent: a workgroup per tile of 64 rows, capped like the other persistent launches
inline unsigned marg_rows_grid(int64_t rows_live, int max_grid) {
    const int64_t g = (rows_live + 63) / 64;
    return (unsigned)(g < 1 ? 1 : g < max_grid ? g : max_grid);
}
template <typename T>
static hipError_t go_marg_rows(const int64_t *pool, const TableMeta *meta, const int32_t *ev, double *out,
                               int64_t rows_live, int max_grid, hipStream_t stream) {
    hipLaunchKernelGGL((marg_rows_kernel<T>), dim3(marg_rows_grid(rows_live, max_grid)), dim3(kBlock), 0, stream, pool,
                       meta, ev, out, rows_live);
    return hipGetLastError();
}
template <typename T>
static hipError_t go_marg_rows_single(const MargRowsSingleArgs &a, int max_grid, hipStream_t stream) {
    hipLaunchKernelGGL((marg_rows_single_kernel<T>), dim3(marg_rows_grid(a.rows_live, max_grid)), dim3(kBlock), 0,
                       stream, a);
    return hipGetLastError();
}

}  // namespace bnpp
