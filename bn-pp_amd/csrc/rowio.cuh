// Device-resident row input and output of the batched calls (gfx950): the four
// steps that take a launch's rows from the caller's device arrays and hand its
// results back to them, so that no value passes through the host.
//
//   stage_rows         ev  = int32[n_rows][n_ev]  ->  the launch's evidence table int32[n_ev][R]
//   stage_lik          lik = [n_rows][Ws]         ->  T[Ws][R] scaled per (row, variable) block, e_row[R]
//   stage_loglik       loglik = [n_rows][Ws]      ->  T[Ws][R] = exp(l - top) / 2, e_row[R], top[n_soft][R]
//   stage_weights      weights = double[n_rows]   ->  the launch's weights table double[R] (expected counts)
//   emit_row_scalars   the result table T[R]      ->  log10_z[row0 + b], z[row0 + b]
//   emit_row_logs      the result table T[R], top ->  ln_z, log10_z, z with the rows' shifts restored
//   emit_row_states    x = uint8[n_vars][K][R]    ->  int32[n_rows][n_vars] / uint8[n_rows][K][n_vars]
//
// row0 is the launch's first row, entry b of a launch is row min(row0 + b,
// n_rows - 1) (the last launch is padded with the call's last row), rows_live
// the launch's rows that are the call's.  include/bnpp.h states each step's
// arithmetic with its single-step entry (bnpp_stage_evidence_rows,
// bnpp_stage_likelihoods, bnpp_emit_row_scalars, bnpp_emit_row_states; the log
// forms: bnpp_stage_loglikelihoods, bnpp_emit_row_logs).
//
// A workgroup owns a tile of 64 rows and a persistent grid walks the tiles.
// Wherever rows are the fastest dimension (the evidence table, T, x, the
// result table) a lane owns a row and the accesses coalesce along b; the
// caller's arrays are row-major, so a wave there reads or writes runs of
// consecutive columns of one row.  The turn between the two goes through an
// LDS tile [64 rows][C columns] whose row pitch P makes both phases free of
// bank conflicts (a 32-lane half of a wave is served at once and must fall on
// distinct banks; 4-byte and every store access: 32 banks of a dword; 8-byte
// loads: 64 banks):
//
//   int32 tiles (stage_rows, the MPE form of emit_row_states): C = 32, P = 33
//     dwords.  Row-wise phase: 32 consecutive lanes touch 32 consecutive
//     dwords of one row, 32 distinct banks at any pitch.  Lane-owns-row phase:
//     lane l touches dword 33 l + c, bank (l + c) mod 32: distinct for 32
//     consecutive l.
//   byte tile (the sampling form of emit_row_states): C = 64, P = 68 bytes = 17
//     dwords.  Fill: lane l stores a byte of dword 17 l + c / 4, bank
//     (17 l + c / 4) mod 32, distinct for 32 consecutive l as 17 is odd.
//     Flush: 64 lanes read the 64 consecutive bytes of one row, 16 consecutive
//     dwords, the four lanes of a dword reading one address (a broadcast).
//   fp64 tile (stage_lik): C = 16, P = 17 doubles, margrows.cuh's tile with the
//     phases swapped.  Fill: 16 consecutive lanes store 16 consecutive doubles
//     of one row, 32 consecutive dwords, all 32 banks once.  Lane-owns-row
//     loads: lane l reads dwords 34 l + 2 c and the next, and 34 l mod 64 =
//     2 (17 l mod 32) takes 32 distinct even values for 32 consecutive l: 32
//     distinct bank pairs of the 64 banks a load sees.
//
// Every tile is private to its wave (the waves split the columns), so a wave
// synchronises with itself only; stage_lik alone meets at a workgroup barrier,
// to add the waves' exponent sums of a row.  The only values shared between
// workgroups are the status words, folded by a 64-bit atomic minimum that
// only an invalid cell touches: results do not depend on the grid.  Plain C++
// and vector memory operations throughout.
//
// The per-column descriptor is one int64 word per column read through the
// scalar cache: from device memory (the _dv calls), or from the
// kernel-argument segment behind the arguments (the single-step entries).
#pragma once
#include "rowio_dev.cuh"

namespace bnpp {

constexpr int kRowioWaves = kBlock / 64;
constexpr int kRowioC32 = 32, kRowioP32 = 33;       // int32 tiles: columns, pitch in dwords
constexpr int kRowioC8 = 64, kRowioP8 = 68;         // byte tile: columns, pitch in bytes
constexpr int kRowioC64 = 16, kRowioP64 = 17;       // fp64 tile: columns, pitch in doubles

// the step's arguments and its descriptor words, both in the kernel-argument segment unless a.words says otherwise
template <typename A>
__device__ __forceinline__ cst_t<RowioSingle<A>> &rowio_args(const RowioSingle<A> &args) {
    return kernarg_of(args);
}

// the wave's LDS stores are visible to its own later loads (and the other way round)
__device__ __forceinline__ void rowio_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- stage_rows ----------------------------------------------------------------------------------------------
// The waves split the chunks of 32 columns.  Fill: the two halves of a wave read 32 consecutive columns of two
// rows; a value outside its column's range is flagged and stored as 0.  Flush: a lane owns a row.
__global__ __launch_bounds__(kBlock) void stage_rows_kernel(const RowioSingle<StageRowsArgs> args) {
    __shared__ int32_t tiles[kRowioWaves][64 * kRowioP32];
    cst_t<RowioSingle<StageRowsArgs>> &s = rowio_args(args);
    cst_t<int64_t> *w = s.a.words ? as_const(s.a.words) : s.single;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int32_t *tile = tiles[wv];
    const gbl_t<int32_t> *ev = (const gbl_t<int32_t> *)s.a.ev;
    gbl_t<int32_t> *out = (gbl_t<int32_t> *)s.a.out;
    const int64_t n_rows = s.a.n_rows, row0 = s.a.row0, R = s.a.R, n_ev = s.a.n_ev;
    const int64_t n_tiles = (R + 63) / 64, n_chunks = (n_ev + kRowioC32 - 1) / kRowioC32;
    const int cc = lane & 31, half = lane >> 5;
    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t b0 = tl * 64;
        for (int64_t ch = wv; ch < n_chunks; ch += kRowioWaves) {
            const int64_t j0 = ch * kRowioC32, j = j0 + cc;
            const int n = n_ev - j0 < kRowioC32 ? (int)(n_ev - j0) : kRowioC32;
            int64_t card = 0;
            bool partial = false;
            if (cc < n) {
                const int64_t word = w[j];
                card = word & 0xffffffff;
                partial = (word >> 32) & 1;
            }
            for (int r = half; r < 64; r += 2) {
                const int64_t b = b0 + r;
                if (cc < n && b < R) {
                    const int64_t row = row0 + b < n_rows - 1 ? row0 + b : n_rows - 1;
                    int32_t v = ev[row * n_ev + j];
                    if (!((v >= 0 && v < card) || (v == -1 && partial))) {
                        rowio_flag(s.a.status, 0, row * n_ev + j);
                        v = 0;
                    }
                    tile[r * kRowioP32 + cc] = v;
                }
            }
            rowio_wave_sync();
            if (b0 + lane < R)
                for (int c = 0; c < n; ++c) out[(j0 + c) * R + b0 + lane] = tile[lane * kRowioP32 + c];
            rowio_wave_sync();
        }
    }
}

// ---- stage_lik -----------------------------------------------------------------------------------------------
// columns [col, col + n) of the tile's 64 rows into the wave's tile, widened to double: 16 lanes per row
__device__ __forceinline__ void lik_fill(double *tile, cst_t<StageLikArgs> &a, int64_t b0, int64_t col, int n, int lane) {
    const int cc = lane & (kRowioC64 - 1), q = lane >> 4;
    for (int r = q; r < 64; r += 4) {
        const int64_t b = b0 + r;
        if (cc < n && b < a.R) {
            const int64_t row = a.row0 + b < a.n_rows - 1 ? a.row0 + b : a.n_rows - 1, at = row * a.Ws + col + cc;
            tile[r * kRowioP64 + cc] = a.lik_f32 ? (double)gload(static_cast<const float *>(a.lik) + at)
                                                 : gload(static_cast<const double *>(a.lik) + at);
        }
    }
    rowio_wave_sync();
}

__device__ __forceinline__ void lik_store(cst_t<StageLikArgs> &a, int64_t at, double v) {
    if (a.out_f32) *((gbl_t<float> *)a.out + at) = lik_to_float(v);
    else *((gbl_t<double> *)a.out + at) = v;
}

// The waves split the soft variables into contiguous runs.  A wave takes as many whole blocks as fit the 16
// columns of its tile at once; a block wider than the tile passes through it in chunks twice, its maximum
// taken first.  A lane owns a row: its block's top, exponent and scaled entries, stored along b.  The log form
// also stores the block's top, per variable: the emit step sums a row's tops in soft_vars order, so the sum does
// not depend on how the waves split the variables
template <bool kLog>
__device__ __forceinline__ void stage_lik_body(cst_t<RowioSingle<StageLikArgs>> &s) {
    __shared__ double tiles[kRowioWaves][64 * kRowioP64];
    __shared__ int64_t esum[kRowioWaves][64];
    cst_t<StageLikArgs> &a = s.a;
    constexpr double kFloor = kLog ? -__builtin_inf() : 0.0;
    cst_t<int64_t> *w = a.words ? as_const(a.words) : s.single;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *tile = tiles[wv];
    const int64_t R = a.R, n_soft = a.n_soft;
    const int64_t i0 = n_soft * wv / kRowioWaves, i1 = n_soft * (wv + 1) / kRowioWaves;
    const int64_t n_tiles = (R + 63) / 64;
    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t b0 = tl * 64, b = b0 + lane;
        const bool live = b < R;
        const int64_t row = a.row0 + b < a.n_rows - 1 ? a.row0 + b : a.n_rows - 1;
        int64_t e_sum = 0;
        for (int64_t i = i0; i < i1;) {
            const int64_t k = w[i] & 0xffffffff, col = w[i] >> 32;
            if (k > kRowioC64) {
                double top = kFloor;
                for (int64_t c0 = 0; c0 < k; c0 += kRowioC64) {
                    const int n = k - c0 < kRowioC64 ? (int)(k - c0) : kRowioC64;
                    lik_fill(tile, a, b0, col + c0, n, lane);
                    for (int x = 0; live && x < n; ++x) {
                        double v = tile[lane * kRowioP64 + x];
                        if (lik_invalid<kLog>(v)) {
                            rowio_flag(a.status, 1, row * a.Ws + col + c0 + x);
                            v = kFloor;
                        }
                        top = v > top ? v : top;
                    }
                    rowio_wave_sync();
                }
                const int e = lik_exponent<kLog>(top);
                e_sum += e;
                if (kLog && live) *((gbl_t<double> *)a.top + i * R + b) = top;
                for (int64_t c0 = 0; c0 < k; c0 += kRowioC64) {
                    const int n = k - c0 < kRowioC64 ? (int)(k - c0) : kRowioC64;
                    lik_fill(tile, a, b0, col + c0, n, lane);
                    for (int x = 0; live && x < n; ++x) {
                        const double v = tile[lane * kRowioP64 + x];
                        lik_store(a, (col + c0 + x) * R + b, lik_scaled<kLog>(v, top, e));
                    }
                    rowio_wave_sync();
                }
                ++i;
            } else {
                int64_t i2 = i;
                int n = 0;
                while (i2 < i1 && n + (w[i2] & 0xffffffff) <= kRowioC64) n += (int)(w[i2++] & 0xffffffff);
                lik_fill(tile, a, b0, col, n, lane);
                int x0 = 0;
                for (; i < i2; ++i) {
                    const int kk = (int)(w[i] & 0xffffffff);
                    double top = kFloor;
                    for (int x = 0; live && x < kk; ++x) {
                        double v = tile[lane * kRowioP64 + x0 + x];
                        if (lik_invalid<kLog>(v)) {
                            rowio_flag(a.status, 1, row * a.Ws + col + x0 + x);
                            v = kFloor;
                        }
                        top = v > top ? v : top;
                    }
                    const int e = lik_exponent<kLog>(top);
                    e_sum += e;
                    if (kLog && live) *((gbl_t<double> *)a.top + i * R + b) = top;
                    for (int x = 0; live && x < kk; ++x) {
                        const double v = tile[lane * kRowioP64 + x0 + x];
                        lik_store(a, (col + x0 + x) * R + b, lik_scaled<kLog>(v, top, e));
                    }
                    x0 += kk;
                }
                rowio_wave_sync();
            }
        }
        esum[wv][lane] = e_sum;
        __syncthreads();
        if (wv == 0 && live) {
            int64_t e = 0;
            for (int q = 0; q < kRowioWaves; ++q) e += esum[q][lane];
            *((gbl_t<int64_t> *)a.e_row + b) = e;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void stage_lik_kernel(const RowioSingle<StageLikArgs> args) {
    stage_lik_body<false>(rowio_args(args));
}
__global__ __launch_bounds__(kBlock) void stage_loglik_kernel(const RowioSingle<StageLikArgs> args) {
    stage_lik_body<true>(rowio_args(args));
}

// ---- emit_row_scalars ----------------------------------------------------------------------------------------
// log10(p * 2^ex) as the host's log10_scaled takes it: of the split frexp gives, every operation rounded once;
// 0x1.34413509f79ffp-2 is the double log10(2.0) folds to
__device__ __forceinline__ double rowio_log10_scaled(double p, int64_t ex) {
    int pe = 0;
    const double pm = frexp(p, &pe);
    return p > 0 ? __dadd_rn(log10(pm), __dmul_rn((double)(ex + pe), 0x1.34413509f79ffp-2)) : -__builtin_inf();
}

// a row with p <= 0 is impossible: counted with an integer atomic add, whose result no order changes
__device__ __forceinline__ void rowio_count_impossible(int64_t *counter, double p) {
    if (counter && !(p > 0)) atomicAdd(reinterpret_cast<unsigned long long *>(counter), 1ull);
}

// ---- stage_weights -------------------------------------------------------------------------------------------
// a lane owns a row: the launch's weights, padding rows 0, no weights 1; a weight that is not finite or is
// negative is flagged in status word 2 and stored as 0
__global__ __launch_bounds__(64) void stage_weights_kernel(const StageWeightsArgs a) {
    for (int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x; b < a.R; b += (int64_t)gridDim.x * 64) {
        const int64_t row = a.row0 + b;
        double w = 0.0;
        if (row < a.n_rows) {
            w = a.weights ? gload(a.weights + row) : 1.0;
            if (!(w >= 0) || w == __builtin_inf()) {
                rowio_flag(a.status, 2, row);
                w = 0.0;
            }
        }
        *((gbl_t<double> *)a.out + b) = w;
    }
}

// a lane owns a row: nothing to turn, so a workgroup is the one wave of its tile
__global__ __launch_bounds__(64) void emit_scalars_kernel(const EmitScalarsArgs a) {
    for (int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x; b < a.rows_live; b += (int64_t)gridDim.x * 64) {
        double p = 0;
        p = __dadd_rn(p, rowio_elem(a.table, a.is_f32, a.has_b ? b : 0));
        rowio_count_impossible(a.n_impossible, p);
        int64_t ex = a.meta ? as_const(a.meta)->exp2 : 0;
        if (a.e_row) ex += gload(a.e_row + b);
        if (a.log10_z) *((gbl_t<double> *)a.log10_z + a.row0 + b) = rowio_log10_scaled(p, ex);
        if (a.z) {
            const int64_t c = ex > (1 << 20) ? (1 << 20) : ex < -(1 << 20) ? -(1 << 20) : ex;
            *((gbl_t<double> *)a.z + a.row0 + b) = ldexp(p, (int)c);
        }
    }
}

// The log form: the row's shift is the sum of its blocks' tops, taken from 0.0 in soft_vars order, and goes back
// to the natural and the decimal log; 0x1.62e42fefa39efp-1 is ln 2, 0x1.bcb7b1526e50ep-2 log10(e).  z = exp(ln_z)
// may overflow.  Each output may be null
__global__ __launch_bounds__(64) void emit_logs_kernel(const EmitScalarsArgs a) {
    for (int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x; b < a.rows_live; b += (int64_t)gridDim.x * 64) {
        double p = 0;
        p = __dadd_rn(p, rowio_elem(a.table, a.is_f32, a.has_b ? b : 0));
        int64_t ex = a.meta ? as_const(a.meta)->exp2 : 0;
        if (a.e_row) ex += gload(a.e_row + b);
        double shift = 0.0;
        for (int64_t i = 0; i < a.n_soft; ++i) shift = __dadd_rn(shift, gload(a.top + i * a.R + b));
        if (a.table_shift) shift = __dadd_rn(shift, gload(a.table_shift));
        rowio_count_impossible(a.n_impossible, p);
        int pe = 0;
        const double pm = frexp(p, &pe), pw = (double)(ex + pe), ninf = -__builtin_inf();
        const double ln_z = p > 0 ? __dadd_rn(__dadd_rn(log(pm), __dmul_rn(pw, 0x1.62e42fefa39efp-1)), shift) : ninf;
        if (a.ln_z) *((gbl_t<double> *)a.ln_z + a.row0 + b) = ln_z;
        if (a.log10_z)
            *((gbl_t<double> *)a.log10_z + a.row0 + b) =
                p > 0 ? __dadd_rn(__dadd_rn(log10(pm), __dmul_rn(pw, 0x1.34413509f79ffp-2)), __dmul_rn(shift, 0x1.bcb7b1526e50ep-2))
                      : ninf;
        if (a.z) *((gbl_t<double> *)a.z + a.row0 + b) = exp(ln_z);
    }
}

// ---- emit_row_states -----------------------------------------------------------------------------------------
// The waves split the (draw, chunk of C variables) pairs.  Fill: a lane owns a row and takes, per variable, the
// row's observed evidence value, else the state byte, else 0.  Flush: the lanes write C consecutive variables
// of one row (the byte form) or of two (the int32 form).
template <typename OutT, int C, int P>
__device__ __forceinline__ void emit_states(cst_t<RowioSingle<EmitStatesArgs>> &s) {
    __shared__ OutT tiles[kRowioWaves][64 * P];
    cst_t<EmitStatesArgs> &a = s.a;
    cst_t<int64_t> *w = a.words ? as_const(a.words) : s.single;
    constexpr bool sampling = sizeof(OutT) == 1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    OutT *tile = tiles[wv];
    const gbl_t<uint8_t> *x = (const gbl_t<uint8_t> *)a.x;
    const gbl_t<int32_t> *ev = (const gbl_t<int32_t> *)a.ev;
    gbl_t<OutT> *out = (gbl_t<OutT> *)a.out;
    const int64_t nv = a.n_vars, K = a.K, R = a.R, rows_live = a.rows_live;
    const int64_t n_tiles = (rows_live + 63) / 64, n_chunks = (nv + C - 1) / C, n_items = K * n_chunks;
    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t b0 = tl * 64, b = b0 + lane;
        const bool live = b < rows_live;
        const int n_live = rows_live - b0 < 64 ? (int)(rows_live - b0) : 64;
        bool impossible = false;
        if (sampling && live) impossible = !(rowio_elem(a.table, a.is_f32, a.has_b ? b : 0) > 0);
        if (sampling && wv == 0 && live && a.n_degenerate)
            *((gbl_t<int64_t> *)a.n_degenerate + a.row0 + b) = impossible ? K * a.n_drawn : (int64_t)gload(a.deg + b);
        for (int64_t it = wv; out && it < n_items; it += kRowioWaves) {
            const int64_t sd = it / n_chunks, v0 = (it - sd * n_chunks) * C;
            const int n = nv - v0 < C ? (int)(nv - v0) : C;
            for (int c = 0; c < n; ++c) {
                const int64_t word = w[v0 + c];
                const int32_t col = (int32_t)(word & 0xffffffff);
                const bool written = (word >> 33) & 1;
                int32_t val = -1, st = 0;
                if (live && col >= 0) val = ev[(int64_t)col * R + b];
                if (live && written && !impossible) st = x[((v0 + c) * K + sd) * R + b];
                tile[lane * P + c] = (OutT)(val >= 0 ? val : st);
            }
            rowio_wave_sync();
            constexpr int kRowsPer = 64 / C;
            const int cc = lane & (C - 1), q = lane / C;
            for (int r = q; r < n_live; r += kRowsPer)
                if (cc < n) out[((a.row0 + b0 + r) * K + sd) * nv + v0 + cc] = tile[r * P + cc];
            rowio_wave_sync();
        }
    }
}

__global__ __launch_bounds__(kBlock) void emit_states_mpe_kernel(const RowioSingle<EmitStatesArgs> args) {
    emit_states<int32_t, kRowioC32, kRowioP32>(rowio_args(args));
}
__global__ __launch_bounds__(kBlock) void emit_states_sample_kernel(const RowioSingle<EmitStatesArgs> args) {
    emit_states<uint8_t, kRowioC8, kRowioP8>(rowio_args(args));
}

}  // namespace bnpp
