// Max-product bucket kernels and the MPE traceback (gfx950).
//
// A max bucket is the generic bucket (kernels.cuh) with `max` in place of the
// sum over the eliminated variable, and a second output: per output entry the
// value of the eliminated variable at which the maximum sat.
//
//   best = p(v = 0);  arg = 0
//   for v in 1 .. k-1:
//       p = ((1 * in_0) * in_1) ...          chain order, each product rounded
//       if p > best:  best = p;  arg = v     strict: ties keep the lowest v
//
// out[e] = best (rescaled and max-tracked exactly as the sum kernels do: max
// commutes with an exact power-of-two scale), arg[e] one byte in the table
// BucketDesc::aux_out.  Tiles are V1 x 1 (V1 = 1, 2, 4): a tile's arg bytes are
// one 8-, 16- or 32-bit store, so a wave's arg store is one contiguous run.
// The kernels are their own family (their own register budget: the running
// arg per tile entry); the sum kernels' source and code are untouched.
//
// mpe_decode_kernel turns the arg tables into one assignment: one workgroup
// walks the elimination tree root first, one tree depth per step.
#pragma once
#include "kernels.cuh"

namespace bnpp {

// One V1 x 1 output tile: its mixed-radix position decoded once, then the
// chain product per value of the eliminated variable, loads batched as in
// compute_tile.  Returns the tile's largest value.
template <typename T, int NIN, int V1, bool O32>
__device__ __forceinline__ T compute_max_tile(const LoadedBucketT<NIN> &b, int64_t tid, T (&best)[V1], uint32_t &argw) {
    using O = toff_t<O32>;
    O pos[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) pos[i] = (O)b.base[i];
    if (b.n_dims > 0) {
        uint64_t q, r;
        divmod_dim((uint64_t)tid, b.t0h, b.t0m, q, r);
        int64_t i0 = (int64_t)r * V1;
#pragma unroll
        for (int i = 0; i < NIN; ++i) pos[i] += (O)i0 * (O)b.s0[i];
        if (b.n_dims > 1) {
            uint64_t q1, r1;
            divmod_dim(q, b.t1h, b.t1m, q1, r1);
#pragma unroll
            for (int i = 0; i < NIN; ++i) pos[i] += (O)r1 * (O)b.s1[i];
            uint64_t rem = q1;
            const int row = 2 + b.n_in;                  // dims-pool row length
            const __attribute__((address_space(4))) int64_t *dp =
                (const __attribute__((address_space(4))) int64_t *)(b.dims + 2 * row);
            for (int j = 2; j < b.n_dims; ++j) {
                uint64_t qq, rr;
                divmod_dim(rem, dp[0], dp[1], qq, rr);
#pragma unroll
                for (int i = 0; i < NIN; ++i)
                    if (i < b.n_in) pos[i] += (O)rr * (O)dp[2 + i];
                rem = qq;
                dp += row;
            }
        }
    }
    uint32_t arg[V1];
#pragma unroll
    for (int j = 0; j < V1; ++j) {
        best[j] = T(0);
        arg[j] = 0;
    }
    constexpr int VB = V1 * NIN >= 16 ? 1 : 16 / (V1 * NIN);
    for (int v0 = 0; v0 < b.k; v0 += VB) {
        T x[VB][NIN][V1];
#pragma unroll
        for (int vv = 0; vv < VB; ++vv) {
            const O v = (O)(v0 + vv);
#pragma unroll
            for (int i = 0; i < NIN; ++i)
                if (VB == 1 || v0 + vv < b.k)              // uniform
                    load_tile<T, V1, 1, O32>(static_cast<const T *>(b.ptr[i]), pos[i] + v * (O)b.es[i], b.s0[i],
                                             b.s1[i], x[vv][i]);
        }
#pragma unroll
        for (int vv = 0; vv < VB; ++vv)
#pragma unroll
            for (int i = 0; i < NIN; ++i)
                if (v0 + vv < b.k && i < b.n_in) expand_tile<T, V1, 1>(x[vv][i], b.s0[i], b.s1[i]);
#pragma unroll
        for (int vv = 0; vv < VB; ++vv) {
            if (v0 + vv < b.k) {                           // uniform
                T p[V1];
#pragma unroll
                for (int j = 0; j < V1; ++j) p[j] = T(1);
#pragma unroll
                for (int i = 0; i < NIN; ++i) {
                    if (i >= b.n_in) continue;             // uniform
#pragma unroll
                    for (int j = 0; j < V1; ++j) p[j] = p[j] * x[vv][i][j];
                }
                if (v0 + vv == 0) {                        // uniform: best = p(v = 0)
#pragma unroll
                    for (int j = 0; j < V1; ++j) best[j] = p[j];
                } else {
#pragma unroll
                    for (int j = 0; j < V1; ++j) {
                        const bool up = p[j] > best[j];    // strict: a tie keeps the lower v
                        best[j] = up ? p[j] : best[j];
                        arg[j] = up ? (uint32_t)(v0 + vv) : arg[j];
                    }
                }
            }
        }
    }
    if (b.flags & kScale) {
#pragma unroll
        for (int j = 0; j < V1; ++j) best[j] = ldexp_t(best[j], b.neg_e);
    }
    argw = 0;
#pragma unroll
    for (int j = 0; j < V1; ++j) argw |= arg[j] << (8 * j);
    T m = T(0);
#pragma unroll
    for (int j = 0; j < V1; ++j) m = best[j] > m ? best[j] : m;
    return m;
}

// the tile's V1 arg bytes as one store (tile `tid` covers entries [tid * V1, tid * V1 + V1);
// arg tables are 256-B aligned, so the store is naturally aligned); read
// once, by the decode: nontemporal like the values
template <int V1>
__device__ __forceinline__ void store_arg(uint8_t *arg, int64_t tid, uint32_t argw) {
    if constexpr (V1 == 4) {
        gbl_t<uint32_t> *q = (gbl_t<uint32_t> *)(arg + tid * 4);
        __builtin_nontemporal_store(argw, q);
    } else if constexpr (V1 == 2) {
        gbl_t<uint16_t> *q = (gbl_t<uint16_t> *)(arg + tid * 2);
        __builtin_nontemporal_store((uint16_t)argw, q);
    } else {
        gbl_t<uint8_t> *q = (gbl_t<uint8_t> *)(arg + tid);
        __builtin_nontemporal_store((uint8_t)argw, q);
    }
}

template <typename T, int NIN, int V1, bool O32>
__global__ __launch_bounds__(kBlock) void max_level_kernel(const BucketDesc *__restrict__ descs, int n_desc,
                                                           const int64_t *__restrict__ pool,
                                                           TableMeta *__restrict__ meta, int64_t total_vblocks) {
    __shared__ T red[kBlock / 64];
    __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kLdsWaveBytes];
    LoadedBucketT<NIN> b;
    uint8_t *arg = nullptr;
    int cur = -1;
    int64_t cur_begin = 0;
    T lmax = T(0);
    for (int64_t vb = blockIdx.x; vb < total_vblocks; vb += gridDim.x) {
        int bi = n_desc == 1 ? 0 : find_bucket(descs, n_desc, vb);
        if (bi != cur) {
            if (cur >= 0) flush_max<T>(lmax, meta, descs[cur].out_table, descs[cur].flags, red);
            cur = bi;
            lmax = T(0);
            cst_t<BucketDesc> &d = *as_const(descs + bi);
            cur_begin = d.vblk_begin;
            load_common(b, d, pool + d.dim_off);
            b.flags = d.flags;
            b.out = meta[d.out_table].ptr;
            arg = static_cast<uint8_t *>(as_const(meta + d.aux_out)->ptr);
            int64_t e_sum = 0, x_sum = 0;
            for (int i = 0; i < NIN; ++i) {
                if (i < d.n_in) {
                    cst_t<TableMeta> &mi = *as_const(meta + d.in_table[i]);
                    b.ptr[i] = mi.ptr;
                    int e = FBits<T>::exponent(mi.maxbits);
                    if (d.flags & kScale) {
                        e_sum += e;
                        x_sum += mi.exp2 + e;
                    } else {
                        x_sum += mi.exp2;
                    }
                } else {
                    b.ptr[i] = b.out;                      // unused slot: entry 0 of the output, never used
                }
            }
            b.neg_e = (int)(-e_sum);
            if (vb == cur_begin && threadIdx.x == 0) meta[d.out_table].exp2 = x_sum;
        }
        const int64_t tid0 = (vb - cur_begin) * kBlock;
        const int64_t tid = tid0 + threadIdx.x;
        T best[V1];
        if (tid < b.n_tiles) {
            uint32_t argw;
            T m = compute_max_tile<T, NIN, V1, O32>(b, tid, best, argw);
            lmax = m > lmax ? m : lmax;
            store_arg<V1>(arg, tid, argw);
        }
        store_tiles<T, V1>(static_cast<T *>(b.out), tid0 + (threadIdx.x & ~63), b.n_tiles, best,
                           lds + (threadIdx.x >> 6) * kLdsWaveBytes);
    }
    if (cur >= 0) flush_max<T>(lmax, meta, descs[cur].out_table, descs[cur].flags, red);
}

// One max bucket with the descriptor in the kernel-argument segment (the
// single-op API, no rescaling); SingleArgs::arg_out may be null (values only).
template <typename T, int NIN, int V1, bool O32>
__global__ __launch_bounds__(kBlock) void max_single_kernel(const SingleArgs args) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)args;
    const SingleArgs &a = *(const __attribute__((address_space(4))) SingleArgs *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    const SingleArgs &a = args;
#endif
    const BucketDesc &d = a.d;
    LoadedBucketT<NIN> b;
    load_common(b, d, a.pool);
    b.flags = 0;
    b.neg_e = 0;
    b.out = a.meta[d.n_in].ptr;
    uint8_t *arg = static_cast<uint8_t *>(a.arg_out);
    for (int i = 0; i < NIN; ++i) b.ptr[i] = i < d.n_in ? a.meta[i].ptr : b.out;
    __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kLdsWaveBytes];
    for (int64_t tid0 = (int64_t)blockIdx.x * kBlock; tid0 < b.n_tiles; tid0 += (int64_t)gridDim.x * kBlock) {
        const int64_t tid = tid0 + threadIdx.x;
        T best[V1];
        if (tid < b.n_tiles) {
            uint32_t argw;
            (void)compute_max_tile<T, NIN, V1, O32>(b, tid, best, argw);
            if (arg) store_arg<V1>(arg, tid, argw);       // uniform
        }
        store_tiles<T, V1>(static_cast<T *>(b.out), tid0 + (threadIdx.x & ~63), b.n_tiles, best,
                           lds + (threadIdx.x >> 6) * kLdsWaveBytes);
    }
}

template <typename T, int NIN, int V1, bool O32>
static hipError_t go_max_level(const LevelArgs &a, int max_grid, hipStream_t stream) {
    int64_t grid = a.vblocks < max_grid ? a.vblocks : max_grid;
    hipLaunchKernelGGL((max_level_kernel<T, NIN, V1, O32>), dim3((unsigned)grid), dim3(kBlock), 0, stream, a.descs,
                       a.n_desc, a.pool, a.meta, a.vblocks);
    return hipGetLastError();
}

template <typename T, int NIN, int V1, bool O32>
static hipError_t go_max_single(const SingleArgs &a, int max_grid, hipStream_t stream) {
    int64_t blocks = (a.d.n_tiles + kBlock - 1) / kBlock;
    int64_t grid = blocks < max_grid ? blocks : max_grid;
    hipLaunchKernelGGL((max_single_kernel<T, NIN, V1, O32>), dim3((unsigned)grid), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

// the instantiated set: input classes 1/2/4/8 x tiles 1x1 2x1 4x1 x 32/64-bit
// offsets; build_desc (BucketSpec::max_out) chooses among exactly these
#define BNPP_MAX_TILES(X, T, NIN) X(T, NIN, 1) X(T, NIN, 2) X(T, NIN, 4)
#define BNPP_MAX_ALL(X, T) BNPP_MAX_TILES(X, T, 1) BNPP_MAX_TILES(X, T, 2) BNPP_MAX_TILES(X, T, 4) BNPP_MAX_TILES(X, T, 8)
#define BNPP_KEY_MAX(NIN, V1) (kMaxKeyBase + NIN * 64 + V1 * 8 + 1)
#define BNPP_LIST_MAX(T, NIN, V1) BNPP_KEY_MAX(NIN, V1), kGenericO32 + BNPP_KEY_MAX(NIN, V1),
#define BNPP_CASE_MAX_LEVEL(T, NIN, V1) \
    case BNPP_KEY_MAX(NIN, V1): return go_max_level<T, NIN, V1, false>(a, max_grid, stream); \
    case kGenericO32 + BNPP_KEY_MAX(NIN, V1): return go_max_level<T, NIN, V1, true>(a, max_grid, stream);
#define BNPP_CASE_MAX_SINGLE(T, NIN, V1) \
    case BNPP_KEY_MAX(NIN, V1): return go_max_single<T, NIN, V1, false>(a, max_grid, stream); \
    case kGenericO32 + BNPP_KEY_MAX(NIN, V1): return go_max_single<T, NIN, V1, true>(a, max_grid, stream);

// ------------------------------------------------------------------ decode
// The traceback of a max-product run.  pool (int64 words, plan.cpp
// decode_pool):
//   [0] n_vars  [1] n_rows  [2] n_depths  [3 .. 3 + n_depths] first row of each depth
//   then n_vars initial values (evidence, 0 elsewhere), n_rows row offsets
//   (relative to pool), and per row: arg table, eliminated variable, n, n x (var, stride).
// Rows are ordered by tree depth, roots first: a row's separator variables
// belong to rows of smaller depth (or are evidence), so one __syncthreads()
// per depth orders every read of x after its write.  x: int32[n_vars].
template <int BLOCK>   // a template so that the header defines no symbol: instantiated in k_max_f64.hip
__global__ __launch_bounds__(BLOCK) void mpe_decode_kernel(const int64_t *__restrict__ pool,
                                                            const TableMeta *__restrict__ meta, int32_t *__restrict__ x) {
    const int n_vars = (int)pool[0], n_depths = (int)pool[2];
    const int64_t *depth_at = pool + 3;
    const int64_t *init = depth_at + n_depths + 1;
    const int64_t *row_off = init + n_vars;
    for (int i = threadIdx.x; i < n_vars; i += BLOCK) x[i] = (int32_t)init[i];
    __syncthreads();
    for (int dp = 0; dp < n_depths; ++dp) {
        for (int64_t r = depth_at[dp] + threadIdx.x; r < depth_at[dp + 1]; r += BLOCK) {
            const int64_t *row = pool + row_off[r];
            const uint8_t *arg = static_cast<const uint8_t *>(meta[row[0]].ptr);
            const int n = (int)row[2];
            int64_t off = 0;
            for (int j = 0; j < n; ++j)
                off += (int64_t)__hip_atomic_load(x + row[3 + 2 * j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) *
                       row[4 + 2 * j];
            __hip_atomic_store(x + row[1], (int32_t)arg[off], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
    }
}

}  // namespace bnpp
