// Host-side launchers: route a descriptor to the translation unit that holds
// its kernel instantiation (k_generic_f32/f64, k_stream_f32/f64, k_slab_f32/f64,
// k_chain_f32/f64, k_max_f32/f64, k_sample_f32/f64, k_condb_f32/f64,
// k_counts_f32/f64, k_margrows_f32/f64).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bnpp_device.h"
#include "runtime.hpp"

namespace bnpp {

hipError_t dispatch_level_f32(int key, const LevelArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_single_f32(int key, const SingleArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_level_f64(int key, const LevelArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_single_f64(int key, const SingleArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_stream_level_f32(int key, const LevelArgs &a, int small_elems, int max_grid, hipStream_t stream);
hipError_t dispatch_stream_single_f32(int key, const SingleArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_stream_level_f64(int key, const LevelArgs &a, int small_elems, int max_grid, hipStream_t stream);
hipError_t dispatch_stream_single_f64(int key, const SingleArgs &a, int max_grid, hipStream_t stream);

hipError_t dispatch_chain_level_f32(int key, const LevelArgs &a, int small_elems, int max_grid, int grid_cap,
                                    hipStream_t stream);
hipError_t dispatch_chain_level_f64(int key, const LevelArgs &a, int small_elems, int max_grid, int grid_cap,
                                    hipStream_t stream);

hipError_t dispatch_max_level_f32(int key, const LevelArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_max_level_f64(int key, const LevelArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_max_single_f32(int key, const SingleArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_max_single_f64(int key, const SingleArgs &a, int max_grid, hipStream_t stream);

hipError_t dispatch_sample_rows_f32(const int64_t *pool, const TableMeta *meta, uint8_t *x, int64_t n, int64_t first,
                                    uint64_t seed, unsigned long long *n_degenerate, int max_grid, hipStream_t stream);
hipError_t dispatch_sample_rows_f64(const int64_t *pool, const TableMeta *meta, uint8_t *x, int64_t n, int64_t first,
                                    uint64_t seed, unsigned long long *n_degenerate, int max_grid, hipStream_t stream);
hipError_t dispatch_sample_rows_batch_f32(const int64_t *pool, const TableMeta *meta, uint8_t *x, unsigned long long *deg_rows,
                                          int64_t lanes, const SampleBatchLaunch &a, int max_grid, hipStream_t stream);
hipError_t dispatch_sample_rows_batch_f64(const int64_t *pool, const TableMeta *meta, uint8_t *x, unsigned long long *deg_rows,
                                          int64_t lanes, const SampleBatchLaunch &a, int max_grid, hipStream_t stream);
hipError_t dispatch_sample_single_f32(const SampleSingleArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_sample_single_f64(const SampleSingleArgs &a, int max_grid, hipStream_t stream);

// condbatch.cuh: one form and one type instantiated per unit (k_condb, k_condbm, k_condbs _f32/f64)
template <typename T, int Form>
hipError_t go_cond_batch(const int64_t *pool, int64_t rest, TableMeta *meta, int out_table, const void *out_ptr,
                         const int32_t *ev, const void *lam, int64_t n_rows, int max_grid, hipStream_t stream);
template <typename T, int Form>
hipError_t go_cond_batch_single(const CondBatchArgs &a, int max_grid, hipStream_t stream);

hipError_t dispatch_counts_f32(const CountsArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_counts_f64(const CountsArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_counts_list_f32(const CountsArgs *list, int n, int64_t rows_max, int64_t rest_max, int max_grid,
                                    hipStream_t stream);
hipError_t dispatch_counts_list_f64(const CountsArgs *list, int n, int64_t rows_max, int64_t rest_max, int max_grid,
                                    hipStream_t stream);

hipError_t dispatch_marg_rows_f32(const int64_t *pool, const TableMeta *meta, const int32_t *ev, double *out,
                                  int64_t rows_live, int max_grid, hipStream_t stream);
hipError_t dispatch_marg_rows_f64(const int64_t *pool, const TableMeta *meta, const int32_t *ev, double *out,
                                  int64_t rows_live, int max_grid, hipStream_t stream);
hipError_t dispatch_marg_rows_single_f32(const MargRowsSingleArgs &a, int max_grid, hipStream_t stream);
hipError_t dispatch_marg_rows_single_f64(const MargRowsSingleArgs &a, int max_grid, hipStream_t stream);

hipError_t dispatch_slab_single_f32(int key, const SingleArgs &a, hipStream_t stream);
hipError_t dispatch_slab_single_f64(int key, const SingleArgs &a, hipStream_t stream);
hipError_t dispatch_slab_level_f32(int key, const LevelArgs &a, hipStream_t stream);
hipError_t dispatch_slab_level_f64(int key, const LevelArgs &a, hipStream_t stream);

// the keys of each dispatch switch above (the generic and stream switches hold
// the same keys for single-op and level launches)
void keys_generic_f32(std::vector<int> &keys);
void keys_generic_f64(std::vector<int> &keys);
void keys_stream_f32(std::vector<int> &keys);
void keys_stream_f64(std::vector<int> &keys);
void keys_slab_f32(int level, std::vector<int> &keys);
void keys_slab_f64(int level, std::vector<int> &keys);
void keys_chain_f32(std::vector<int> &keys);
void keys_chain_f64(std::vector<int> &keys);
void keys_max_f32(std::vector<int> &keys);
void keys_max_f64(std::vector<int> &keys);

// Result tables out of the arena: blockIdx.x picks the table, the
// kCopyParts workgroups along y share it grid-stride (a multi-GB
// variable_elimination result would crawl through one workgroup); 16-B moves
// while both ends allow them (tables are 256-B aligned in the arena and the
// results buffer), 4-B ones for the tail (sizes are whole fp32 / fp64 entries).
constexpr int kCopyParts = 64;
__global__ __launch_bounds__(256) void copy_tables_kernel(const CopyItem *__restrict__ items, int n) {
    const CopyItem c = items[blockIdx.x];
    const int64_t n16 = c.bytes / 16;
    const int64_t first = (int64_t)blockIdx.y * blockDim.x + threadIdx.x, step = (int64_t)gridDim.y * blockDim.x;
    const uint4 *s16 = static_cast<const uint4 *>(c.src);
    uint4 *d16 = static_cast<uint4 *>(c.dst);
    for (int64_t i = first; i < n16; i += step) d16[i] = s16[i];
    const uint32_t *s4 = static_cast<const uint32_t *>(c.src);
    uint32_t *d4 = static_cast<uint32_t *>(c.dst);
    for (int64_t i = n16 * 4 + first; i < c.bytes / 4; i += step) d4[i] = s4[i];
    (void)n;
}

hipError_t launch_copies(const CopyItem *items, int n, int64_t max_bytes, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    // a workgroup per 64 KiB of the largest table, up to kCopyParts
    const int64_t parts = std::min<int64_t>(kCopyParts, std::max<int64_t>(1, max_bytes >> 16));
    hipLaunchKernelGGL(copy_tables_kernel, dim3((unsigned)n, (unsigned)parts), dim3(256), 0, stream, items, n);
    return hipGetLastError();
}

hipError_t launch_single(int is_f32, const SingleArgs &a, int max_grid, hipStream_t stream) {
    if (a.d.n_tiles <= 0) return hipSuccess;
    const SingleKey sk = single_key(is_f32, a);
    if (sk.family == kFamSlab)
        return is_f32 ? dispatch_slab_single_f32(sk.key, a, stream) : dispatch_slab_single_f64(sk.key, a, stream);
    if (sk.family == kFamStream)
        return is_f32 ? dispatch_stream_single_f32(sk.key, a, max_grid, stream)
                      : dispatch_stream_single_f64(sk.key, a, max_grid, stream);
    return is_f32 ? dispatch_single_f32(sk.key, a, max_grid, stream) : dispatch_single_f64(sk.key, a, max_grid, stream);
}

hipError_t launch_max_single(int is_f32, const SingleArgs &a, int max_grid, hipStream_t stream) {
    if (a.d.n_tiles <= 0) return hipSuccess;
    const SingleKey sk = max_single_key(is_f32, a);
    return is_f32 ? dispatch_max_single_f32(sk.key, a, max_grid, stream) : dispatch_max_single_f64(sk.key, a, max_grid, stream);
}

hipError_t launch_sample_rows(int is_f32, const int64_t *pool, const TableMeta *meta, uint8_t *x, int64_t n,
                              int64_t first, uint64_t seed, unsigned long long *n_degenerate, int max_grid,
                              hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    return is_f32 ? dispatch_sample_rows_f32(pool, meta, x, n, first, seed, n_degenerate, max_grid, stream)
                  : dispatch_sample_rows_f64(pool, meta, x, n, first, seed, n_degenerate, max_grid, stream);
}

hipError_t launch_sample_rows_batch(int is_f32, const int64_t *pool, const TableMeta *meta, uint8_t *x,
                                    unsigned long long *deg_rows, int64_t lanes, const SampleBatchLaunch &a, int max_grid,
                                    hipStream_t stream) {
    if (lanes <= 0 || a.n_valid <= 0) return hipSuccess;
    return is_f32 ? dispatch_sample_rows_batch_f32(pool, meta, x, deg_rows, lanes, a, max_grid, stream)
                  : dispatch_sample_rows_batch_f64(pool, meta, x, deg_rows, lanes, a, max_grid, stream);
}

hipError_t launch_sample_single(int is_f32, const SampleSingleArgs &a, int max_grid, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    return is_f32 ? dispatch_sample_single_f32(a, max_grid, stream) : dispatch_sample_single_f64(a, max_grid, stream);
}

template <typename T>
static hipError_t cond_batch_form(int form, const int64_t *pool, int64_t rest, TableMeta *meta, int out_table,
                                  const void *out_ptr, const int32_t *ev, const void *lam, int64_t n_rows, int max_grid,
                                  hipStream_t stream) {
    switch (form) {
    case kCondPlain: return go_cond_batch<T, kCondPlain>(pool, rest, meta, out_table, out_ptr, ev, lam, n_rows, max_grid, stream);
    case kCondMasked: return go_cond_batch<T, kCondMasked>(pool, rest, meta, out_table, out_ptr, ev, lam, n_rows, max_grid, stream);
    case kCondWeighted: return go_cond_batch<T, kCondWeighted>(pool, rest, meta, out_table, out_ptr, ev, lam, n_rows, max_grid, stream);
    }
    return hipErrorInvalidValue;
}
template <typename T>
static hipError_t cond_batch_single_form(int form, const CondBatchArgs &a, int max_grid, hipStream_t stream) {
    switch (form) {
    case kCondPlain: return go_cond_batch_single<T, kCondPlain>(a, max_grid, stream);
    case kCondMasked: return go_cond_batch_single<T, kCondMasked>(a, max_grid, stream);
    case kCondWeighted: return go_cond_batch_single<T, kCondWeighted>(a, max_grid, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_cond_batch(int is_f32, int form, const int64_t *pool, int64_t rest, TableMeta *meta, int out_table,
                             const void *out_ptr, const int32_t *ev, const void *lam, int64_t n_rows, int max_grid,
                             hipStream_t stream) {
    if (n_rows <= 0 || rest <= 0) return hipSuccess;
    return is_f32 ? cond_batch_form<float>(form, pool, rest, meta, out_table, out_ptr, ev, lam, n_rows, max_grid, stream)
                  : cond_batch_form<double>(form, pool, rest, meta, out_table, out_ptr, ev, lam, n_rows, max_grid, stream);
}

hipError_t launch_cond_batch_single(int is_f32, int form, const CondBatchArgs &a, int max_grid, hipStream_t stream) {
    if (a.n_rows <= 0) return hipSuccess;
    return is_f32 ? cond_batch_single_form<float>(form, a, max_grid, stream)
                  : cond_batch_single_form<double>(form, a, max_grid, stream);
}

hipError_t launch_counts(int is_f32, const CountsArgs &a, int max_grid, hipStream_t stream) {
    if (a.rows_live <= 0 || a.n_rest_entries <= 0) return hipSuccess;
    return is_f32 ? dispatch_counts_f32(a, max_grid, stream) : dispatch_counts_f64(a, max_grid, stream);
}

hipError_t launch_counts_list(int is_f32, const CountsArgs *list, int n, int64_t rows_max, int64_t rest_max,
                              int max_grid, hipStream_t stream) {
    if (n <= 0 || rows_max <= 0 || rest_max <= 0) return hipSuccess;
    return is_f32 ? dispatch_counts_list_f32(list, n, rows_max, rest_max, max_grid, stream)
                  : dispatch_counts_list_f64(list, n, rows_max, rest_max, max_grid, stream);
}

hipError_t launch_marg_rows(int is_f32, const int64_t *pool, const TableMeta *meta, const int32_t *ev, double *out,
                            int64_t rows_live, int max_grid, hipStream_t stream) {
    if (rows_live <= 0) return hipSuccess;
    return is_f32 ? dispatch_marg_rows_f32(pool, meta, ev, out, rows_live, max_grid, stream)
                  : dispatch_marg_rows_f64(pool, meta, ev, out, rows_live, max_grid, stream);
}

hipError_t launch_marg_rows_single(int is_f32, const MargRowsSingleArgs &a, int max_grid, hipStream_t stream) {
    if (a.rows_live <= 0) return hipSuccess;
    return is_f32 ? dispatch_marg_rows_single_f32(a, max_grid, stream) : dispatch_marg_rows_single_f64(a, max_grid, stream);
}

void kernel_keys(int is_f32, int level, int family, std::vector<int> &keys) {
    if (family == kFamGeneric) is_f32 ? keys_generic_f32(keys) : keys_generic_f64(keys);
    else if (family == kFamStream) is_f32 ? keys_stream_f32(keys) : keys_stream_f64(keys);
    else if (family == kFamSlab) is_f32 ? keys_slab_f32(level, keys) : keys_slab_f64(level, keys);
    else if (family == kFamMax) is_f32 ? keys_max_f32(keys) : keys_max_f64(keys);
    else if (family == kFamChain && level) is_f32 ? keys_chain_f32(keys) : keys_chain_f64(keys);   // runs are level launches only
}

hipError_t launch_level(int is_f32, int variant, const BucketDesc *descs, int n_desc, const int64_t *pool,
                        TableMeta *meta, int64_t total_vblocks, int small_elems, int max_grid, int grid_cap,
                        hipStream_t stream) {
    if (n_desc <= 0 || total_vblocks <= 0) return hipSuccess;
    LevelArgs a{descs, n_desc, pool, meta, total_vblocks};
    if (variant >= kMaxKeyBase)                         // max-product buckets (maxout.cuh)
        return is_f32 ? dispatch_max_level_f32(variant, a, max_grid, stream) : dispatch_max_level_f64(variant, a, max_grid, stream);
    if (variant >= 16384)                               // slab form: flat grid, one workgroup per virtual block
        return is_f32 ? dispatch_slab_level_f32(variant, a, stream) : dispatch_slab_level_f64(variant, a, stream);
    if (variant >= 8192)
        return is_f32 ? dispatch_chain_level_f32(variant, a, small_elems, max_grid, grid_cap, stream)
                      : dispatch_chain_level_f64(variant, a, small_elems, max_grid, grid_cap, stream);
    if (variant >= 4096)
        return is_f32 ? dispatch_stream_level_f32(variant, a, small_elems, max_grid, stream)
                      : dispatch_stream_level_f64(variant, a, small_elems, max_grid, stream);
    return is_f32 ? dispatch_level_f32(variant, a, max_grid, stream) : dispatch_level_f64(variant, a, max_grid, stream);
}

}  // namespace bnpp
