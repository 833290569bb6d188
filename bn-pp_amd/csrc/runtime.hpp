// Device runtime: context, source upload, schedule execution (HIP).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "bnpp_device.h"
#include "model_io.hpp"
#include "plan.hpp"

namespace bnpp {

hipError_t launch_level(int is_f32, int variant, const BucketDesc *descs, int n_desc, const int64_t *pool,
                        TableMeta *meta, int64_t total_vblocks, int small_elems, int max_grid, int grid_cap,
                        hipStream_t stream);

// single bucket with the descriptor passed by value (no device-side metadata,
// no rescaling): the exact Factor::product / sum_out / conditioning semantics.
constexpr int kMaxPool = 320;   // dims-pool words that fit the kernel-argument segment
struct SingleArgs {
    // slab form: the big input's first entry and summed-variable stride,
    // resolved on the host so the kernel's first loads wait on one kernarg read
    const void *big_ptr;
    int64_t big_es;
    BucketDesc d;
    TableMeta meta[kMaxIn + 1];  // inputs 0..n_in-1, output at index n_in
    int64_t pool[kMaxPool];
    // max buckets (maxout.cuh): the arg table, one byte per output entry (null: values only)
    void *arg_out;
};
hipError_t launch_single(int is_f32, const SingleArgs &a, int max_grid, hipStream_t stream);
// the kernel a single-op launch runs: family (0 generic, 1 stream, 2 slab) and
// the key its dispatcher switches on.  launch_single dispatches by it and
// bnpp_plan_single reports it, so the report is what launches
enum KernelFamily : int { kFamGeneric = 0, kFamStream = 1, kFamSlab = 2, kFamChain = 3, kFamMax = 4 };
struct SingleKey {
    int family, key;
};
inline SingleKey single_key(int is_f32, const SingleArgs &a) {
    if (a.d.big >= 0 && a.d.bcls == kBigSlab)
        return {kFamSlab, slab_key(a.d.k, a.d.v1, a.d.v2, a.d.lanes, 1, a.d.slab_y2 ? 8 : a.d.n_in)};
    if (a.d.big >= 0) return {kFamStream, stream_key(a.d.bcls, a.d.v1, a.d.v2, a.d.n_in)};
    int64_t in_bytes = 0;
    for (int i = 0; i < a.d.n_in && i < kMaxIn; ++i)
        in_bytes = in_bytes > a.meta[i].size * (is_f32 ? 4 : 8) ? in_bytes : a.meta[i].size * (is_f32 ? 4 : 8);
    return {kFamGeneric, variant_key(a.d.n_in, a.d.v1, a.d.v2) + (generic_o32(in_bytes) ? kGenericO32 : 0)};   // plan.hpp generic_variant
}
// a max bucket (BucketSpec::max_out; build_desc keeps it out of the stream
// and slab forms): the generic key of its shape above kMaxKeyBase
inline SingleKey max_single_key(int is_f32, const SingleArgs &a) {
    return {kFamMax, kMaxKeyBase + single_key(is_f32, a).key};
}
hipError_t launch_max_single(int is_f32, const SingleArgs &a, int max_grid, hipStream_t stream);
// the traceback of a max-product run (maxout.cuh mpe_decode_kernel): one workgroup
hipError_t launch_mpe_decode(const int64_t *pool, const TableMeta *meta, int32_t *x, hipStream_t stream);
// the traceback of a batched MPE plan (maxbatch.cuh): pool the step's words in
// the dims pool, x = uint8[n_vars][n_rows], a lane per row, the grid capped at max_grid
hipError_t launch_mpe_decode_batch(const int64_t *pool, const TableMeta *meta, uint8_t *x, int64_t n_rows, int max_grid,
                                   hipStream_t stream);
// posterior sampling (sample.cuh): all rows of a sampling step (pool: the
// step's words in the dims pool) for samples [0, n) of x = uint8[n_vars][n],
// global sample index first + s.  seed and first are launch arguments, not
// plan data; n_degenerate (device, may be null) is added to, never cleared
hipError_t launch_sample_rows(int is_f32, const int64_t *pool, const TableMeta *meta, uint8_t *x, int64_t n,
                              int64_t first, uint64_t seed, unsigned long long *n_degenerate, int max_grid,
                              hipStream_t stream);
// ... and one row with its metadata in the kernel-argument segment (bnpp_bucket_sample)
struct SampleSingleArgs {
    int64_t pool[kMaxPool];
    TableMeta meta[kMaxIn];
    uint8_t *x;
    int64_t n, first;
    uint64_t seed;
    unsigned long long *n_degenerate;
};
hipError_t launch_sample_single(int is_f32, const SampleSingleArgs &a, int max_grid, hipStream_t stream);
// batched draws (sample.cuh sample_rows_batch_kernel): the draw step of a
// batched sampling plan (pool: its words in the dims pool) for `lanes` = R * K
// lanes of x = uint8[n_vars][K][R]; deg_rows = int64[R] (device), added to,
// never cleared.  What varies per launch is launch data, not plan data: sample
// (b, s) draws at global index first + (row0 + b) * row_stride + s, and rows
// b >= n_valid are padding
struct SampleBatchLaunch {
    uint64_t seed;
    int64_t first, row_stride, row0, n_valid;
};
hipError_t launch_sample_rows_batch(int is_f32, const int64_t *pool, const TableMeta *meta, uint8_t *x,
                                    unsigned long long *deg_rows, int64_t lanes, const SampleBatchLaunch &a, int max_grid,
                                    hipStream_t stream);
// batched conditioning (condbatch.cuh): one gather step of a batch plan (pool:
// the step's words in the dims pool, rest: its rest entries) in one of the
// three forms (plan.hpp CondForm) into table out_table (at out_ptr) for the
// n_rows rows of ev = int32[.][n_rows]; lam = T[Ws][n_rows] is the weighted
// form's alone, null in the others
hipError_t launch_cond_batch(int is_f32, int form, const int64_t *pool, int64_t rest, TableMeta *meta, int out_table,
                             const void *out_ptr, const int32_t *ev, const void *lam, int64_t n_rows, int max_grid,
                             hipStream_t stream);
// ... and one gather with its metadata in the kernel-argument segment (bnpp_condition_batch, _mv, _sv): a form's
// pool holds at most cond_single_pool_words(form) words
struct CondBatchArgs {
    int64_t pool[cond_single_pool_words(kCondWeighted)];
    const void *src;
    void *out;
    const int32_t *ev;
    const void *lam;
    int64_t n_rows;
};
hipError_t launch_cond_batch_single(int is_f32, int form, const CondBatchArgs &a, int max_grid, hipStream_t stream);
// expected counts (counts.cuh): one factor's belief T over (rest, b) folded
// into its accumulator, normalised row by row (include/bnpp.h,
// bnpp_bucket_counts, states the arithmetic).  Everything by value in the
// kernel-argument segment; scratch holds 3 x 8 bytes per row
struct CountsArgs {
    const void *table;                  // T, b fastest (row stride n_rows, or 0 without B)
    const int32_t *ev;                  // int32[.][n_rows], variable-major (unused when n_e == 0)
    const double *weights;              // double[n_rows], null: all 1
    const void *valid;                  // table of the dtype, null: every row valid
    double *acc;                        // the factor's accumulator, natural layout over its scope
    void *scratch;
    int64_t n_rows, rows_live, n_rest_entries, n_keys;
    int32_t n_e, n_rest, has_b, valid_b;
    int64_t e_row[kCountsMaxDims], e_stride[kCountsMaxDims], e_card[kCountsMaxDims];   // evidence variables in the scope
    int64_t r_card[kCountsMaxDims], r_stride[kCountsMaxDims];                           // T's other dims, fastest first
};
constexpr int64_t kCountsScratchPerRow = 24;
// the arguments of one accumulate step from its pool words (plan.cpp
// build_counts_desc) and its device addresses; false: a malformed descriptor
bool counts_args(const int64_t *words, int64_t n_rows, int64_t rows_live, const void *table, const int32_t *ev,
                 const double *weights, const void *valid, double *acc, void *scratch, CountsArgs &a);
hipError_t launch_counts(int is_f32, const CountsArgs &a, int max_grid, hipStream_t stream);
// ... and n steps (device array, at most kCountsListMax, scratch of its own each) in one launch of each pass
constexpr int kCountsListMax = 65535;
hipError_t launch_counts_list(int is_f32, const CountsArgs *list, int n, int64_t rows_max, int64_t rest_max,
                              int max_grid, hipStream_t stream);
// batched marginals (margrows.cuh): the emit step of a batched-marginals plan
// (pool: its words in the dims pool) normalises every target's table row by
// row into out = double[R][W] for rows [0, rows_live) (include/bnpp.h,
// bnpp_bucket_marginal_rows, states the arithmetic); ev = int32[.][R]
hipError_t launch_marg_rows(int is_f32, const int64_t *pool, const TableMeta *meta, const int32_t *ev, double *out,
                            int64_t rows_live, int max_grid, hipStream_t stream);
// ... and one call with its words (tables by address, 0: none) in the kernel-argument segment
constexpr int kMargRowsSingleMax = 64;  // targets of a single-op call
struct MargRowsSingleArgs {
    int64_t words[kMargRowsPoolHead + kMargRowsColWords * kMargRowsSingleMax];
    const int32_t *ev;
    double *out;
    int64_t rows_live;
};
hipError_t launch_marg_rows_single(int is_f32, const MargRowsSingleArgs &a, int max_grid, hipStream_t stream);
// device-resident row input and output (rowio.cuh; include/bnpp.h states each step with its single-step entry).
// A step's descriptor is one int64 word per column, read through the scalar cache: `words` in device memory
// (the _dv calls), or null: the `single` words behind the arguments in the kernel-argument segment
constexpr int kRowioSingleMax = 320;    // descriptor words of a single-step call
struct StageRowsArgs {                  // word j: card | partial << 32
    const int64_t *words;
    const int32_t *ev;                  // int32[n_rows][n_ev], row-major
    int32_t *out;                       // int32[n_ev][R]
    int64_t *status;                    // int64[2]; word 0: the first invalid cell
    int64_t n_rows, row0, R, n_ev;
};
struct StageLikArgs {                   // word i: card | first column << 32
    const int64_t *words;
    const void *lik;                    // [n_rows][Ws], doubles or (lik_f32) floats
    void *out;                          // T[Ws][R], floats (out_f32) or doubles
    int64_t *e_row;                     // int64[R]
    int64_t *status;                    // int64[2]; word 1: the first invalid cell
    int64_t n_rows, row0, R, Ws, n_soft;
    int32_t lik_f32, out_f32;
    double *top;                        // the log form: double[n_soft][R], each block's largest entry
};
struct EmitScalarsArgs {
    const void *table;                  // T[R] (has_b) or T[1]; null: the constant 1
    const TableMeta *meta;              // the table's metadata (its exp2); null: 0
    const int64_t *e_row;               // int64[R] or null
    double *log10_z, *z;                // the caller's arrays (z may be null); entry row0 + b
    int64_t row0, rows_live;
    int32_t is_f32, has_b;
    const double *top;                  // the log form: double[n_soft][R] (n_soft 0: no shift), and its natural log
    double *ln_z;
    int64_t n_soft, R;
    const double *table_shift;          // the log form: one double added to every row's shift (log-form tables), or null
    int64_t *n_impossible;              // a counter the rows with p <= 0 are added to, or null
};
struct StageWeightsArgs {
    const double *weights;              // double[n_rows], or null: every row weighs 1
    double *out;                        // double[R]: the launch's weights, padding rows 0
    int64_t *status;                    // word 2: the first row whose weight is not finite or is negative
    int64_t n_rows, row0, R;
};
// device-resident model tables (tables.cuh).  words, per factor: its first entry in values, its size, its byte
// offset in out_buf; in device memory, or null: the `single` words behind the arguments
constexpr int kTablesSingleMax = 96;    // factors of a single-step call
struct StageTablesArgs {
    const int64_t *words;
    const void *values;                 // flat, doubles or (values_f32) floats
    void *out_buf;                      // the tables, floats (out_f32) or doubles
    TableMeta *out_meta;                // [n_factors]
    double *out_shift;                  // [1 + n_factors]: the shift, then every factor's top
    int64_t *status;                    // word 0: the first invalid entry (its flat index)
    int64_t n_factors;
    int32_t values_f32, out_f32;
};
struct StageTablesSingle {
    StageTablesArgs a;
    int64_t single[3 * kTablesSingleMax];
};
struct MstepArgs {
    const int64_t *words;               // per factor: first entry, k, first configuration; then the configurations in all
    const double *counts, *old_values;
    double *new_values;
    double prior;
    int64_t n_factors;
};
hipError_t launch_stage_tables(const StageTablesSingle &a, bool log_form, int max_grid, hipStream_t stream);
hipError_t launch_mstep(const MstepArgs &a, int64_t n_cfg, int max_grid, hipStream_t stream);
hipError_t launch_stage_weights(const StageWeightsArgs &a, int max_grid, hipStream_t stream);
struct EmitStatesArgs {                 // word v: (uint32) evidence column (-1: none) | partial << 32 | written << 33
    const int64_t *words;
    const uint8_t *x;                   // uint8[n_vars][K][R]
    const int32_t *ev;                  // the staged evidence table int32[n_ev][R] (null: no column)
    const void *table;                  // sampling: the result table, as EmitScalarsArgs (null: 1)
    const unsigned long long *deg;      // sampling: the draw step's counters, [R]
    void *out;                          // MPE: int32[n_rows][n_vars]; sampling: uint8[n_rows][K][n_vars]; may be null
    int64_t *n_degenerate;              // sampling: int64[n_rows], or null
    int64_t n_vars, K, R, row0, rows_live, n_drawn;
    int32_t sampling, is_f32, has_b, pad;
};
template <typename A>
struct RowioSingle {
    A a;
    int64_t single[kRowioSingleMax];
};
hipError_t launch_stage_rows(const RowioSingle<StageRowsArgs> &a, int max_grid, hipStream_t stream);
hipError_t launch_stage_lik(const RowioSingle<StageLikArgs> &a, int max_grid, hipStream_t stream);
hipError_t launch_stage_loglik(const RowioSingle<StageLikArgs> &a, int max_grid, hipStream_t stream);
hipError_t launch_emit_scalars(const EmitScalarsArgs &a, int max_grid, hipStream_t stream);
hipError_t launch_emit_logs(const EmitScalarsArgs &a, int max_grid, hipStream_t stream);
hipError_t launch_emit_states(const RowioSingle<EmitStatesArgs> &a, int max_grid, hipStream_t stream);
// the keys a family's dispatch switch holds (single-op or level launches),
// appended to `keys`: generated from the X-macro lists of the switches
// themselves (kernels.cuh, slab.cuh, chain.cuh, chainsplit.cuh), so the two
// cannot diverge; chain runs (kFamChain) exist as level launches only
void kernel_keys(int is_f32, int level, int family, std::vector<int> &keys);
// the reference's running sum of a single-op call (seqsum.hip): the terms
// prod_n in[n][pos_n(i, val)] (or in[0] / in[1]) for i over the output dims
// (reference scope order, last fastest) and val < k inner, added in order
constexpr int kSeqMaxDims = 32;
struct SeqSumArgs {
    const void *in[kMaxIn];                        // input tables, base offsets applied
    double *out;                                   // device
    int64_t n_terms;                               // output entries * k
    int64_t k;                                     // card of the summed variable (1: none)
    int n_in, n_dims, divide, pad;
    int64_t card[kSeqMaxDims];
    int64_t stride[kMaxIn][kSeqMaxDims + 1];       // per input: on each output dim, then on the summed variable
};
hipError_t launch_seq_sum(bool f32, const SeqSumArgs &a, hipStream_t stream);
// message exchange steps of sliced runs (xchg.hip; plan.hpp BucketSpec::xchg)
hipError_t launch_xchg_sync(bool f32, TableMeta *meta, int in_t, int x_t, int R, hipStream_t s);
hipError_t launch_xchg_pack(bool f32, TableMeta *meta, int in_t, int x_t, int out_t, int R, int mode, int64_t n,
                            hipStream_t s);
hipError_t launch_xchg_unpack(bool f32, TableMeta *meta, int in_t, int x_t, int out_t, int R, int64_t n,
                              hipStream_t s);
hipError_t launch_xchg_meta(TableMeta *meta, int in_t, int out_t, hipStream_t s);
// stream `s` waits `ns` nanoseconds on the device (one sleeping wave)
hipError_t launch_delay(double ns, hipStream_t s);
// the collective a sliced run's exchanges call (bnpp_collective_fn, include/bnpp.h)
struct XchgHooks {
    int (*fn)(void *user, int op, const void *send, void *recv, int64_t bytes, void *stream) = nullptr;
    void *user = nullptr;
};
// loopy BP, one workgroup (bp.hip)
hipError_t launch_sum_product(const BpArgs &a, hipStream_t stream);
// multi-workgroup flood (bp.hip): messages set to 1/|x|; one iteration (three
// launches); the marginals
hipError_t launch_bp_flood_init(const BpFlood &a, hipStream_t stream);
hipError_t launch_bp_flood_iteration(const BpFlood &a, int it, hipStream_t stream);
hipError_t launch_bp_flood_marginals(const BpFlood &a, hipStream_t stream);

enum DType { kF64 = 0, kF32 = 1 };

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    int max_grid = 2048;                // workgroups of a persistent launch (generic, stream, one-thread chain)
    int default_max_grid = 2048;        // ... as bnpp_ctx_create sized it
    int grid_cap = 0;                   // bnpp_ctx_set_max_grid (0: none): also caps the split chain launches
    std::string last_error;
    // arena kept between one-shot calls (partition / marginals): mapping and
    // unmapping a few hundred GB of HBM costs ~1 s each way, like a caching
    // allocator the context holds on to it until it is destroyed
    void *arena_cache = nullptr;
    int64_t arena_cache_pad = 0;        // bytes between the hipMalloc'd pointer and arena_cache (alignment)
    int64_t arena_cache_bytes = 0;
    // small device buffers (sources, descriptors, dims pool, metadata, results)
    // kept for reuse: a one-shot call otherwise pays ~10 hipMalloc / hipFree
    // pairs (hipFree synchronises), several ms of a small model's PR
    std::mutex buf_mu;
    std::vector<std::pair<void *, size_t>> buf_free;   // (buffer, capacity)
    size_t buf_free_bytes = 0;
    // the second lane of two-front schedules (Schedule::n_lanes), made on first use
    hipStream_t lane_stream = nullptr;
    // scratch of the single-op accumulate step (bnpp_bucket_counts), grown on demand
    void *counts_scratch = nullptr;
    size_t counts_scratch_cap = 0;
};

// a device buffer of at least `bytes` from the context's cache (or hipMalloc);
// `cap` receives its capacity, to hand back with put_buffer
hipError_t get_buffer(Context &ctx, size_t bytes, void **p, size_t *cap);
void put_buffer(Context &ctx, void *p, size_t cap);
void drop_buffer_cache(Context &ctx);

// Sources uploaded for one dtype: one device buffer, each factor pre-scaled by
// an exact power of two so its max lies in [0.5, 1).
struct DeviceSources {
    DType dtype = kF64;
    void *buf = nullptr;
    size_t buf_cap = 0;
    std::vector<TableMeta> meta;
    std::vector<int64_t> size;
};

// one result table copied out of the arena (launch_copies: one launch for all)
struct CopyItem {
    const void *src;
    void *dst;
    int64_t bytes;
};

// A schedule bound to device buffers, launchable many times.
struct Executable {
    DType dtype = kF64;
    bool own_arena = true;
    Schedule sched;
    void *arena = nullptr;
    TableMeta *d_meta = nullptr;        // live metadata
    TableMeta *d_meta0 = nullptr;       // pristine copy, restored before every launch
    BucketDesc *d_desc = nullptr;
    int64_t *d_pool = nullptr;
    std::vector<TableMeta> h_meta;
    CopyItem *d_copies = nullptr;       // result tables -> the program's results buffer
    int n_copies = 0;
    int64_t copy_max_bytes = 0;         // the largest of them
    // lanes: events a group records (-1: none) and the events it waits for
    // (producers of its inputs on the other lane); events[0] starts lane 1
    // after the metadata reset, events[1] joins it back before the results
    std::vector<hipEvent_t> events;
    std::vector<int> g_record;
    std::vector<std::vector<int>> g_wait;
    // lanes: the order the groups are enqueued in (empty: schedule order), the
    // lanes' windows alternating (lane_order.hpp)
    std::vector<int> g_order;
    size_t cap_meta = 0, cap_meta0 = 0, cap_desc = 0, cap_pool = 0, cap_copies = 0;   // buffer capacities
    // a sampling step (kSampleKey) draws with these at the next launch (bnpp_sample sets them per call)
    uint64_t sample_seed = 0;
    int64_t sample_first = 0;
    // ... and a batched draw step (kSampleBatchKey) with these too (run_sample_batch sets them per launch)
    int64_t sample_row_stride = 0, sample_row0 = 0, sample_n_valid = 0;
    // the accumulate steps (kCountsKey) add into counts_acc for the first counts_rows rows of the next launch
    double *counts_acc = nullptr;
    int64_t counts_rows = 0;
    // the emit step (kMargRowsKey) writes the first marg_rows_live rows of the next launch (run_marginals_batch sets it)
    int64_t marg_rows_live = 0;
    // their arguments: staged here per launch, copied to d_counts_args (one entry per accumulate step)
    std::vector<CountsArgs> h_counts_args;
    CountsArgs *d_counts_args = nullptr;
    size_t cap_counts_args = 0;
};

// Several schedules (target batches of one MAR job) run back to back in one
// shared arena; each batch's result tables are copied into a persistent
// results buffer before the next batch reuses the arena.
struct Program {
    DType dtype = kF64;
    std::vector<Executable> parts;
    void *arena = nullptr;
    int64_t arena_pad = 0;              // bytes between the hipMalloc'd pointer and arena (alignment)
    int64_t arena_bytes = 0;
    bool arena_cached = false;          // arena is the context's cache (not freed with the program)
    bool arena_reused = false;          // ... and was already allocated before this program
    double arena_alloc_ms = 0;          // hipMalloc of the arena (0 when reused), incl. the driver's HBM clearing wait
    void *results = nullptr;
    size_t results_cap = 0;
    int64_t results_bytes = 0;
    std::vector<std::vector<int64_t>> res_off;    // per part, per plan: byte offset (-1: constant 1)
    std::vector<std::vector<int64_t>> res_size;   // per part, per plan: entries
    XchgHooks hooks;                              // sliced runs: the ranks' collective
};

int upload_sources(Context &ctx, const std::vector<std::vector<double>> &values, DType dt, DeviceSources &out);
void free_sources(Context &ctx, DeviceSources &s);
int make_executable(Context &ctx, const DeviceSources &src, Schedule &&s, Executable &ex, void *shared_arena = nullptr);
int launch(Context &ctx, Executable &ex, hipStream_t stream, const XchgHooks *hooks = nullptr);
// waits for `stream`, downloads result tables: values as stored (double) and the exp2 scale
int fetch_results(Context &ctx, Executable &ex, hipStream_t stream, std::vector<std::vector<double>> &vals,
                  std::vector<int64_t> &exp2);
void free_executable(Context &ctx, Executable &ex);

int make_program(Context &ctx, const DeviceSources &src, std::vector<Schedule> &&batches, Program &pg,
                 bool use_cache = false);
// copy n result tables (device array of CopyItem) in one launch (launch.hip)
hipError_t launch_copies(const CopyItem *items, int n, int64_t max_bytes, hipStream_t stream);
// release the context's cached arena
void drop_arena_cache(Context &ctx);
int launch_program(Context &ctx, Program &pg, hipStream_t stream);
// result values (as stored, double) and exp2 of every plan, batches in order
int fetch_program(Context &ctx, Program &pg, hipStream_t stream, std::vector<std::vector<double>> &vals,
                  std::vector<int64_t> &exp2);
void free_program(Context &ctx, Program &pg);

}  // namespace bnpp
