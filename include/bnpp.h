/*
 * bnpp.h — C ABI of the MI355X-native bn-pp variable-elimination engine.
 *
 * The reference (GEO-IASS/bn-pp) has no FFI: its hot path sits behind the C++
 * class API of code/factor.hh and code/model.hh.  Every entry point below names
 * the reference interface it replaces (file:line into the reference's code/).
 * The C++ mirror of that class API (bn::Variable/Domain/Factor/BN/MN) lives in
 * include/bnpp/bn.hpp and is implemented on top of these calls.
 *
 * Conventions
 *   - Plain pointers and sizes; no C++ types; no exceptions cross the ABI.
 *   - Every call returns an int status (BNPP_OK == 0, negative on error);
 *     bnpp_strerror(status) names it, bnpp_last_error() gives the detail of the
 *     last failure on the calling thread.
 *   - Tables are row-major over their scope with the LAST variable fastest
 *     (domain.cpp:15-26).  Scopes are arrays of variable ids; `cards` is indexed
 *     by variable id and holds n_cards entries: an id outside [0, n_cards)
 *     anywhere in a call is BNPP_ERR_INVALID (the array is never read past).
 *   - Device tables passed to the single-op calls are caller-owned device
 *     buffers (bnpp_malloc, hipMalloc or a torch tensor's data_ptr); the engine
 *     never frees them.  `stream` is a hipStream_t (NULL: the context stream).
 *     Single-op calls only enqueue work.
 *   - No CPU fallback: without a usable MI355X every compute call fails with
 *     BNPP_ERR_NO_DEVICE.  Model loading, evidence loading, ordering and scope
 *     rules are host-only and work everywhere.
 *   - Thread safety: one context per device; calls on distinct contexts or
 *     distinct streams may run concurrently; model objects are read-only after
 *     creation.
 */
#ifndef BNPP_H
#define BNPP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BNPP_VERSION 205   /* 200: single ops take n_cards (the length of cards); 201: sliced bucket-tree marginals;
                              202: single ops return the reference's partition sum (out_sum);
                              203: planning introspection for tests (bnpp_plan_single, bnpp_kernel_keys);
                              204: chain-run introspection (bnpp_plan_groups, chain keys, bnpp_ctx_set_max_grid);
                              205: MPE (bnpp_mpe, bnpp_bucket_max, bnpp_plan_max_single, bnpp_plan_mpe_groups, job kind 4, kernel family 4);
                              still 205: posterior sampling (bnpp_sample, bnpp_bucket_sample, bnpp_plan_sample) only
                              adds symbols and shifts no argument of an existing one; likewise batched evidence
                              (bnpp_condition_batch, bnpp_partition_batch, bnpp_posterior_batch, bnpp_plan_batch,
                              bnpp_evidence_load_batch) and expected counts (bnpp_bucket_counts,
                              bnpp_expected_counts, bnpp_plan_counts) and batched marginals
                              (bnpp_bucket_marginal_rows, bnpp_marginals_batch, bnpp_plan_marginals_batch) */

enum bnpp_status {
    BNPP_OK = 0,
    BNPP_ERR_INVALID = -1,      /* bad shape / argument  (reference: throw const char*, assert) */
    BNPP_ERR_NO_DEVICE = -2,    /* no usable GPU */
    BNPP_ERR_OOM = -3,
    BNPP_ERR_HIP = -4,
    BNPP_ERR_IO = -5,           /* cannot open / parse a file (io.cpp:124, 150, 177: return -1/-2) */
    BNPP_ERR_UNSUPPORTED = -6
};

enum bnpp_dtype { BNPP_F64 = 0, BNPP_F32 = 1 };
/* OR-ed into the lik_dtype of a _dv call: the likelihood array holds natural logs (the log form, below) */
#define BNPP_LIK_LOG 2

/* elimination-order heuristics: bn flags -mf / -wmf / -md (bn.cpp:183-191) */
enum bnpp_heuristic { BNPP_ORDER_GIVEN = 0, BNPP_MIN_FILL = 1, BNPP_WEIGHTED_MIN_FILL = 2, BNPP_MIN_DEGREE = 3 };

const char *bnpp_strerror(int status);
const char *bnpp_last_error(void);
int bnpp_version(void);
/* 1 when the loaded library speaks the ABI this header declares.  Callers
 * check it once: a library of another version links (the symbol names are
 * unchanged) but would read shifted arguments. */
static inline int bnpp_abi_matches(void) { return bnpp_version() == BNPP_VERSION; }
/* Phase split (ms) of this thread's last bnpp_partition / bnpp_marginals /
 * bnpp_marginals_tree[_part] call -- the reference times these tasks as one
 * "uptime" (model.cpp:258/296, 309/343):
 *   out[0] ordering + planning + schedule (host)   out[1] source upload
 *   out[2] device program (arena, descriptors)     out[3] launch enqueue
 *   out[4] device run + result fetch                out[5] free
 *   out[6] total                                    out[7] 1 if the context's cached arena was reused
 *   out[8] of out[2]: the arena's hipMalloc (0 when reused) -- where a call
 *          waits for the driver to clear HBM that was freed shortly before
 *          (by any process: ~36 GB/s of backlog on MI355X)
 * Writes min(n, 9) values. */
int bnpp_last_timing(double *out, int n);

/* ------------------------------------------------------------- device */
typedef struct bnpp_ctx bnpp_ctx;

int bnpp_device_count(int *n);
int bnpp_ctx_create(int device, bnpp_ctx **out);
int bnpp_ctx_destroy(bnpp_ctx *ctx);
int bnpp_ctx_stream(bnpp_ctx *ctx, void **stream);
/* release the device memory the context keeps between calls (the cached arena
 * of the last partition / marginals call and the small-buffer cache) */
int bnpp_ctx_trim(bnpp_ctx *ctx);
/* Testing: every persistent launch of this context from now on uses at most n
 * workgroups (n = 0: the default grids again), so that the kernels' tile loops
 * iterate on small inputs: the generic, stream and chain launches.  The slab
 * launches have a flat grid (one workgroup per virtual block) and keep it.
 * Plans, cached jobs and results do not depend on it. */
int bnpp_ctx_set_max_grid(bnpp_ctx *ctx, int n);
int bnpp_malloc(bnpp_ctx *ctx, size_t bytes, void **dptr);
int bnpp_free(bnpp_ctx *ctx, void *dptr);
int bnpp_memcpy_h2d(bnpp_ctx *ctx, void *dst, const void *src, size_t bytes);
int bnpp_memcpy_d2h(bnpp_ctx *ctx, void *dst, const void *src, size_t bytes);
int bnpp_synchronize(bnpp_ctx *ctx, void *stream);

/* ------------------------------------------------- scope rules (host) */
/* Output scope of ((Factor(1.0) * in_0) * in_1) ... .sum_out(elim_var):
 * Domain(d1,d2) union order (domain.cpp:32-52) then Domain(d,v) removal
 * (domain.cpp:54-72).  elim_var < 0: pure product.  Writes *out_ndims ids. */
int bnpp_out_scope(int n_in, const int *in_ndims, const int *const *in_vars, int elim_var, int cap,
                   int *out_ndims, int *out_vars);

/* --------------------------------------------- single ops (device)
 * out_sum (every single op): NULL, or a DEVICE double that receives, when the
 * stream reaches it, the reference's running sum of the op (Factor::_partition,
 * factor.hh:26/47) with its bits: the op's terms added one at a time from 0.0
 * in fp64 in the reference's loop order -- product / divide / conditioning:
 * the output entries in linear order of the reference's output scope
 * (factor.cpp:129-139, 161-172, 226-236); sum_out and a fused bucket: the
 * INPUT (chain-product) entries in (output entry, summed value) order
 * (factor.cpp:196-208).  A sequential sum by definition (one wave, ~2e8
 * terms/s): ask for it only where the caller reads partition().  Single ops
 * compute the reference's unscaled values, so there is no log10 scale to
 * return (the VE entry points below carry theirs).  fp32 tables: the fp32
 * terms, widened, summed in fp64.  At most 32 output variables with out_sum
 * (BNPP_ERR_UNSUPPORTED otherwise, checked before the op is launched).  One
 * case the ABI cannot reproduce: Factor::sum_out of a variable NOT in the
 * scope returns a copy that keeps the input's STORED _partition
 * (factor.cpp:185-188), which may differ from the linear sum of its entries
 * (e.g. 1.0 after normalize); out_sum is always the linear sum -- a caller
 * that tracks _partition (the C++ mirror does) keeps its own value there. */
/* Fused bucket:  out = sum_{elim_var} prod_i in_i   — replaces the bucket body of
 * BN::variable_elimination (model.cpp:414-418):
 *     Factor prod(1.0); for (pf : bucket) prod *= *pf; prod.sum_out(var)
 * i.e. Factor::operator*= (factor.cpp:77-81) + Factor::product (factor.cpp:117-147)
 * + Factor::sum_out (factor.cpp:182-212) in one pass with no intermediate table.
 * fp64 results are bit-identical to that chain evaluated in input order.
 * out_vars must be the layout from bnpp_out_scope (or any permutation of it).
 * 1 <= n_in <= 8; elim_var < 0 means no summation; elim_var absent from every
 * input makes it a copy (factor.cpp:185-188). */
int bnpp_bucket_eliminate(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, int n_in,
                          const void *const *in_tables, const int *in_ndims, const int *const *in_vars,
                          int elim_var, void *out_table, int out_ndims, const int *out_vars, double *out_sum);

/* Max bucket (no reference counterpart: bn-pp has no MPE):
 *     out[e] = max_{elim_var} prod_i in_i,   out_arg[e] = the maximising value
 * the arithmetic of bnpp_bucket_eliminate with max in place of the sum: per
 * value v of elim_var the chain product ((1 * in_0) * in_1) ..., each product
 * rounded (no contraction); best starts as the product at v = 0 and a later v
 * replaces it only when its product is strictly greater, so ties keep the
 * LOWEST v (an all-zero row has arg 0).  out_arg: a DEVICE array of one uint8
 * per output entry, laid out as out_table, or NULL (values only).  elim_var is
 * required; absent from every input the call is a copy with arg 0.  A maximised
 * variable of more than 256 values: BNPP_ERR_UNSUPPORTED (checked on the host,
 * nothing is launched).  Unscaled, like every single op. */
int bnpp_bucket_max(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, int n_in,
                    const void *const *in_tables, const int *in_ndims, const int *const *in_vars, int elim_var,
                    void *out_table, int out_ndims, const int *out_vars, uint8_t *out_arg /* device, may be NULL */);

/* One posterior-sampling draw per sample (no reference counterpart: bn-pp
 * samples the prior only, from random_device).  State: x, a DEVICE array
 * uint8[n_cards][n_samples], variable-major: row v holds the value of variable
 * v in every sample.  For sample s and variable `var` of k = cards[var] values,
 * with the inputs in the given order, for v = 0 .. k-1:
 *     p_v = ((1 * in_0[..]) * in_1[..]) ...   dtype, each product rounded, no
 *                                             contraction; the other scope
 *                                             variables are read from x[.][s]
 *     c_v = c_{v-1} + (double)p_v             c_{-1} = 0.0, fp64, in order of v
 * t = u * c_{k-1} (one fp64 product); the drawn value is the LOWEST v with
 * c_v > t.  The comparison is strict, so a value with p_v == 0 is never drawn,
 * even for u == 0 (the reference's `prob <= p`, factor.cpp:279, would draw it).
 * If no v qualifies (c_{k-1} == 0, or NaN) the value is 0 and the draw is
 * counted in *n_degenerate (a DEVICE int64, may be NULL; the call clears it
 * first).  No inputs: p_v = 1, a uniform draw.  A common power-of-two scale of
 * the inputs changes no draw.
 * u: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments
 * 0x9E3779B9, 0xBB67AE85; round c' = (hi(M1 c2)^c1^k0, lo(M1 c2), hi(M0 c0)^c3^k1,
 * lo(M0 c0)), the key bumped after each of 10 rounds) with key (seed &
 * 0xffffffff, seed >> 32) and counter (g & 0xffffffff, g >> 32, var, 0), g =
 * first_sample + s; from the output words r0..r3, u = (((uint64)r0 << 32 | r1)
 * >> 11) * 2^-53, in [0, 1).  A draw depends on (seed, g, var) and the state
 * only: not on the grid, bnpp_ctx_set_max_grid, n_samples or how a range of g
 * is split over calls.
 * Tables are whole, in the given scope order; 0 to 8 inputs.  The call reads
 * the rows of the other scope variables and writes row `var`, nothing else.
 * Refused: ids outside [0, n_cards), n_samples < 1 (BNPP_ERR_INVALID); `var` or
 * a scope variable of more than 256 values (BNPP_ERR_UNSUPPORTED, before any
 * launch).  The state values in x are NOT checked, on the host or the device:
 * a value at or above its variable's card reads outside the tables. */
int bnpp_bucket_sample(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, int n_in,
                       const void *const *in_tables, const int *in_ndims, const int *const *in_vars, int var,
                       int64_t n_samples, int64_t first_sample, uint64_t seed,
                       uint8_t *x /* device [n_cards][n_samples] */, int64_t *n_degenerate /* device, may be NULL */);

/* Factor::product (factor.cpp:117-147; factor.hh:35) */
int bnpp_product(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *a, int a_ndims,
                 const int *a_vars, const void *b, int b_ndims, const int *b_vars, void *out, int out_ndims,
                 const int *out_vars, double *out_sum);

/* Factor::divide (factor.cpp:149-180; factor.hh:36): out = a / b over the
 * union scope (out_vars: any order of it).  The reference asserts on a zero
 * divisor (factor.cpp:165); here it yields inf / nan in that entry. */
int bnpp_divide(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *a, int a_ndims,
                const int *a_vars, const void *b, int b_ndims, const int *b_vars, void *out, int out_ndims,
                const int *out_vars, double *out_sum);

/* Factor::sum_out (factor.cpp:182-212; factor.hh:34) */
int bnpp_sum_out(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in, int ndims,
                 const int *vars, int var, void *out, int out_ndims, const int *out_vars, double *out_sum);

/* Factor::conditioning (factor.cpp:214-242; factor.hh:38): out scope = vars minus
 * evidence vars, order preserved (domain.cpp:74-90) */
int bnpp_condition(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in, int ndims,
                   const int *vars, int n_ev, const int *ev_vars, const int *ev_vals, void *out, double *out_sum);

/* Batched conditioning (no reference counterpart): the conditioning of `in` on
 * n_rows evidence assignments at once,
 *   out[rest][b] = in[ sum_j ev[j][b] * stride(ev_vars[j]) + offset(rest) ]
 * in: a table over vars in its natural layout; rest: its variables that are not
 * in ev_vars, order preserved, row-major; b, the evidence row, is the fastest
 * dimension of out (entries(rest) * n_rows elements).  ev: DEVICE
 * int32[n_ev][n_rows], variable-major.  Evidence variables outside the scope
 * are ignored, as in bnpp_condition.  The kernel moves values and does no
 * arithmetic on them.  A value outside its variable's range is clamped into
 * it (no read leaves `in`); the model-level calls below reject such rows on
 * the host.  At most 32 evidence variables may lie in the scope, and the
 * other variables may form at most 8 separate runs between them
 * (BNPP_ERR_UNSUPPORTED).  Only enqueues on `stream`. */
int bnpp_condition_batch(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in,
                         int ndims, const int *vars, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int32_t *ev /* device, [n_ev][n_rows] */, void *out);

/* ------------------------------------------------------ models (host) */
typedef struct bnpp_model bnpp_model;

/* read_uai_model (io.cpp:102-154) without the BAYES/MARKOV split: both kinds load */
int bnpp_model_load_uai(const char *path, bnpp_model **out);
/* the same data from arrays: scopes concatenated, values concatenated (row-major) */
int bnpp_model_from_arrays(int is_bayes, int n_vars, const int *cards, int n_factors, const int *widths,
                           const int *scopes, const double *values, bnpp_model **out);
/* Frees the model; every live context also drops what it caches for it (its
 * uploaded sources and a cached one-shot job planned for it -- a context in the
 * middle of a call keeps its job until its next one-shot call replaces it).
 * The contexts' cached arena is not the model's and stays: bnpp_ctx_trim. */
int bnpp_model_free(bnpp_model *m);
int bnpp_model_info(const bnpp_model *m, int *is_bayes, int *n_vars, int *n_factors);
int bnpp_model_cards(const bnpp_model *m, int *cards);
/* the model's values as one flat array in the layout of counts (bnpp_counts_size entries): what a
 * bnpp_tables of the model starts from */
int bnpp_model_values(const bnpp_model *m, double *values);
/* read_uai_evidence (io.cpp:157-180): *n pairs (0 unless the first integer is 1) */
int bnpp_evidence_load(const char *path, int cap, int *n, int *vars, int *vals);
/* An .evid file of any number of samples: the sample count, then per sample
 * `k v_1 x_1 ... v_k x_k`.  Every sample must observe the same variable set
 * (in any order); the variables are sorted per sample.  *n_ev variables into
 * ev_vars (ascending), *n_rows rows into ev_vals[row][*n_ev] (row-major).  A
 * sample observing another variable set than the first: BNPP_ERR_UNSUPPORTED
 * naming that sample.  More variables than cap_vars or samples than cap_rows:
 * BNPP_ERR_INVALID with *n_ev and *n_rows set (call again with room).
 * bnpp_evidence_load is unchanged: it reads such a file only when the count is 1. */
int bnpp_evidence_load_batch(const char *path, int cap_vars, int64_t cap_rows, int *n_ev, int *ev_vars,
                             int64_t *n_rows, int *ev_vals);

/* Graph::ordering (graph.cpp:41-101) over the graph of the evidence-conditioned
 * factors, as BN::variable_elimination builds it (model.cpp:360-369).
 * vars NULL: all non-evidence variables.  *width_out: induced width. */
int bnpp_ordering(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int n_vars,
                  const int *vars, int heuristic, int *order_out, int *width_out);

/* ------------------------------------------------ inference (device) */
/* BN::partition (model.cpp:250-301), VE branch: conditioning + VE.  Messages are
 * kept resident in HBM and rescaled by exact powers of two, so Z is returned as
 * log10 (always finite unless Z == 0) and as a double (may overflow to inf, as
 * the reference's would).  order: explicit order (heuristic BNPP_ORDER_GIVEN),
 * NULL otherwise.  uptime_ms covers ordering + planning + device run, like the
 * reference's steady_clock scope (model.cpp:258/296). */
int bnpp_partition(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                   int heuristic, const int *order, int n_order, int dtype, double *log10_z, double *z,
                   double *uptime_ms);

/* Most probable explanation (no reference counterpart: bn-pp has no MPE): the
 * joint assignment of all non-evidence variables with the largest unnormalised
 * probability given the evidence, by max-product bucket elimination over the
 * partition's elimination order and a traceback on the device.
 * Arithmetic: bnpp_partition's with max in place of + (same chain order, same
 * exact power-of-two rescaling, which max commutes with); every eliminating
 * bucket records its argmax (bnpp_bucket_max's tie rule: strict >, the lowest
 * value wins), and one workgroup then walks the elimination tree from the
 * roots, one tree depth per step.  *log10_value: log10 of the maximum (finite
 * unless it is 0).  assignment: n_vars values, evidence variables keep their
 * evidence value, a variable in no factor reads 0.  With ties, the assignment
 * is one maximiser (which one depends on the elimination order).
 * Limits: every maximised variable has at most 256 values
 * (BNPP_ERR_UNSUPPORTED otherwise, before anything is launched); all arg
 * tables (one byte per entry of every message) stay resident until the
 * traceback, beside the messages: BNPP_ERR_OOM, naming both sizes, when that
 * exceeds the memory budget (no checkpointing).  order: explicit order covering
 * every non-evidence variable (BNPP_ORDER_GIVEN), or NULL.  The planned job
 * stays with the context and an identical call relaunches it; the job kind is
 * part of the cache key, so it never shares a job with bnpp_partition. */
int bnpp_mpe(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
             const int *order, int n_order, int dtype, double *log10_value, int *assignment /* n_vars, evidence included */,
             double *uptime_ms);

/* Exact joint samples of P(x | evidence) (no reference counterpart: the
 * reference's logical sampling, likelihood weighting and Gibbs, model.cpp:541-720,
 * sample the prior and reject or weight, from random_device).
 * 1. Forward pass: bnpp_partition's elimination over the same order, with no
 *    fused chain runs (every eliminating bucket's inputs exist as tables); the
 *    sum kernels run unchanged.  *log10_z is the partition function's.
 * 2. One sampling step: one row per non-evidence variable, in REVERSE
 *    elimination order, each a bnpp_bucket_sample draw over the views of the
 *    variable's eliminating bucket as that bucket read them (after the forward
 *    pass they are P(x_i | separator) up to a constant).  Evidence variables
 *    keep their value; a variable in no remaining factor is drawn uniformly.
 * Samples are independent and exact: no burn-in, no rejection.  Sample s of the
 * call has the global index g = first_sample + s and depends on (seed, g) only,
 * so a range of g may be split over calls (or devices) in any way.
 * out: HOST array uint8[n_vars][n_samples], variable-major.  *n_degenerate:
 * draws whose weights summed to 0 or NaN (value 0 taken); 0 on a consistent
 * model with possible evidence.  Impossible evidence (Z = 0 or NaN, *log10_z =
 * -inf) has no posterior to draw from: every sampled value is 0 and every draw
 * counts as degenerate (n_samples x the non-evidence variables), also where the
 * zero reached Z without passing through the bucket of a draw.
 * Limits: every sampled variable has at most 256 values (BNPP_ERR_UNSUPPORTED
 * otherwise, before anything is launched); all messages stay resident until
 * the draws, beside n_vars * n_samples bytes of samples: BNPP_ERR_OOM, naming
 * both sizes, when that exceeds the memory budget (no checkpointing).
 * n_samples < 1: BNPP_ERR_INVALID.  The planned job stays with the context; the
 * cache key holds the job kind and n_samples but neither seed nor first_sample,
 * so a call with another seed relaunches the cached job. */
int bnpp_sample(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                const int *order, int n_order, int dtype, int64_t n_samples, int64_t first_sample, uint64_t seed,
                uint8_t *out /* host, [n_vars][n_samples] */, double *log10_z, int64_t *n_degenerate, double *uptime_ms);

/* Batched evidence (no reference counterpart): the partition function, or the
 * posterior of one target, for n_rows evidence assignments over ONE set of
 * evidence variables ev_vars[n_ev], values ev_vals[n_rows][n_ev] (row-major,
 * host), from one plan.
 * Plan: a virtual variable B ("which row", card = R rows per launch) is added.
 * Every factor that mentions an evidence variable is gathered once per launch
 * into a table over (its other variables, B) (bnpp_condition_batch's kernel);
 * that table takes exactly the place the conditioned view of the factor has in
 * the single call's plan.  The elimination then is the single call's: the
 * order depends on the evidence VARIABLES only (bnpp_partition's order over the
 * non-evidence variables; bnpp_marginals' over those but the target), bucket
 * assignment and chain order are the single call's, the sum kernels run
 * unchanged with B as the fastest dimension of every message evidence reaches;
 * a message no evidence reaches carries no B and is computed once per launch.
 * No fused chain runs (the unfused buckets do the same arithmetic).
 * Arithmetic: messages are rescaled by exact powers of two per table, so the
 * scale is shared by the rows of a launch and differs from the single call's;
 * mantissas do not, as long as nothing goes subnormal.  In fp64 z[b] is
 * bit-identical to bnpp_partition's z for row b; log10_z[b] = log10(p) + exp2 *
 * log10(2) may differ from the single call's by the rounding of those three
 * operations (it is taken of the split of Z that frexp gives, so it depends on
 * rows_per_launch no more than z does).  Posteriors are normalised per row on the host as bnpp_marginals
 * does (sequential sum, one division; the scale cancels exactly): fp64
 * posteriors are bit-identical to bnpp_marginals with targets = {target}.
 * Z_b == 0: log10_z = -inf, z = 0; the posterior row is what bnpp_marginals
 * returns for that evidence (0 / 0: NaN in every entry).
 * Shared scale (a limit): a row whose messages lie more than the dtype's
 * exponent range below the largest row of the same launch loses bits or
 * flushes to zero -- 2^-1022 in fp64, out of reach of real models; 2^-126 in
 * fp32, reachable when a launch mixes a near-certain row with a very unlikely
 * one (use fp64, or group such rows into calls of their own).
 * rows_per_launch: 0 = the largest power of two, at most 2^16, whose arena fits
 * the memory budget (BNPP_MEM_BUDGET_GB, else the device's free memory) -- and
 * no larger than the smallest power of two that holds n_rows, so that no
 * launch works mostly on padding; R >= 1 is used as given.  One plan of card(B) = R is launched
 * ceil(n_rows / R) times, each launch on the next R rows; the last launch is
 * padded by repeating its last row.  Results do not depend on R (fp64: bit for
 * bit).  Even R = 1 over the budget: BNPP_ERR_OOM naming both sizes.
 * BNPP_ERR_INVALID: n_rows < 1; a duplicate or out-of-range evidence variable;
 * an evidence value outside its variable's range in any row (the message names
 * the row and the variable; nothing is launched); target out of range or an
 * evidence variable.  Values are int: no limit on cardinalities.
 * The planned job stays with the context; the cache key holds the job kind, the
 * evidence variable set, R and the target but not the values, which are launch
 * data: a call with other values relaunches the cached job (plan time 0).
 * order (partition only): explicit order (BNPP_ORDER_GIVEN) or NULL.
 * bnpp_last_timing covers the whole call (every launch). */
int bnpp_partition_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals /* [n_rows][n_ev] */, int heuristic, const int *order, int n_order,
                         int dtype, int64_t rows_per_launch, double *log10_z /* [n_rows] */,
                         double *z /* [n_rows], may be NULL */, double *uptime_ms);
int bnpp_posterior_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals /* [n_rows][n_ev] */, int heuristic, int target, int dtype,
                         int64_t rows_per_launch, double *out /* [n_rows][card(target)] */, double *uptime_ms);

/* Batched MPE (no reference counterpart): the most probable joint completion
 * of n_rows evidence assignments over ONE evidence variable set, from one plan.
 * Row b: log10_value[b] and assignment[b * n_vars ..] are what bnpp_mpe returns
 * for evidence row b under the same elimination order, which depends on the
 * evidence VARIABLES only (as in bnpp_partition_batch).  Evidence variables keep
 * their value in the assignment; a variable in no factor reads 0.
 * Plan: bnpp_partition_batch's gather steps, evidence table and row variable B
 * (card = R rows per launch), then bnpp_mpe's elimination over them: every
 * eliminating bucket maximises and records its argmax (one byte per entry) in a
 * table over its output scope -- B the fastest dimension exactly where the
 * message has it; a bucket no evidence reaches has neither and runs once per
 * launch.  No fused chain runs; pure-product prefixes stay products.  One
 * traceback step then decodes R assignments at once, a lane per row.
 * Same assignment, entry for entry: bucket assignment, chain order and the
 * strict-> tie rule (a tie keeps the lowest value) are the single call's; the
 * rows of a launch share each message's power-of-two scale, and multiplying
 * both sides of p > best by the same exact power of two changes no comparison.
 * So every arg byte, hence assignment[b], equals bnpp_mpe's in every entry, ties
 * included, in fp64 and in fp32, as long as nothing goes subnormal.
 * log10_value[b] is taken of the split of the maximum that frexp gives (as
 * log10_z in bnpp_partition_batch), so it depends on rows_per_launch no more
 * than the maximum does; it lies within 4 ulp of max(1, |log10_value|) of
 * bnpp_mpe's.  A row whose maximum is 0: log10_value = -inf and the assignment
 * bnpp_mpe returns for it (all-zero entries take arg 0); its neighbours are
 * not affected.  The shared-scale limit of bnpp_partition_batch applies.
 * rows_per_launch: chosen exactly as in bnpp_partition_batch; the arena now
 * also holds every arg table, resident up to the traceback, and the assignment
 * state (n_vars bytes per row).  No checkpointing: BNPP_ERR_OOM names the
 * message bytes and the arg bytes.  Results do not depend on R (assignments
 * equal, log10_value bit for bit in fp64).  The last launch is padded by
 * repeating its last row.
 * Limits and errors: bnpp_mpe's plus bnpp_partition_batch's.  A maximised
 * variable has at most 256 values (BNPP_ERR_UNSUPPORTED before any launch); an
 * explicit order covers every non-evidence variable; the BNPP_ERR_INVALID cases
 * and messages (naming row and variable) are bnpp_partition_batch's.  The
 * arguments are checked before the context is looked at; a NULL context then
 * gives BNPP_ERR_NO_DEVICE where no device is visible, else BNPP_ERR_INVALID.
 * Evidence values are int, so assignment is int.  Either output may be NULL.
 * The planned job stays with the context under a job kind of its own; the
 * cache key holds the kind, the evidence variable set and R, never the values. */
int bnpp_mpe_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                   const int *ev_vals /* [n_rows][n_ev] */, int heuristic, const int *order, int n_order, int dtype,
                   int64_t rows_per_launch, double *log10_value /* [n_rows] */,
                   int *assignment /* [n_rows][n_vars], row-major */, double *uptime_ms);

/* Batched posterior sampling (no reference counterpart): K = n_per_row exact
 * joint samples of P(x | evidence row b) for each of n_rows evidence
 * assignments over ONE evidence variable set, from one plan.
 * Same bytes as the single call: sample (b, s) is the sample bnpp_sample draws
 * for evidence row b with the same seed at the global index
 *   g = first_sample + b * row_stride + s        (b: the row's index in the call)
 * in every byte, in fp64 and in fp32, as long as nothing goes subnormal.  The
 * elimination order depends on the evidence VARIABLES only, bucket assignment
 * and chain order are the single call's, and the draw c_v > u * c_{k-1} does
 * not see the power-of-two scale the rows of a launch share (exp2 is never
 * read).  The Philox counter stays (g lo, g hi, variable, 0).
 * row_stride = 0 gives every row the same random numbers (common random
 * numbers: equal rows give equal samples); row_stride >= K gives the rows
 * disjoint streams, hence independent draws.  A range of rows may be split over
 * calls: the call that starts at row b0 passes first_sample + b0 * row_stride.
 * Plan: bnpp_partition_batch's gather steps, evidence table and row variable B
 * (card = R rows per launch), then bnpp_sample's unfused forward pass over
 * them; a view carries B exactly where evidence reaches it, a bucket that no
 * evidence reaches runs once per launch.  One draw step ends the plan: lane t
 * of R * K owns (b, s) = (t % R, t / R), state uint8[n_vars][K][R].
 * out: HOST array uint8[n_rows][K][n_vars], row-major; evidence variables hold
 * their row's value.  log10_z[b] has bnpp_partition_batch's bits.
 * n_degenerate[b] is the single call's count for row b: an impossible row has
 * log10_z = -inf, every draw degenerate and every sampled value 0, as the
 * single call gives, and leaves its neighbours alone.  Results do not depend on rows_per_launch,
 * the grid cap or how rows are split over calls, byte for byte; the padding
 * rows of the last launch are neither written out nor counted.
 * Limits: bnpp_sample's plus bnpp_partition_batch's.  A sampled variable, or
 * an evidence variable (out holds bytes), of more than 256 values is
 * BNPP_ERR_UNSUPPORTED before any launch; an explicit order covers every
 * non-evidence variable; the shared-scale limit of bnpp_partition_batch
 * applies.  All forward messages (times R where they carry B) and the n_vars
 * * R * K state bytes stay resident until the draws (no checkpointing):
 * BNPP_ERR_OOM names both sizes.  rows_per_launch 0: chosen as in
 * bnpp_partition_batch, the state counted in the arena.
 * Errors: the BNPP_ERR_INVALID cases and messages (naming row and variable)
 * are bnpp_partition_batch's; also n_per_row < 1, row_stride < 0,
 * first_sample < 0, or first_sample + (n_rows - 1) * row_stride + n_per_row
 * overflowing int64.  The arguments are checked before the context is looked
 * at; a NULL context then gives BNPP_ERR_NO_DEVICE where no device is visible,
 * else BNPP_ERR_INVALID.  Any output may be NULL.
 * The planned job stays with the context under a job kind of its own; the
 * cache key holds the kind, the evidence variable set, R and K, never the
 * values, seed, first_sample or row_stride. */
int bnpp_sample_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                      const int *ev_vals /* [n_rows][n_ev] */, int heuristic, const int *order, int n_order, int dtype,
                      int64_t rows_per_launch, int64_t n_per_row /* K >= 1 */, int64_t first_sample,
                      int64_t row_stride /* >= 0 */, uint64_t seed,
                      uint8_t *out /* host [n_rows][K][n_vars], row-major */, double *log10_z /* [n_rows], may be NULL */,
                      int64_t *n_degenerate /* [n_rows], may be NULL */, double *uptime_ms);

/* Expected sufficient statistics (no reference counterpart): for every factor f
 * with scope S_f, N_f(x_S) = sum_b w_b P(x_S | evidence row b) -- what EM's E
 * step and the gradient of sum_b w_b log Z_b need (N_f = theta_f * d/d theta_f).
 * Plan: bnpp_partition_batch's plan (gather steps, the same forward buckets in
 * the same order, the same result table over (B)) continued by the backward
 * pass of the bucket tree with B kept in every message evidence reaches; for
 * every factor the belief of its bucket, summed down to (S_f minus evidence, B),
 * is folded into a persistent fp64 accumulator by the accumulate step below
 * (all factors' steps in one launch of each of its two passes).
 * counts: host, sum over factors of the table sizes, factors in model order,
 * each in its natural layout over its full scope (evidence variables included).
 * weights: n_rows doubles, NULL = all 1; a negative or non-finite weight is
 * BNPP_ERR_INVALID naming the row.  log10_z[b] (may be NULL) is computed
 * exactly as bnpp_partition_batch's; *n_impossible (may be NULL) counts the rows
 * with Z_b == 0, which contribute to no factor.  Arguments are checked before
 * the context is looked at.  rows_per_launch and BNPP_ERR_OOM as
 * bnpp_partition_batch, but every forward message stays resident through the
 * backward pass (no checkpointing).  The fp64 counts do not depend on
 * rows_per_launch, bit for bit (the accumulate step's order of additions, below;
 * the shared-scale limit of bnpp_partition_batch applies: a row whose belief
 * underflows to zeros beside a much likelier row of its launch is skipped).
 * Rows with different missing patterns are the caller's to group by pattern:
 * counts add, so call once per pattern and sum.
 * The planned job stays with the context, keyed like a batch job (the evidence
 * variable set, never the values or the weights). */
int bnpp_counts_size(const bnpp_model *m, int64_t *n /* the doubles bnpp_expected_counts writes */);
int bnpp_expected_counts(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals /* [n_rows][n_ev] */, const double *weights /* [n_rows] or NULL */,
                         int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                         double *counts, double *log10_z /* [n_rows] or NULL */, int64_t *n_impossible,
                         double *uptime_ms);

/* The accumulate step on caller-owned device buffers (what bnpp_condition_batch
 * is to the gather kernel): only enqueues on `stream`, adds into acc (the
 * caller zeroes it).  table: the belief T over (scope minus the evidence
 * variables, in scope order, then b), b fastest, n_rows = R rows; has_b = 0: T
 * has no b dimension and is read with row stride 0.  ev: device
 * int32[n_ev][R], variable-major; weights: device double[R] or NULL (all 1);
 * valid: device table of the dtype, R entries, or NULL; acc: device double[],
 * the factor's natural layout over scope[n_scope].
 * Contract -- all arithmetic in fp64 on values converted from T, every
 * operation rounded once, no contraction, in this order:
 *   c[b] = sum over rest, ascending linear rest index, sequentially from 0.0,
 *          of (double)T[rest][b];
 *   row b is skipped when b >= rows_live, w[b] == 0, c[b] == 0 or NaN, or
 *          valid[b] == 0;
 *   else   acc[offset(rest, evidence values of row b)] += w[b] * ((double)T[rest][b] / c[b]);
 *   the contributions to one entry are added in ascending row order, one at a
 *   time, continuing from the entry's value in acc.
 * Hence the result depends on neither the grid (bnpp_ctx_set_max_grid) nor R
 * nor how rows split over calls; a belief's scale cancels in t / c.  An
 * evidence value is clamped into its variable's range.  At most 32 evidence
 * variables and 32 others in the scope.  The step keeps 24 bytes per row of
 * scratch with the context: calls that share a context must be ordered on one
 * stream. */
int bnpp_bucket_counts(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *table,
                       int n_scope, const int *scope, int n_ev, const int *ev_vars, int64_t n_rows, int64_t rows_live,
                       const int32_t *ev, const double *weights, const void *valid, int has_b, double *acc);

/* Batched marginals (no reference counterpart): every single-variable posterior
 * P(X_t | evidence row b) of every row from ONE plan -- what a loop of
 * bnpp_posterior_batch over the targets computes with one plan and one forward
 * elimination per target.  Plan: bnpp_expected_counts's batched bucket tree (the
 * gather steps, bnpp_partition_batch's forward buckets and result table over
 * (B), the backward pass with B kept in every message evidence reaches); for
 * every target the smallest belief that contains it is summed down to
 * (target, B), and one emit step (below) normalises the tables row by row into
 * a row-major device array that one copy per launch moves into `out`.
 * targets NULL: all variables (n_targets is ignored); else n_targets >= 1 ids
 * in range, none twice.  out: host [n_rows][W], row-major, W = sum of the
 * targets' cards, the targets in the given order.  A target that is an evidence
 * variable gets the one-hot of the row's value; a variable in no remaining
 * factor 1 / card.  Arguments are checked before the context is looked at: the
 * rows as bnpp_partition_batch (messages naming row and variable), a target
 * out of range or listed twice, an explicit order that leaves out a
 * non-evidence variable.
 * Guarantees: log10_z[b] (may be NULL) has bnpp_partition_batch's bits.  The
 * fp64 out does not depend on rows_per_launch, the grid cap
 * (bnpp_ctx_set_max_grid) or how rows split over calls, bit for bit.  Row b is
 * within 1e-12 (fp64) / 1e-5 (fp32) absolute of bnpp_marginals for that row's
 * evidence -- not bit-identical to bnpp_posterior_batch: the sums associate
 * differently.  A row with Z_b == 0 gets log10_z = -inf, NaN in its belief
 * columns and keeps its one-hot evidence columns; its neighbours are not
 * touched.  The shared-scale limit of bnpp_partition_batch applies: a row that
 * flushes to zero beside a much likelier row of its launch reads NaN.  One
 * evidence variable set per call (group rows by missing pattern); cardinalities
 * have no limit.  rows_per_launch and BNPP_ERR_OOM as bnpp_expected_counts (every
 * forward message resident, no checkpointing); the arena also holds the
 * rows_per_launch * W * 8 bytes of the output table, and the message names the
 * message bytes and the output bytes.  The planned job stays with the context,
 * keyed by its kind, the evidence variable set, R and the target list (never
 * the values). */
int bnpp_marginals_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals /* [n_rows][n_ev] */, int heuristic, const int *order, int n_order,
                         int n_targets, const int *targets /* NULL: all variables */, int dtype, int64_t rows_per_launch,
                         double *out /* host [n_rows][W] */, double *log10_z /* [n_rows] or NULL */, double *uptime_ms);

/* The emit step on caller-owned device buffers (what bnpp_bucket_counts is to
 * the accumulate step): only enqueues on `stream`.  Target j has cards[j]
 * values and the table tables[j] of the dtype over (x, b), b fastest, n_rows =
 * R rows; has_b[j] = 0: no b dimension, read with row stride 0.  tables[j]
 * NULL: an evidence block when ev_row[j] >= 0 (the row of ev = device
 * int32[n_ev][R], variable-major, that holds the target's values), else a free
 * block.  out: device double[R][W], row-major, W = sum of cards, target j's
 * block at column off_j = cards[0] + .. + cards[j - 1].
 * Contract -- all arithmetic in fp64 on values converted from the table, every
 * operation rounded once, no contraction:
 *   c = sum over x, ascending, sequentially from 0.0, of (double)T_j[x][b];
 *   out[b][off_j + x] = (double)T_j[x][b] / c      (c == 0: 0/0 = NaN, nothing special-cased);
 *   evidence block: 1.0 at the row's value (clamped into range), 0.0 elsewhere;
 *   free block: 1.0 / card;
 *   rows b >= rows_live are not written.
 * The result depends on neither the grid (bnpp_ctx_set_max_grid) nor how rows
 * split over calls; a table's scale cancels in t / c.  BNPP_ERR_INVALID:
 * n_targets < 1 or a card < 1; rows_live outside [0, R]; a target with no
 * table, ev_row[j] < 0 and has_b[j] set; ev_row[j] >= 0 with ev == NULL.  At most
 * 64 targets per call (the descriptors travel in the kernel-argument segment;
 * BNPP_ERR_UNSUPPORTED beyond): split a longer list by columns. */
int bnpp_bucket_marginal_rows(bnpp_ctx *ctx, void *stream, int dtype, int n_targets, const int *cards /* per target */,
                              const void *const *tables /* NULL: evidence or free */, const int *has_b,
                              const int *ev_row /* -1: none */, int64_t n_rows /* R */, int64_t rows_live,
                              const int32_t *ev /* device int32[n_ev][R], may be NULL */, double *out /* device double[R][W] */);

/* BN::marginals (model.cpp:303-346), VE branch: one VE per target with every
 * other variable eliminated, then Factor::normalize (factor.cpp:244-255).  All
 * targets run as one batched device schedule.  targets NULL: all variables.
 * out receives sum(card[t]) values target-major; an evidence variable's marginal
 * is written one-hot (the UAI MAR format; the reference prints a width-0 factor). */
int bnpp_marginals(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                   int heuristic, int n_targets, const int *targets, int dtype, double *out, double *uptime_ms);

/* All marginals from ONE two-pass bucket tree (Shafer-Shenoy message passing
 * on the VE bucket tree of the partition's elimination order) instead of one VE
 * per target (model.cpp:326-334): about three VE passes of device work and one
 * host ordering, whatever the number of targets.  Same output as
 * bnpp_marginals (normalised, evidence one-hot); values agree with the
 * reference to rounding (not bit-exact: the sums are associated differently).
 * order: explicit elimination order covering every non-evidence variable
 * (heuristic BNPP_ORDER_GIVEN), or NULL.  BNPP_ERR_OOM when every forward
 * message cannot stay resident within the memory budget. */
int bnpp_marginals_tree(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                        int heuristic, const int *order, int n_order, int n_targets, const int *targets, int dtype,
                        double *out, double *uptime_ms);

/* One part of bnpp_marginals_tree for multi-GPU runs (one process per GPU,
 * part = rank, n_parts = world size): this part computes only the marginals it
 * owns (a contiguous segment of a chain-shaped bucket tree, else every
 * n_parts-th target) and writes zeros for the others; owned[i] (optional)
 * flags targets[i].  Summing `out` over the parts gives bnpp_marginals_tree's
 * output (one all-reduce, no other exchange). */
int bnpp_marginals_tree_part(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                             int heuristic, const int *order, int n_order, int n_targets, const int *targets,
                             int part, int n_parts, int dtype, double *out, int *owned, double *uptime_ms);

/* Message-sliced bucket-tree marginals for multi-GPU runs (no reference
 * counterpart: the reference is single-process; this replaces the N
 * independent VEs of BN::marginals, model.cpp:303-346, across N ranks).  Every
 * message of the chain-shaped bucket tree is split into n_ranks blocks by
 * log2(n_ranks) binary variables that stay in the separators for a window of
 * the chain; rank r holds and computes the block whose slice variables read r
 * (slowest first), and between windows a message is re-sliced by one
 * all-to-all through `coll` (at the chain's ends an all-gather).  n_ranks: a
 * power of two >= 2; every rank calls this with the same model, evidence,
 * order, targets and budget_gb (> 0: the device memory in GB the plan must
 * fit, which sets its checkpoint count -- it must agree across ranks, e.g. the
 * smallest free memory; <= 0: this device's).  The collective is called synchronously from this
 * thread, in the same sequence on every rank (two-lane schedules: the lanes'
 * windows alternately, each lane on its own stream), and must be complete (or
 * enqueued on `stream`) when it returns:
 *   op BNPP_COLL_ALLGATHER: each rank contributes `bytes` at send; recv gets
 *                           rank r's at recv + r * bytes
 *   op BNPP_COLL_ALLTOALL:  send holds n_ranks blocks of `bytes`, block d for
 *                           rank d; recv gets rank s's block at recv + s * bytes
 * Output: this rank's share of each target's unnormalised marginal, as
 * mantissas (out, sum(card) doubles) times 2^out_exp2[i] per target
 * (out_exp2 = -2^40 for an all-zero share); the marginal is the normalised sum
 * of the shares over the ranks (bnpp.dist.sliced_tree_marginals).  Trees that
 * are not chains, or chains without such windows: BNPP_ERR_UNSUPPORTED.  As
 * bnpp_marginals_tree, the planned job stays with the context, and an
 * identical call (same model, evidence, order, targets, dtype, rank, n_ranks
 * and budget) relaunches it; coll / user are bound per call. */
#define BNPP_COLL_ALLGATHER 0
#define BNPP_COLL_ALLTOALL 1
typedef int (*bnpp_collective_fn)(void *user, int op, const void *send, void *recv, int64_t bytes, void *stream);
int bnpp_marginals_tree_sliced(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                               int heuristic, const int *order, int n_order, int n_targets, const int *targets,
                               int rank, int n_ranks, bnpp_collective_fn coll, void *user, double budget_gb,
                               int dtype, double *out, int64_t *out_exp2, double *uptime_ms);
/* A collective for one GPU (user: const int[4] = {n_ranks, flags, link MB/s,
 * latency us}): every received block is a copy of the sent one -- a world of
 * identical ranks, for timing one rank's share of a sliced run (the data it
 * computes is not a real world's); flags & 1: nothing is copied (the compute
 * alone); flags & 2: the calling stream waits the transfer's modelled time,
 * latency + bytes sent / (min(n_ranks - 1, 7) links x MB/s). */
int bnpp_collective_loopback(void *user, int op, const void *send, void *recv, int64_t bytes, void *stream);

/* BN::marginals with options["sum-product"] (model.cpp:313-317; the `bn -sp`
 * flag): loopy BP on the factor graph of the model's factors,
 * FactorGraph::update(max_iter, eps) (graph.cpp:298-332; the reference uses
 * 10000, 0.001, model.cpp:749) then FactorGraph::marginal per variable
 * (graph.cpp:393-403).  Evidence is not used, as in the reference.  fp64.
 * out: sum(card) values, var-major; *iterations = update's return value
 * (max_iter when it did not converge).  Small models run in one workgroup,
 * larger ones (or any factor table of 2^31+ entries, indexed in 64 bits) as a
 * multi-workgroup flood (BNPP_BP_MODE=single|multi forces either). */
int bnpp_sum_product(bnpp_ctx *ctx, const bnpp_model *m, int max_iter, double eps, double *out, int *iterations,
                     double *uptime_ms);

/* BN::variable_elimination (model.cpp:348-446) over the factors of `m` taken
 * as given (already conditioned by the caller): eliminates `vars` (heuristic
 * order, or exactly this order with BNPP_ORDER_GIVEN) and returns the result
 * factor: *out_ndims scope ids in out_vars (reference chain order), *out_size
 * values in out_values, scaled: true value = out_values[i] * 2^(*exp2). */
int bnpp_variable_elimination(bnpp_ctx *ctx, const bnpp_model *m, int n_vars, const int *vars, int heuristic,
                              int dtype, int cap_vars, int *out_ndims, int *out_vars, int64_t cap_values,
                              int64_t *out_size, double *out_values, int64_t *exp2);

/* Host-only planning statistics (no device needed): kind 0 partition (explicit
 * order if `order` is non-NULL), 1 marginals of all variables (one VE each),
 * 2 bnpp_variable_elimination of the variables in `order`, 3 bucket-tree
 * marginals of all variables, 4 MPE (the arena bytes then hold the messages
 * and every arg table).  stats as bnpp_job_stats. */
int bnpp_plan_stats(const bnpp_model *m, int kind, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                    const int *order, int n_order, int dtype, double *stats, int n_stats);

/* Planning introspection for tests (host only, no device): which kernel a
 * single-op call launches.  The arguments of bnpp_bucket_eliminate without
 * tables or stream; divide != 0 plans bnpp_divide (two inputs, elim_var -1);
 * n_ev > 0 plans the inputs as bnpp_condition's views of that evidence
 * (out_vars then holds the variables left).  It fails exactly where the call
 * would.  info[0 .. n_info), n_info <= 12:
 * [0] family (0 generic, 1 stream, 2 slab)  [1] dispatch key  [2] n_in
 * [3] k (card of the summed variable, 1: none)  [4] v1  [5] v2 (register tile)
 * [6] big class (0: generic)  [7] 32-bit offsets  [8] n_tiles  [9] lanes
 * [10] slab_y2  [11] 1 when the key is instantiated for the dtype */
int bnpp_plan_single(int dtype, int n_cards, const int *cards, int n_in, const int *in_ndims, const int *const *in_vars,
                     int elim_var, int out_ndims, const int *out_vars, int divide, int n_ev, const int *ev_vars,
                     const int *ev_vals, int64_t *info, int n_info);

/* The same for bnpp_bucket_max (its arguments without tables or stream): the
 * max-family kernel the call launches, info laid out as bnpp_plan_single's
 * ([0] family = 4, [6] = 0).  It fails exactly where the call would. */
int bnpp_plan_max_single(int dtype, int n_cards, const int *cards, int n_in, const int *in_ndims,
                         const int *const *in_vars, int elim_var, int out_ndims, const int *out_vars, int64_t *info,
                         int n_info);

/* Planning introspection for tests: the dispatch keys instantiated for a dtype
 * in the generic (0), stream (1), slab (2), chain (3) or max (4) family, for single-op
 * (launch 0) or level (launch 1) launches: *n keys, the first min(*n, cap) in
 * keys.  Chain runs are level launches only (launch 0 lists none); their
 * fused-belief kernels are listed under their own keys. */
int bnpp_kernel_keys(int dtype, int launch, int family, int *keys, int cap, int *n);

/* Planning introspection for tests: *supported = 1 when the planner's own
 * predicate (chain_supported: what build_desc asks before it picks a chain
 * form) accepts `key` for the dtype.  bnpp_kernel_keys family 3 lists exactly
 * the keys it accepts. */
int bnpp_chain_key_supported(int dtype, int key, int *supported);

/* Planning introspection for tests (host only, no device): the launch groups
 * of the plan bnpp_plan_stats reports on (same kind, evidence, order, dtype
 * and planning switches; kind 3 also by part of n_parts as
 * bnpp_plan_tree_part, else part 0 of 1).  One row of BNPP_PLAN_GROUP_FIELDS
 * values per group, batches in order: [0] batch  [1] level  [2] dispatch key
 * [3] descriptors in the launch (a split chain key runs its one-run kernel
 * with 1, its multi-run kernel with more)  [4] virtual blocks  [5] lane.
 * *n_rows groups, the first min(*n_rows, cap_rows) in rows. */
#define BNPP_PLAN_GROUP_FIELDS 6
int bnpp_plan_groups(const bnpp_model *m, int kind, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                     const int *order, int n_order, int dtype, int part, int n_parts, int64_t *rows, int cap_rows,
                     int *n_rows);

/* The same for the plan of bnpp_mpe (bnpp_plan_stats kind 4; bnpp_plan_groups
 * itself takes the sum plans, kinds 0-3, only): rows as bnpp_plan_groups's,
 * one batch, lane 0.  Keys: max buckets 65536 + the generic key of their
 * shape (bnpp_kernel_keys family 4), the traceback 2^24 + 4096 (one group, the
 * last), pure-product prefixes and the final product ordinary generic keys. */
int bnpp_plan_mpe_groups(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                         const int *order, int n_order, int dtype, int64_t *rows, int cap_rows, int *n_rows);

/* Host-only planning of bnpp_sample (its plan has no kind in bnpp_plan_stats,
 * bnpp_plan_groups or bnpp_job_create): stats[0..8) as bnpp_job_stats (the
 * arena bytes hold the messages and the n_vars * n_samples sample bytes), then
 * [8] rows of the sampling step, [9] bytes of the samples; rows as
 * bnpp_plan_groups's.  Every key but the last is an ordinary sum-plan key (no
 * chain key); the sampling step is the last group, key 2^24 + 8192. */
int bnpp_plan_sample(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                     const int *order, int n_order, int dtype, int64_t n_samples, double *stats, int n_stats,
                     int64_t *rows, int cap_rows, int *n_rows);

/* Host-only planning of bnpp_partition_batch (target < 0) or
 * bnpp_posterior_batch (target >= 0; order is then ignored): stats[0..8) as
 * bnpp_job_stats for the plan of one launch, then [8] the rows per launch R
 * (rows_per_launch, or the automatic choice for 0 under BNPP_MEM_BUDGET_GB or
 * 64 GB: no device is consulted), [9] the gather steps; rows as
 * bnpp_plan_groups's.  The gather steps are the groups of level 0, one each,
 * key 2^24 + 12288; every other key is an ordinary sum-plan key (no chain key).
 * result_scope (room for 2 ids, may be NULL): the scope of the result table,
 * slowest first, B reported as the id n_vars -- (B), (target, B), or without B
 * when no evidence reaches the result. */
int bnpp_plan_batch(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order, int n_order,
                    int target, int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows,
                    int cap_rows, int *n_rows, int *result_scope, int *n_result_scope);

/* Host-only planning of bnpp_mpe_batch, modelled on bnpp_plan_batch:
 * stats[0..10) as bnpp_plan_batch's ([8] the rows per launch R, [9] the gather
 * steps), then [10] arg_bytes, the bytes of all arg tables before alignment,
 * [11] the max buckets, [12] the arg tables that carry B and [13] those that do
 * not, [14] the entries per row of the former (summed) and [15] the entries of
 * the latter: arg_bytes = [14] * R + [15].  rows as bnpp_plan_groups's: the
 * gather steps at level 0 (key 2^24 + 12288), max-family keys and product keys,
 * and the traceback step as the last group, key 2^24 + 20480. */
#define BNPP_PLAN_MPE_BATCH_STATS 16
int bnpp_plan_mpe_batch(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order, int n_order,
                        int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows, int cap_rows,
                        int *n_rows);

/* Host-only planning of bnpp_sample_batch, modelled on bnpp_plan_mpe_batch:
 * stats[0..10) as bnpp_plan_batch's ([1] the arena bytes, the state included,
 * [8] the rows per launch R, [9] the gather steps), then [10] K = n_per_row,
 * [11] the state bytes n_vars * R * K, [12] the draw rows (one per
 * non-evidence variable), [13] those with an input that carries B and [14]
 * those without.  rows as bnpp_plan_groups's: the gather steps at level 0 (key
 * 2^24 + 12288), ordinary sum-plan keys (no chain key), and the draw step as
 * the last group, key 2^24 + 24576. */
#define BNPP_PLAN_SAMPLE_BATCH_STATS 15
int bnpp_plan_sample_batch(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order, int n_order,
                           int dtype, int64_t rows_per_launch, int64_t n_per_row, double *stats, int n_stats,
                           int64_t *rows, int cap_rows, int *n_rows);

/* Host-only planning of bnpp_expected_counts, modelled on bnpp_plan_batch:
 * stats[0..10) as bnpp_plan_batch's, then [10] the accumulate steps (one per
 * factor, key 2^24 + 16384, one group each) and [11] the last level of the
 * forward pass -- the groups up to that level are bnpp_plan_batch's for the
 * same arguments; rows as bnpp_plan_groups's.  belief_off[n_factors + 1] and
 * belief_vars[cap_belief] (may be NULL): per factor the variables of the
 * belief table its accumulate step reads, slowest first, B reported as the id
 * n_vars; *n_belief the ids in all.  no_b_elim (may be NULL): 1 when no bucket
 * of the plan sums B or holds it inside a composite variable. */
int bnpp_plan_counts(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order, int n_order,
                     int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows, int cap_rows,
                     int *n_rows, int *belief_off, int *belief_vars, int cap_belief, int *n_belief, int *no_b_elim);

/* Host-only planning of bnpp_marginals_batch, modelled on bnpp_plan_counts:
 * stats[0..10) as bnpp_plan_batch's ([1] the arena bytes, the output table
 * included), then [10] the emit steps (1; key 2^24 + 28672, the last group, at
 * a level of its own), [11] the last level of the forward pass -- the groups up
 * to that level are bnpp_plan_batch's for the same arguments --, [12] the belief
 * column blocks, [13] the evidence blocks, [14] the free blocks, [15] W, [16]
 * the output bytes per launch (R * W * 8) and [17] the belief blocks whose table
 * carries B; rows as bnpp_plan_groups's.  targets NULL: all variables.
 * col_kind[n_targets] (may be NULL): per target 1 a belief with B, 0 a belief
 * without, -1 an evidence block, -2 a free block. */
#define BNPP_PLAN_MARGINALS_BATCH_STATS 18
int bnpp_plan_marginals_batch(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order,
                              int n_order, int n_targets, const int *targets, int dtype, int64_t rows_per_launch,
                              double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *col_kind);

/* ------------------------------------------------ missing values (batched calls)
 * The batched calls above take ONE evidence variable set per call and no
 * "missing" value.  The _mv siblings take one more argument, partial[n_ev] (or
 * NULL): partial[j] != 0 declares ev_vars[j] PARTIAL -- ev_vals may then hold
 * BNPP_MISSING (-1) for it in any row.  Row b's result is, by definition, the
 * single call's for evidence equal to the row's observed entries.
 *
 * A partial variable is not conditioned away: it stays a model variable, it is
 * eliminated (the order is computed from the other, "hard", evidence variables
 * only, and an explicit order covers it where it covers the non-evidence
 * variables), and exactly ONE factor that holds it is gathered under a per-row
 * 0/1 mask (masked gather step, launch-group key 2^24 + 32768, level 0):
 *   out[rest][b] = in[hard offsets(b) + offset(rest)]  if for every partial p of the scope
 *                                                      ev[p][b] < 0 or ev[p][b] == digit_p(rest)
 *                  0                                   otherwise
 * The factor: 1. one that holds a hard evidence variable (it is gathered
 * anyway); 2. among those, else among all factors that hold the variable, the
 * fewest entries after conditioning; 3. the lowest factor index.  A partial
 * variable in no factor carries no mask.  Everything downstream is the code of
 * the call without the argument, so row b equals that call on the model whose
 * mask-carrying factors were multiplied by row b's indicator, with the hard
 * evidence only.  Width, message sizes and cost are those of a call WITHOUT the
 * partial variables as evidence; a mask on a factor with no hard evidence makes
 * its gathered table R times the factor.  The shared scale of a launch applies.
 * partial == NULL (or all zero) is the call without the argument, bit for bit;
 * the entries without _mv pass NULL, and -1 stays BNPP_ERR_INVALID there.
 * -1 in a column that is not partial, any value below -1 and any value >= the
 * card are BNPP_ERR_INVALID naming the row and the variable.  A posterior
 * target may not be listed as evidence, partial or not.  bnpp_mpe_batch_mv and
 * bnpp_sample_batch_mv write the observed entries of partial variables from the
 * row (impossible rows included).  The job cache key includes the flags.
 * bnpp_plan_*_mv also return mask_factor[n_ev] (may be NULL): the factor that
 * carries variable j's mask, -1 for a hard variable or one in no factor.
 * bnpp_condition_batch_mv runs the (masked) gather on caller-owned device
 * buffers: a partial variable of the scope stays a dim of `out`; a negative
 * value of it is "missing", a value >= its card matches nothing (zeros, no
 * read).  bnpp_evidence_load_batch_mv reads an .evid file whose samples observe
 * differing variable sets: ev_vars is the union, ascending, ev_vals holds -1
 * where a sample is silent and partial[j] = 1 for a variable some sample lacks
 * (capacity protocol of bnpp_evidence_load_batch). */
#define BNPP_MISSING (-1)
int bnpp_partition_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int heuristic, const int *order,
                            int n_order, int dtype, int64_t rows_per_launch, double *log10_z, double *z,
                            double *uptime_ms);

int bnpp_posterior_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int heuristic, int target, int dtype,
                            int64_t rows_per_launch, double *out, double *uptime_ms);

int bnpp_mpe_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                      const int *ev_vals, const unsigned char *partial, int heuristic, const int *order, int n_order,
                      int dtype, int64_t rows_per_launch, double *log10_value, int *assignment, double *uptime_ms);

int bnpp_sample_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals, const unsigned char *partial, int heuristic, const int *order,
                         int n_order, int dtype, int64_t rows_per_launch, int64_t n_per_row, int64_t first_sample,
                         int64_t row_stride, uint64_t seed, uint8_t *out, double *log10_z, int64_t *n_degenerate,
                         double *uptime_ms);

int bnpp_expected_counts_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, const double *weights, int heuristic,
                            const int *order, int n_order, int dtype, int64_t rows_per_launch, double *counts,
                            double *log10_z, int64_t *n_impossible, double *uptime_ms);

int bnpp_marginals_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int heuristic, const int *order,
                            int n_order, int n_targets, const int *targets, int dtype, int64_t rows_per_launch,
                            double *out, double *log10_z, double *uptime_ms);

int bnpp_plan_batch_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int heuristic,
                       const int *order, int n_order, int target, int dtype, int64_t rows_per_launch, double *stats,
                       int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *result_scope, int *n_result_scope,
                       int *mask_factor);

int bnpp_plan_mpe_batch_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial,
                           int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                           double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *mask_factor);

int bnpp_plan_sample_batch_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial,
                              int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                              int64_t n_per_row, double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows,
                              int *mask_factor);

int bnpp_plan_counts_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial,
                        int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                        double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *belief_off,
                        int *belief_vars, int cap_belief, int *n_belief, int *no_b_elim, int *mask_factor);

int bnpp_plan_marginals_batch_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial,
                                 int heuristic, const int *order, int n_order, int n_targets, const int *targets,
                                 int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows,
                                 int cap_rows, int *n_rows, int *col_kind, int *mask_factor);

int bnpp_condition_batch_mv(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in,
                            int ndims, const int *vars, int n_ev, const int *ev_vars,
                            const unsigned char *partial /* [n_ev] or NULL */, int64_t n_rows,
                            const int32_t *ev /* device, [n_ev][n_rows] */, void *out);
int bnpp_evidence_load_batch_mv(const char *path, int cap_vars, int64_t cap_rows, int *n_ev, int *ev_vars,
                                int64_t *n_rows, int *ev_vals, unsigned char *partial /* [cap_vars] */);

/* ------------------------------------------------ soft evidence (batched calls)
 * A row can say "X = 2" (hard) or "X unknown" (missing).  The _sv siblings let
 * it say "X is 0/1/2 with likelihoods 0.7/0.2/0.1": beside ev_vars / partial
 * they name SOFT variables soft_vars[n_soft] and lik, double[n_rows][Ws]
 * row-major with Ws = sum card(soft_vars[i]); the variables' blocks come in the
 * listed order (the layout bnpp_marginals_batch returns).  Row b's result is,
 * by definition, the _mv call's result on the model that has one more unary
 * factor lik_b,i on each soft_vars[i], with the row's hard and partial evidence.
 * Hard and missing values are the corners: a one-hot and an all-ones block.
 *
 * Values: every likelihood is finite and >= 0, with no upper bound.  A NaN, an
 * inf or a negative value is BNPP_ERR_INVALID naming the row and the variable,
 * checked with the rows, before the context is looked at.  A (row, variable)
 * block of all zeros makes the row impossible: it reads as an impossible row of
 * the call reads (-inf, NaN or zeros, n_impossible, every draw degenerate); its
 * neighbours keep their bits.
 *
 * Scaling: the runtime multiplies each (row, variable) block by an exact power
 * of two so that its largest entry lies in [0.5, 1), sums the exponents per row
 * (e_b) and gives them back: log10_z[b] and log10_value[b] are the logarithm of
 * p * 2^(exp2 + e_b), z[b] is scaled by 2^e_b.  Posteriors, marginals, counts,
 * assignments and samples do not see the scale.  Every weight is then at most
 * 1, so a gathered table keeps its source's bound, and rows of any magnitude
 * share a launch.  The scaled block is converted to the call's dtype.
 *
 * Arguments: a variable in both ev_vars and soft_vars, one listed twice and an
 * id out of range are BNPP_ERR_INVALID.  A soft variable in no factor is
 * BNPP_ERR_UNSUPPORTED, naming it: its likelihoods would scale Z with no table
 * to carry them.  The target of bnpp_posterior_batch_sv may not be soft; a soft
 * target of bnpp_marginals_batch_sv is a belief column and reads the posterior
 * with its likelihoods included.  n_ev = 0 with n_soft > 0 is a valid call.
 * Sampling keeps its limit of 256 values for a sampled variable.  n_soft = 0 is
 * the _mv call, bit for bit (plans, groups, stats, job keys, results); the _mv
 * entries pass 0.  partial may be NULL.
 *
 * Planning: a soft variable stays a model variable, as a partial one does: the
 * order comes from the hard evidence variables only; it is eliminated,
 * maximised, drawn and counted like any other variable (bnpp_mpe_batch_sv and
 * bnpp_sample_batch_sv write it from the traceback and the draws).  Exactly ONE
 * factor that holds it carries its likelihoods, by the rule of the masks:
 * 1. a factor that holds a hard evidence variable; 2. among those, else among
 * all its factors, the fewest entries after conditioning; 3. the lowest index.
 * That factor is gathered by the weighted gather step (launch-group key
 * 2^24 + 36864, level 0, one group per step), masks and weights together:
 *   out[rest][b] = mask_b(rest) ? ((in[hard offsets(b) + offset(rest)] * lam_d1[digit_d1][b]) * lam_d2[digit_d2][b]) ... : 0
 * the soft dims d1, d2, ... in the order of the factor's scope, left to right,
 * each product rounded once in the call's dtype.  A soft dim is never merged
 * with a neighbour and counts against the 8 rest dims of a gather step
 * (BNPP_ERR_UNSUPPORTED).  The job cache key includes the soft variable list,
 * never the values: a call with other likelihoods relaunches the cached job.
 * bnpp_plan_*_sv ignore lik (it may be NULL) and also return lam_factor[n_soft]
 * (may be NULL): the factor that carries variable i's likelihoods.
 *
 * bnpp_condition_batch_sv runs the weighted gather on caller-owned device
 * buffers: lam is T[Ws][n_rows] in the call's dtype, (variable, value)-major,
 * rows fastest, used as it is (no scaling); a soft variable of the scope stays
 * a dim of `out`, one outside the scope is ignored.
 * bnpp_likelihood_load reads a text file: n_soft, the ids, n_rows, then Ws
 * numbers per row.  n_soft and n_rows are always set; soft_vars is filled when
 * cap_vars >= n_soft, and lik when also cap_vals >= n_rows * Ws (else
 * BNPP_ERR_INVALID, so a caller may ask for the sizes, then the ids, first). */
int bnpp_expected_counts_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows, const
                            int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars, const
                            double *lik, const double *weights, int heuristic, const int *order, int n_order, int
                            dtype, int64_t rows_per_launch, double *counts, double *log10_z, int64_t *n_impossible,
                            double *uptime_ms);

int bnpp_plan_counts_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int n_soft,
                        const int *soft_vars, const double *lik, int heuristic, const int *order, int n_order, int
                        dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows, int cap_rows, int
                        *n_rows, int *belief_off, int *belief_vars, int cap_belief, int *n_belief, int *no_b_elim,
                        int *mask_factor, int *lam_factor);

int bnpp_marginals_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows, const
                            int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars, const
                            double *lik, int heuristic, const int *order, int n_order, int n_targets, const int
                            *targets, int dtype, int64_t rows_per_launch, double *out, double *log10_z, double
                            *uptime_ms);

int bnpp_plan_marginals_batch_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial,
                                 int n_soft, const int *soft_vars, const double *lik, int heuristic, const int
                                 *order, int n_order, int n_targets, const int *targets, int dtype, int64_t
                                 rows_per_launch, double *stats, int n_stats, int64_t *rows, int cap_rows, int
                                 *n_rows, int *col_kind, int *mask_factor, int *lam_factor);

int bnpp_partition_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows, const
                            int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars, const
                            double *lik, int heuristic, const int *order, int n_order, int dtype, int64_t
                            rows_per_launch, double *log10_z, double *z, double *uptime_ms);

int bnpp_posterior_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows, const
                            int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars, const
                            double *lik, int heuristic, int target, int dtype, int64_t rows_per_launch, double *out,
                            double *uptime_ms);

int bnpp_mpe_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows, const int
                      *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars, const double *lik,
                      int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch, double
                      *log10_value, int *assignment, double *uptime_ms);

int bnpp_plan_mpe_batch_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int
                           n_soft, const int *soft_vars, const double *lik, int heuristic, const int *order, int
                           n_order, int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows,
                           int cap_rows, int *n_rows, int *mask_factor, int *lam_factor);

int bnpp_sample_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows, const int
                         *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars, const double
                         *lik, int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                         int64_t n_per_row, int64_t first_sample, int64_t row_stride, uint64_t seed, uint8_t *out,
                         double *log10_z, int64_t *n_degenerate, double *uptime_ms);

int bnpp_plan_sample_batch_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int
                              n_soft, const int *soft_vars, const double *lik, int heuristic, const int *order, int
                              n_order, int dtype, int64_t rows_per_launch, int64_t n_per_row, double *stats, int
                              n_stats, int64_t *rows, int cap_rows, int *n_rows, int *mask_factor, int *lam_factor);

int bnpp_plan_batch_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int n_soft,
                       const int *soft_vars, const double *lik, int heuristic, const int *order, int n_order, int
                       target, int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows, int
                       cap_rows, int *n_rows, int *result_scope, int *n_result_scope, int *mask_factor, int
                       *lam_factor);

int bnpp_condition_batch_sv(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in,
                            int ndims, const int *vars, int n_ev, const int *ev_vars,
                            const unsigned char *partial /* [n_ev] or NULL */, int n_soft, const int *soft_vars,
                            const void *lam /* device, T[Ws][n_rows] */, int64_t n_rows,
                            const int32_t *ev /* device, [n_ev][n_rows] */, void *out);
int bnpp_likelihood_load(const bnpp_model *m, const char *path, int cap_vars, int64_t cap_vals, int *n_soft,
                         int *soft_vars, int64_t *n_rows, double *lik);

/* ------------------------------- device-resident batched calls (_dv) */
/* The _sv calls with every row array in device memory: ev_vals
 * (int32[n_rows][n_ev]) and lik ([n_rows][Ws], doubles or floats: lik_dtype is
 * BNPP_F64 or BNPP_F32, floats are widened exactly; with BNPP_LIK_LOG: natural
 * logs, see "the log form" below) are read from the
 * context's device, and log10_z, z, out, log10_value, assignment, samples and
 * n_degenerate are written there.  The variable lists, partial, order and
 * targets stay host arrays.  Row b's results are, by definition, the _sv
 * sibling's for the same arguments: z, the marginals, the assignments, the
 * samples and n_degenerate bit for bit, log10_z and log10_value within 4 ulp of
 * max(|value|, 1) (the device's log10 of the mantissa is the one operation
 * that is not the host's).  The plan, R and the job cache key are the
 * sibling's, so the two forms share a cached job.
 * Everything is enqueued on the context's stream in order: per launch the two
 * staging steps below, the plan's kernels and the emit steps, with no host wait
 * between launches; the call waits for the stream once, at its end, so the
 * outputs are complete when it returns.  Work on another stream that produces
 * the inputs must have been ordered before the context's stream by the caller.
 * The variable sets, partial, soft_vars, targets, order, dtype, lik_dtype,
 * rows_per_launch, n_per_row, first_sample, row_stride and the null checks are
 * validated on the host as by the sibling (and fail the same without a
 * device); the values are validated on the device: the first bad evidence
 * cell in row-major order, else the first bad likelihood, returns
 * BNPP_ERR_INVALID with the sibling's message.  After an error the outputs
 * are unspecified.  BNPP_TIMING prints the call's stage / enqueue / wait. */
int bnpp_partition_batch_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int32_t *ev_vals /* device */, const unsigned char *partial, int n_soft,
                            const int *soft_vars, const void *lik /* device */, int lik_dtype, int heuristic,
                            const int *order, int n_order, int dtype, int64_t rows_per_launch,
                            double *log10_z /* device, [n_rows] */, double *z /* device, [n_rows] or NULL */,
                            double *uptime_ms);
int bnpp_marginals_batch_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int32_t *ev_vals /* device */, const unsigned char *partial, int n_soft,
                            const int *soft_vars, const void *lik /* device */, int lik_dtype, int heuristic,
                            const int *order, int n_order, int n_targets, const int *targets, int dtype,
                            int64_t rows_per_launch, double *out /* device, [n_rows][W] */,
                            double *log10_z /* device, [n_rows] or NULL */, double *uptime_ms);
int bnpp_mpe_batch_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                      const int32_t *ev_vals /* device */, const unsigned char *partial, int n_soft,
                      const int *soft_vars, const void *lik /* device */, int lik_dtype, int heuristic,
                      const int *order, int n_order, int dtype, int64_t rows_per_launch,
                      double *log10_value /* device, [n_rows] or NULL */,
                      int32_t *assignment /* device, [n_rows][n_vars] or NULL */, double *uptime_ms);
int bnpp_sample_batch_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int32_t *ev_vals /* device */, const unsigned char *partial, int n_soft,
                         const int *soft_vars, const void *lik /* device */, int lik_dtype, int heuristic,
                         const int *order, int n_order, int dtype, int64_t rows_per_launch, int64_t n_per_row,
                         int64_t first_sample, int64_t row_stride, uint64_t seed,
                         uint8_t *out /* device, [n_rows][n_per_row][n_vars] or NULL */,
                         double *log10_z /* device, [n_rows] or NULL */,
                         int64_t *n_degenerate /* device, [n_rows] or NULL */, double *uptime_ms);

/* The four steps of the _dv calls on caller-owned device buffers (rowio.cuh).
 * A launch of R rows starts at row row0 of the call's n_rows; its entry b is
 * row min(row0 + b, n_rows - 1) (the last launch is padded with the last row);
 * rows_live of its entries are the call's.  status is int64[2] on the device,
 * set to INT64_MAX by the caller beforehand; only an invalid cell touches it,
 * by an atomic minimum, so afterwards a word that is not INT64_MAX names the
 * first invalid cell in row-major order.  Results do not depend on the grid.
 *
 * bnpp_stage_evidence_rows: ev = int32[n_rows][n_ev] to out = int32[n_ev][R],
 *   out[j][b] = ev[min(row0 + b, n_rows - 1)][j].  A value x is valid when
 *   0 <= x < cards[j], or x == -1 and partial[j] (partial may be NULL); an
 *   invalid value is stored as 0 and its cell index row * n_ev + j folded into
 *   status[0].  At most 320 columns.
 * bnpp_stage_likelihoods: lik = [n_rows][Ws] (lik_dtype) to out = T[Ws][R]
 *   (dtype) and e_row = int64[R]; Ws = sum of cards, at most 320 variables.
 *   Per (row, variable) block: top = its largest entry, e = frexp's exponent of
 *   top (0 when top == 0), every entry ldexp(v, -e) rounded once to T (to the
 *   nearest even, subnormal floats included); e_row[b] = the sum of the row's
 *   e.  An entry that is NaN, infinite or negative counts as 0 and its cell
 *   index row * Ws + w is folded into status[1].
 * bnpp_emit_row_scalars: p = (double)table[has_b ? b : 0] (table NULL: 1),
 *   ex = meta->exp2 (meta: a device int64[4] whose third word is the scale;
 *   NULL: 0) + e_row[b] (NULL: 0);
 *   log10_z[row0 + b] = p > 0 ? log10(frexp mantissa of p) + (double)(ex +
 *   frexp exponent of p) * log10(2) : -inf, every operation in fp64 and rounded
 *   once; z[row0 + b] = ldexp(p, clamp(ex, -2^20, 2^20)) (z may be NULL); for
 *   b < rows_live.
 * bnpp_emit_row_states: x = uint8[n_vars][K][R], ev = the staged int32[n_ev][R].
 *   Per variable v: ev_col[v] (-1: none) and written[v] (a step wrote x's row
 *   of v).  Cell (row0 + b, s, v), b < rows_live, is ev[ev_col[v]][b] when that
 *   is >= 0 (observed), else x[v][s][b] when written[v], else 0.
 *   sampling == 0: K = 1, out = int32[n_rows][n_vars]; table, deg and
 *   n_degenerate are ignored.  sampling != 0: out = uint8[n_rows][K][n_vars];
 *   a row whose p (as above) is not > 0 reads 0 in every cell that is not
 *   observed and n_degenerate[row0 + b] = K * n_drawn, every other row
 *   n_degenerate[row0 + b] = deg[b] (n_degenerate may be NULL).  At most 320
 *   variables. */
int bnpp_stage_evidence_rows(bnpp_ctx *ctx, void *stream, int n_ev, const int *cards, const unsigned char *partial,
                             int64_t n_rows, int64_t row0, int64_t R, const int32_t *ev, int32_t *out,
                             int64_t *status);
int bnpp_stage_likelihoods(bnpp_ctx *ctx, void *stream, int dtype, int lik_dtype, int n_soft, const int *cards,
                           int64_t n_rows, int64_t row0, int64_t R, const void *lik, void *out, int64_t *e_row,
                           int64_t *status);
int bnpp_emit_row_scalars(bnpp_ctx *ctx, void *stream, int dtype, const void *table, int has_b, const void *meta,
                          const int64_t *e_row, int64_t row0, int64_t rows_live, double *log10_z, double *z);
int bnpp_emit_row_states(bnpp_ctx *ctx, void *stream, int sampling, int n_vars, const int *ev_col,
                         const unsigned char *written, int64_t K, int64_t R, int64_t row0, int64_t rows_live,
                         const uint8_t *x, const int32_t *ev, int dtype, const void *table, int has_b,
                         const uint64_t *deg, int64_t n_drawn, void *out, int64_t *n_degenerate);

/* ------------------------------------ log-space soft evidence (the log form) */
/* lik_dtype BNPP_F64 | BNPP_LIK_LOG (2) or BNPP_F32 | BNPP_LIK_LOG (3): the
 * likelihood array of a _dv call holds natural logs l[b][v][x], doubles or
 * floats (widened exactly).  An entry is valid when it is finite or -inf (the
 * likelihood 0); NaN and +inf count as -inf and are named by the error
 * "evidence row R: the likelihood of value X of soft variable V must not be
 * NaN or +inf".  Row b's results are the linear call's for lik = E, where
 * E[b][v][x] = exp(l[b][v][x] - top[b][v]) and top is the block's largest entry
 * (a block of nothing but -inf: E = 0 throughout, an impossible row):
 * marginals, assignments, samples and n_degenerate bit for bit, log10_z and
 * log10_value with shift_b * log10(e) added, shift_b being the fp64 sum of the
 * row's tops taken from 0.0 in soft_vars order; z = exp of the row's natural
 * log, which may overflow to inf and carries no bit contract.  The plans and job
 * keys are the linear calls'.  The host-array calls have no log form.
 *
 * bnpp_stage_loglikelihoods: bnpp_stage_likelihoods for the log form, with
 *   top = double[n_soft][R].  Per (row, variable) block: top = its largest
 *   entry after invalid ones are replaced by -inf.  top == -inf: every entry is
 *   stored as 0 and the block adds 0 to e_row.  Else every entry is
 *   ldexp(exp(v - top), -1) (the difference rounded once), rounded once to T,
 *   and the block adds 1 to e_row: what bnpp_stage_likelihoods makes of E,
 *   whose largest entry is 1.0 = 0.5 * 2^1.  The cell index of an invalid entry
 *   is folded into status[1].
 * bnpp_emit_row_logs: p, ex as bnpp_emit_row_scalars, pm and pe the frexp
 *   mantissa and exponent of p, shift = the sum of top[i][b], i = 0 .. n_soft-1
 *   in order from 0.0 (n_soft 0: 0.0);
 *   ln_z[row0 + b] = p > 0 ? (ln(pm) + (double)(ex + pe) * 0x1.62e42fefa39efp-1) + shift : -inf,
 *   log10_z[row0 + b] = p > 0 ? (log10(pm) + (double)(ex + pe) * 0x1.34413509f79ffp-2)
 *                               + shift * 0x1.bcb7b1526e50ep-2 : -inf,
 *   z[row0 + b] = exp(ln_z); every operation in fp64 and rounded once.  Each of
 *   the three outputs may be NULL (not all).
 * bnpp_log_partition_dv: ln Z of every row, and with post != NULL (and
 *   n_soft > 0) the posterior of every soft variable, post[b][w] over the Ws
 *   columns of loglik: d ln Z_b / d l[b][v][x] = P(X_v = x | row b), the
 *   likelihoods included, so post is the gradient of ln_z.  post == NULL: the
 *   batch plan (the job and key of bnpp_partition_batch_dv); else the batched
 *   marginals plan with targets = soft_vars (the job of
 *   bnpp_marginals_batch_dv on those targets), ln_z from its result table and
 *   post written as that call writes out (an impossible row: NaN).  n_soft == 0
 *   is valid: ln_z of the hard evidence, post untouched.  lik_dtype must be 2 or
 *   3.  The host-side checks are the siblings'. */
int bnpp_stage_loglikelihoods(bnpp_ctx *ctx, void *stream, int dtype, int lik_dtype, int n_soft, const int *cards,
                              int64_t n_rows, int64_t row0, int64_t R, const void *loglik, void *out, int64_t *e_row,
                              double *top, int64_t *status);
int bnpp_emit_row_logs(bnpp_ctx *ctx, void *stream, int dtype, const void *table, int has_b, const void *meta,
                       const int64_t *e_row, int n_soft, const double *top, int64_t R, int64_t row0, int64_t rows_live,
                       double *ln_z, double *log10_z, double *z);
int bnpp_log_partition_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                          const int32_t *ev_vals /* device */, const unsigned char *partial, int n_soft,
                          const int *soft_vars, const void *loglik /* device */, int lik_dtype /* 2 or 3 */,
                          int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                          double *ln_z /* device, [n_rows] */, double *post /* device, [n_rows][Ws], or NULL */,
                          double *uptime_ms);

/* ------------------------------------------ device-resident model tables
 * A model is read-only after creation, and the planner reads only its scopes
 * and cards.  A bnpp_tables is the tables of one model on one context in one
 * dtype, rewritten in place on the device: one plan, one job and one program
 * serve every iteration of a training loop.  Symbols added to version 205.
 *
 * bnpp_tables_create: the set starts as the model's own values.  It owns the
 *   layout the engine uploads a model in (every factor pre-scaled by a power of
 *   two, on a 256-byte line), the factors' metadata on the device, one device
 *   double `shift` and a uid of its own from the counter of the models' uids.
 *   The buffer's address never changes; only its bytes and the factors'
 *   maxbits / exp2 words do.  The set keeps what it needs of the model (the
 *   sizes), so bnpp_model_free leaves it valid but useless: a call takes the
 *   set together with the model it was created for.  bnpp_ctx_destroy takes
 *   back the buffers of its context's sets: such a set can still be freed, and
 *   every other use of it is BNPP_ERR_INVALID.  A set is not synchronised
 *   against calls of other threads.
 * bnpp_tables_free: a cached job planned for the set is evicted first.
 * bnpp_tables_set_dv: values is one flat device array in the layout of counts
 *   (bnpp_counts_size entries: the factors in model order, each in its natural
 *   layout), doubles or floats (widened exactly).  One step on the context's
 *   stream (bnpp_stage_tables states it), then the call waits and reports the
 *   first invalid entry as BNPP_ERR_INVALID, naming the factor and the entry's
 *   index in it; the set then holds the valid entries and 0 for the others.
 * bnpp_stage_tables: the step on caller-owned buffers.  Factor f has sizes[f]
 *   entries, starts at the sum of the earlier sizes in values and at the sum of
 *   the earlier factors' bytes, each rounded up to 256, in out_buf.  out_meta
 *   is n_factors records {void *ptr; uint64 maxbits; int64 exp2; int64 size},
 *   out_shift is double[1 + n_factors] (the shift, then every factor's top),
 *   status one int64 the caller sets to INT64_MAX: it receives the smallest
 *   flat index of an invalid entry.  At most 96 factors.  Per factor,
 *   linear form (values_dtype 0 or 1): an entry that is NaN, infinite or
 *     negative is invalid and counts as 0; top = the largest entry; e = the
 *     exponent frexp gives top (0 for top = 0); stored entry = ldexp(v, -e),
 *     converted once to dtype; maxbits = the bits of the largest stored entry,
 *     exp2 = e; shift = 0.  This is what the engine makes of a model's values.
 *   log form (values_dtype | BNPP_LIK_LOG): the entries are natural logs, -inf
 *     the value 0; NaN and +inf are invalid and count as -inf; top = the largest
 *     entry; stored entry = exp(l - top) / 2, exp2 = 1, maxbits = the bits of
 *     0.5; a factor of nothing but -inf is stored as zeros with exp2 = 0 and
 *     maxbits = 0.  shift = the sum of the tops in factor order from 0.0, in
 *     fp64, every add rounded once, the factors of nothing but -inf left out.
 *   Nothing depends on the grid (bnpp_ctx_set_max_grid).
 * bnpp_expected_counts_dv: bnpp_expected_counts_sv with every per-row array
 *   (ev_vals, lik, weights) and every output in device memory.  tables == NULL:
 *   the model's own values, and without a flag counts are the host-array
 *   call's bit for bit, log10_z as the other _dv calls' (the device's log10),
 *   n_impossible equal; the plan, R and the cached job are that call's.  With
 *   tables (of this model, this dtype and this context, else
 *   BNPP_ERR_INVALID) the call reads them instead, under a job key of their
 *   own; after a linear set of v the results are those of tables == NULL on a
 *   model made of v, bit for bit.  After a log set ln_z and log10_z include
 *   the set's shift (ln Z of the tables exp(l)); counts are those of exp(l).
 *   flags: BNPP_COUNTS_ACCUMULATE adds to what counts holds, continuing the
 *   fold between launches across calls; else counts is zeroed first.  weights:
 *   device, or NULL for 1; the first weight that is not finite or is negative
 *   is reported with the sibling's message.  log10_z, ln_z and n_impossible
 *   (one int64, the rows with Z = 0) may each be NULL.  counts == NULL: the
 *   batch plan (the job of bnpp_partition_batch_dv) under the tables -- the
 *   rows' likelihood without the backward pass; weights are then not read,
 *   and one of log10_z and ln_z is needed.
 * bnpp_mstep_dv: the M step of a BAYES model (else BNPP_ERR_UNSUPPORTED), all
 *   factors in one launch on `stream` (NULL: the context's), not waited for.
 *   A factor's child is the last variable of its scope (k values), so a parent
 *   configuration is k contiguous entries: num_i = counts_i + prior,
 *   tot = ((0.0 + num_0) + num_1) + ..., new_i = tot > 0 ? num_i / tot : old_i,
 *   in fp64, every operation rounded once.  new_values may be old_values; it
 *   must not overlap counts.  prior must be finite and not negative.  The
 *   context keeps the per-factor words of the last model on the device; when
 *   the model changes, the call waits for the stream of the last M step (not
 *   for the device) before it uploads the new ones. */
#define BNPP_COUNTS_ACCUMULATE 1
typedef struct bnpp_tables bnpp_tables;
int bnpp_tables_create(bnpp_ctx *ctx, const bnpp_model *m, int dtype, bnpp_tables **out);
int bnpp_tables_free(bnpp_tables *t);
int bnpp_tables_set_dv(bnpp_tables *t, const void *values /* device, flat */, int values_dtype);
int bnpp_stage_tables(bnpp_ctx *ctx, void *stream, int dtype, int values_dtype, int n_factors, const int64_t *sizes,
                      const void *values, void *out_buf, void *out_meta, double *out_shift, int64_t *status);
int bnpp_expected_counts_dv(bnpp_ctx *ctx, const bnpp_model *m, const bnpp_tables *tables /* NULL: the model's own */,
                            int n_ev, const int *ev_vars, int64_t n_rows, const int32_t *ev_vals /* device */,
                            const unsigned char *partial, int n_soft, const int *soft_vars, const void *lik /* device */,
                            int lik_dtype, const double *weights /* device or NULL */, int flags, int heuristic,
                            const int *order, int n_order, int dtype, int64_t rows_per_launch,
                            double *counts /* device, or NULL */, double *log10_z, double *ln_z,
                            int64_t *n_impossible /* device or NULL */, double *uptime_ms);
int bnpp_mstep_dv(bnpp_ctx *ctx, void *stream, const bnpp_model *m, const double *counts, double prior,
                  const double *old_values, double *new_values /* may alias old_values */);

/* Host-only planning of one part of bnpp_marginals_tree_part (all variables
 * as targets): owned[v] = 1 when this part computes v's marginal; stats as
 * bnpp_job_stats for this part's plan (may be NULL).  The memory budget is
 * BNPP_MEM_BUDGET_GB or 64 GB (no device is consulted). */
int bnpp_plan_tree_part(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                        const int *order, int n_order, int part, int n_parts, int dtype, int *owned, double *stats,
                        int n_stats);

/* Host-only planning of one rank of bnpp_marginals_tree_sliced (all
 * variables as targets): slice_bit[v] (may be NULL) = the rank bit that
 * indexes v's scalar share (-1: a table over v); stats as bnpp_job_stats, then
 * [8] message exchanges, [9] bytes this rank sends per call. */
int bnpp_plan_tree_sliced(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                          const int *order, int n_order, int rank, int n_ranks, int dtype, int *slice_bit,
                          double *stats, int n_stats);

/* ------------------------------------------- prepared jobs (benchmark) */
/* A planned, device-resident inference that can be launched repeatedly. */
typedef struct bnpp_job bnpp_job;
/* kind 0: partition (targets ignored)   kind 1: marginals of `targets` (one VE
 * each)   kind 3: marginals of `targets` from one bucket tree   kind 4: MPE
 * (targets ignored) */
int bnpp_job_create(bnpp_ctx *ctx, const bnpp_model *m, int kind, int n_ev, const int *ev_vars,
                    const int *ev_vals, int heuristic, const int *order, int n_order, int n_targets,
                    const int *targets, int dtype, bnpp_job **out);
/* stats: [0] factor-entries per launch, [1] arena bytes, [2] levels, [3] buckets,
 *        [4] max induced width, [5] largest message entries, [6] algorithmic bytes,
 *        [7] target batches */
int bnpp_job_stats(const bnpp_job *job, double *stats, int n_stats);
int bnpp_job_launch(bnpp_job *job, void *stream);
/* waits on stream; partition: out[0] = log10 Z; marginals: sum(card) values;
 * MPE: out[0] = log10 of the maximum, then the n_vars assignment entries */
int bnpp_job_results(bnpp_job *job, void *stream, double *out);
int bnpp_job_free(bnpp_job *job);

#ifdef __cplusplus
}
#endif
#endif
