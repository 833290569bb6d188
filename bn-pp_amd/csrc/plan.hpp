// Host-side planning for the fused bucket kernels (no HIP calls; unit-testable on CPU).
#pragma once
#include <cstdint>
#include <climits>
#include <cstdlib>
#include <functional>
#include <string>
#include <memory>
#include <utility>
#include <vector>

#include "bnpp_device.h"

namespace bnpp {

// Environment switches.  The product reads only the switches the tests use to
// compare kernel forms and plan shapes bit for bit (BNPP_NO_CHAIN, _NO_SPLIT,
// _NO_DENSE, _NO_SLAB, _NO_BEL_FUSE, _TREE_SLOTS, _KEEP_LOG2, ...), the memory
// budget and diagnostics.  Tuning knobs -- launch shapes and layouts measured
// once and settled (tools/) -- are read only by a build with
// -DBNPP_TUNING_KNOBS (tools/build_variant.sh); elsewhere they read as unset.
#ifdef BNPP_TUNING_KNOBS
inline const char *tuning_knob(const char *name) { return std::getenv(name); }
#else
inline const char *tuning_knob(const char *) { return nullptr; }
#endif
// the switches that change a plan (the job cache and the slot memo key on them)
constexpr const char *kPlanKnobs[] = {"BNPP_NO_CHAIN", "BNPP_NO_SPLIT", "BNPP_NO_DENSE", "BNPP_NO_SLAB",
                                      "BNPP_NO_SLAB_OUTER", "BNPP_NO_BEL_FUSE", "BNPP_NO_CHAIN_FWDV",
                                      "BNPP_NO_FREE_REDUCE", "BNPP_NO_REDUCE_MANY", "BNPP_NO_DEDUP",
                                      "BNPP_TREE_SLOTS", "BNPP_KEEP_LOG2", "BNPP_SLOW_LOG2", "BNPP_SPLIT_MIN_F",
                                      "BNPP_CHAIN_RUN_MAX", "BNPP_MEM_BUDGET_GB", "BNPP_NO_O32", "BNPP_VE_CHAIN"};

// Run body(i) for i in [0, n) on up to `threads` host threads (0: hardware
// concurrency, capped at 16 — the per-GPU CPU share of the target machines).
void parallel_for(int64_t n, const std::function<void(int64_t)> &body, int threads = 0);
// parallel_for calls on this thread with threads = 0 use `n` threads while in scope (0: default)
extern thread_local int t_host_threads;
struct ScopedHostThreads {
    int saved;
    explicit ScopedHostThreads(int n) : saved(t_host_threads) { t_host_threads = n; }
    ~ScopedHostThreads() { t_host_threads = saved; }
};

// A table as one bucket input sees it: table id, evidence base offset, and the
// (variable, stride) pairs that remain after conditioning (domain.cpp:74-90).
struct View {
    int table = -1;
    int64_t base = 0;
    std::vector<int> vars;
    std::vector<int64_t> strides;
};

// Row-major strides, last variable fastest (domain.cpp:15-26).
// Sizes, strides and byte counts saturate at kSatMax (2^60): a min-fill order
// on a large grid plans tables of 2^100+ entries that no device could hold;
// they must compare as "too big" against any memory budget, not overflow.
constexpr int64_t kSatMax = (int64_t)1 << 60;
inline int64_t sat_mul(int64_t a, int64_t b) {
    int64_t r;
    return __builtin_mul_overflow(a, b, &r) || r > kSatMax ? kSatMax : r;
}
inline int64_t sat_add(int64_t a, int64_t b) {
    int64_t r;
    return __builtin_add_overflow(a, b, &r) || r > kSatMax ? kSatMax : r;
}
// entries a view can reach from its table's start (base + the last entry's
// offset + 1): what the 32-bit-offset generic kernels are chosen by
inline int64_t view_span(const View &v, const std::vector<int> &cards) {
    int64_t span = sat_add(v.base, 1);
    for (size_t j = 0; j < v.vars.size() && j < v.strides.size(); ++j)
        span = sat_add(span, sat_mul(cards[v.vars[j]] - 1, v.strides[j]));
    return span;
}
// generic-kernel variant of a bucket whose largest input view reaches
// max_in_bytes: the 32-bit-offset kernels only when every offset fits
inline int generic_variant(int n_in, int v1, int v2, int64_t max_in_bytes, bool no_o32 = false) {
    return variant_key(n_in, v1, v2) + (generic_o32(max_in_bytes) && !no_o32 ? kGenericO32 : 0);
}
std::vector<int64_t> natural_strides(const std::vector<int> &vars, const std::vector<int> &cards);
int64_t table_size(const std::vector<int> &vars, const std::vector<int> &cards);
View natural_view(int table, const std::vector<int> &vars, const std::vector<int> &cards);
// Factor::conditioning as a view (factor.cpp:214-242): evidence vars leave the
// scope and move into the base offset.  ev_val[v] < 0 means "no evidence on v".
View conditioned_view(int table, const std::vector<int> &vars, const std::vector<int> &cards,
                      const std::vector<int> &ev_val);

// Scope rules of the reference.
std::vector<int> union_scope(const std::vector<int> &a, const std::vector<int> &b);   // domain.cpp:32-41
std::vector<int> chain_scope(const std::vector<View> &in);                             // Factor(1.0) *= ...
std::vector<int> remove_var(const std::vector<int> &s, int v);                         // domain.cpp:54-59

struct BucketSpec {
    std::vector<View> in;
    int elim_var = -1;              // -1: pure product
    std::vector<int> out_vars;      // output layout (slowest first)
    int out_table = -1;
    int level = 0;
    // chain form (bnpp_device.h, ChainForm): in[0] is the message entering a
    // run of fused buckets, bucket j sums chain_x[j] and brings in chain_n[j];
    // in[1..] are the G tables of the buckets whose bit is set in chain_gmask
    std::vector<int> chain_x, chain_n;
    int chain_gmask = 0;
    // a dense backward split run may also form a delivery's belief (kChainBel):
    // its table here, the forward message it multiplies by the last entry of
    // `in` (after the G tables)
    int bel_table = -1;
    bool divide = false;            // Factor::divide: in[0] / in[1] (generic kernel, no sum)
    // build_schedule: a small bucket of a level with several kernel variants
    // runs in the level's one generic 1x1 launch (launch count, not bandwidth,
    // bounds such levels)
    bool simple = false;
    // message-sliced runs (plan_bucket_tree_chain with n_slices > 1): one step
    // of a message exchange between ranks, run by the executor, not a kernel
    // variant -- kXchgSync: all-gather of each rank's (largest true exponent,
    // exp2) of in[0] into out (2 (n_slices + 1) int64 words); kXchgPack: in[0]
    // scaled to the common exponent (read from in[1]) into out, blocks of the
    // destination ranks slowest (xchg_mode 0: in[0] already is, 1: they are
    // in[0]'s fastest variables -- a transpose); kXchgComm: collective from
    // in[0] to out (xchg_mode 0: all-to-all, 1: all-gather), out's blocks by
    // source rank slowest; kXchgUnpack: out = in[0] with the source blocks
    // moved from slowest to fastest (a transpose; xchg_mode 2: the blocks came
    // unpacked, and each is scaled to the common exponent read from in[1])
    int xchg = 0;
    int xchg_mode = 0;
    int xchg_blocks = 1;
    // stream lane (sliced two-front schedules: 0 forward messages, 1 backward
    // messages and deliveries): lanes run concurrently, ordered by the
    // cross-lane table dependencies only
    int lane = 0;
    // max-product (maxout.cuh): the bucket maximises over elim_var instead of
    // summing, and records the maximising value per output entry in arg_table
    // (one byte each; -1: a single-op call that passes the address itself).
    // Generic-shaped kernels only: never the stream, slab or chain forms, tiles
    // 1x1, 2x1 or 4x1; card(elim_var) <= kMaxOutCard
    bool max_out = false;
    int arg_table = -1;
    // the traceback that ends an MPE plan (plan_mpe): one row per max bucket,
    // ordered by depth in the elimination tree (roots first); `in` lists every
    // arg table, so that all of them live to this step; out_table holds the
    // assignment, int32 per model variable (decode_init: evidence values, 0
    // for a variable in no factor)
    struct DecodeRow {
        int arg_table, elim_var, depth;
        std::vector<int> vars;              // the bucket's separator, as its output is laid out
        std::vector<int64_t> strides;
    };
    bool decode = false;
    std::vector<DecodeRow> decode_rows;
    std::vector<int> decode_init;
    // the sampling step that ends a sampling plan (plan_sample, sample.cuh):
    // one row per non-evidence variable in REVERSE elimination order, each
    // with the views of the variable's eliminating bucket exactly as that
    // bucket read them (so p_v has the bits of the term the sum kernel added;
    // no views: a variable in no remaining factor, drawn uniformly); `in`
    // lists every table the rows read, so that all of them live to this step;
    // out_table holds x = uint8[n_vars][n_samples] and, behind it at the next
    // multiple of 8 bytes, the 8-byte counter of degenerate draws
    struct SampleRow {
        int var;
        std::vector<View> in;
    };
    bool sample = false;
    std::vector<SampleRow> sample_rows;
    std::vector<std::pair<int, int>> sample_ev;   // (evidence variable, value): rows of x filled as they are
    int64_t n_samples = 0;
    // a gather step of a batch plan (plan_batch, condbatch.cuh): in[0] is the
    // natural view of a source that mentions evidence variables, in[1] the
    // evidence table (int32[n_ev][rows], variable-major, uploaded per launch);
    // out_table, over out_vars = the source's other variables then the row
    // variable B, holds per row the entries the single call's conditioned view
    // of that source reaches.  cond_rows[j]: the row of the evidence table that
    // holds the values of in[0].vars[j] (-1: not an evidence variable)
    bool cond_batch = false;
    std::vector<int> cond_rows;
    // missing values: mask_rows[j] >= 0 names the row of the evidence table of a PARTIAL evidence variable
    // in[0].vars[j] whose mask this step carries (cond_rows[j] is then -1 and the variable stays in out_vars);
    // empty, or all -1: an unmasked step
    std::vector<int> mask_rows;
    // soft evidence: soft_rows[j] >= 0 names the first row of the likelihood table (in[2]) of a SOFT variable
    // in[0].vars[j] whose weights this step carries (the variable stays in out_vars); empty, or all -1: none
    std::vector<int> soft_rows;
    // an accumulate step of a counts plan (plan_counts, counts.cuh): in[0] is
    // the belief of one factor over (its non-evidence variables, B) -- B the
    // fastest dim, absent when no evidence reaches the belief -- and the other
    // inputs name the raw tables below, so that all of them live to this step.
    // counts_scope is the factor's own scope, counts_rows[j] the row of the
    // evidence table that holds counts_scope[j] (-1: not an evidence variable),
    // counts_acc_off the factor's first entry in the accumulator buffer.
    // out_table is a one-entry placeholder: the step writes the accumulators,
    // which live outside the arena
    // the traceback that ends a batched MPE plan (plan_mpe_batch, maxbatch.cuh):
    // decode_rows in REVERSE elimination order (a bucket after the buckets that
    // maximise its separator), each row's vars the bucket's output scope -- the
    // row variable B last where the arg table carries it; `in` lists every arg
    // table and the evidence table, so that all of them live to this step;
    // out_table holds x = uint8[n_vars][decode_batch_rows], variable-major,
    // of which the step writes the rows of the maximised variables only
    bool decode_batch = false;
    int64_t decode_batch_rows = 0;
    // the draw step that ends a batched sampling plan (plan_sample_batch,
    // sample.cuh): sample_rows as in a sampling step, over views that carry the
    // row variable B (the plan's last variable) exactly where evidence reaches
    // them; sample_batch_rows = R rows per launch, sample_batch_k = K draws per
    // row; `in` lists every table the rows read and the evidence table;
    // out_table holds x = uint8[n_vars][K][R] (of which the step writes the
    // rows of the sampled variables only) and, behind it at the next multiple
    // of 8 bytes, int64[R] degenerate draws per row
    bool sample_batch = false;
    int64_t sample_batch_rows = 0, sample_batch_k = 0;
    bool counts = false;
    int counts_factor = -1;
    std::vector<int> counts_scope, counts_rows;
    int64_t counts_acc_off = 0;
    int counts_ev_table = -1, counts_w_table = -1, counts_valid_table = -1, counts_scratch_table = -1;
    bool counts_valid_b = false;        // the validity table is over (B) (else one entry)
    // the emit step that ends a batched-marginals plan (plan_marginals_batch,
    // margrows.cuh): one column block per target, in the caller's order -- a
    // belief (the target's table over (target, B), B the fastest dim, or over
    // (target) alone where no evidence reaches it), an evidence block (one-hot
    // of the row's value, from row ev_row of the evidence table) or a free
    // block (a variable in no remaining factor: 1 / card).  `in` lists every
    // target table and the evidence table, so that all of them live to this
    // step; out_table holds out = double[marg_n_rows][W], row-major, W the
    // sum of the blocks' cards
    struct MargCol {
        int var = -1, card = 1;
        int table = -1;                 // the belief's table (-1: evidence or free)
        bool has_b = false;             // ... carries B
        int ev_row = -1;                // the evidence table's row (-1: no evidence variable)
    };
    bool marg_rows = false;
    std::vector<MargCol> marg_cols;
    int marg_ev_table = -1;
    int64_t marg_n_rows = 0;
};
enum XchgKind { kXchgNone = 0, kXchgSync = 1, kXchgPack = 2, kXchgComm = 3, kXchgUnpack = 4 };
// schedule group variant of an exchange step: kXchgKeyBase + kind * 16 + mode
// (above every kernel variant key, bnpp_device.h)
constexpr int kXchgKeyBase = 1 << 24;
// ... of the MPE traceback (BucketSpec::decode): the executor's too, above the exchange kinds
constexpr int kMpeDecodeKey = kXchgKeyBase + 4096;
// ... of the sampling step (BucketSpec::sample): the executor's as well
constexpr int kSampleKey = kXchgKeyBase + 8192;
// ... of a gather step of a batch plan (BucketSpec::cond_batch): the executor's, one group per step
constexpr int kCondBatchKey = kXchgKeyBase + 12288;
// ... of an accumulate step of a counts plan (BucketSpec::counts): the executor's, one group per step
constexpr int kCountsKey = kXchgKeyBase + 16384;
// ... of the traceback of a batched MPE plan (BucketSpec::decode_batch): the executor's
constexpr int kMpeDecodeBatchKey = kXchgKeyBase + 20480;
constexpr int kDecodeBatchPoolHead = 4;   // words before the rows of a batched traceback's pool
// ... of the draw step of a batched sampling plan (BucketSpec::sample_batch): the executor's
constexpr int kSampleBatchKey = kXchgKeyBase + 24576;
constexpr int kSampleBatchPoolHead = 4;   // words before the rows of a batched draw step's pool
// ... of the emit step of a batched-marginals plan (BucketSpec::marg_rows): the executor's
constexpr int kMargRowsKey = kXchgKeyBase + 28672;
// ... of a masked gather step (BucketSpec::cond_batch with mask_rows: partial evidence variables): the executor's
constexpr int kCondBatchMaskKey = kXchgKeyBase + 32768;
// ... of a weighted gather step (BucketSpec::cond_batch with soft_rows: soft variables, masks beside them): the executor's
constexpr int kCondBatchSoftKey = kXchgKeyBase + 36864;
// the three forms of a gather step (condbatch.cuh), and the form a launch-group key stands for (-1: no gather key)
enum CondForm { kCondPlain = 0, kCondMasked = 1, kCondWeighted = 2 };
constexpr int cond_form_of_key(int key) {
    return key == kCondBatchKey ? kCondPlain : key == kCondBatchMaskKey ? kCondMasked : key == kCondBatchSoftKey ? kCondWeighted : -1;
}
constexpr int kMargRowsPoolHead = 4;      // words before the column blocks of an emit step's pool
constexpr int kMargRowsColWords = 5;      // words per column block
constexpr int kCountsMaxDims = 32;  // evidence variables, and other variables, in one factor scope of an accumulate step
constexpr int kCountsPoolHead = 12; // words before the per-variable rows of an accumulate step's pool
constexpr int kCondMaxRest = 8;     // rest dims of a gather step after merging adjacent ones
constexpr int kCondMaxEv = 32;      // evidence variables in one scope of a single-op gather
// the most pool words of a single-op gather of a form: the head, the evidence and rest words, then a count and
// kCondMaxRest pairs for the masks and again for the weights
static_assert(kCondPlain == 0 && kCondMasked == 1 && kCondWeighted == 2, "a form's value counts its blocks after the rest words");
constexpr int cond_single_pool_words(int form) { return 4 + 3 * kCondMaxEv + 2 * kCondMaxRest + form * (1 + 2 * kCondMaxRest); }
// byte offset of the degenerate-draw counter in a sampling step's out_table
inline int64_t sample_counter_offset(int64_t n_vars, int64_t n_samples) { return (n_vars * n_samples + 7) / 8 * 8; }

// Compile one bucket into a descriptor + dims-pool rows.  max_vec: 4 (fp32) / 2 (fp64).
// Returns false (with msg) on an invalid shape.
bool build_desc(const BucketSpec &b, const std::vector<int> &cards, int max_vec, BucketDesc &d,
                std::vector<int64_t> &pool, std::string *msg, bool slab_outer = true);

// Fused chain runs: is the chain kernel with this key (bnpp_device.h,
// chain_key) instantiated for this element size (k_chain_f32/f64.hip)?
bool chain_supported_f32(int key);
bool chain_supported_f64(int key);
inline bool chain_supported(int elem_bytes, int key) {
    return elem_bytes == 4 ? chain_supported_f32(key) : chain_supported_f64(key);
}

struct MsgTable {
    std::vector<int> vars;
    int64_t size = 1;
};

// Symbolic VE plan (BN::variable_elimination, model.cpp:348-446).
struct VEPlan {
    int n_src = 0;                      // tables [0, n_src) are the (conditioned) sources
    std::vector<MsgTable> msgs;         // table id = n_src + index
    std::vector<BucketSpec> buckets;    // execution order (non-decreasing level)
    int n_levels = 0;
    int result_table = -1;              // -1: result is the constant 1 (no factors)
    std::vector<int> result_vars;
    // multi-result plans (bucket-tree marginals): one table per target, -1 =
    // no table (evidence / variable in no factor); replaces result_table
    std::vector<int> results;
    std::vector<std::vector<int>> results_vars;
    std::vector<char> results_owned;    // per result: computed by this part (empty: all)
    // cards of the model followed by virtual (composite) variables the plan
    // sums in one pass; empty: the model's cards
    std::vector<int> cards_ext;
    int64_t max_table = 0;              // largest message entries
    double entries = 0;                 // sum over buckets of prod(card) over the union scope
    double elems_moved = 0;             // sum over buckets of (|inputs| + |output|): algorithmic traffic
    int width = 0;                      // largest bucket output width
    // message slicing: ranks that share the messages (1: none), this plan's
    // rank, and per result the rank bit that indexes it (-1: the result is a
    // table over its target; else a scalar, the target being a slice
    // variable whose value is that bit of the rank)
    int n_slices = 1, slice_rank = 0;
    std::vector<int> results_slice_bit;
    int64_t arg_bytes = 0;              // plan_mpe: bytes of all arg tables (resident to the traceback)
    // plan_mpe_batch: max buckets; arg tables that carry B and their entries per row; ... that do not, and
    // their entries (arg_bytes = arg_b_entries * rows + arg_nob_entries, the tables' bytes before alignment)
    int n_max_buckets = 0, n_arg_b = 0, n_arg_nob = 0;
    int64_t arg_b_entries = 0, arg_nob_entries = 0;
    int64_t sample_bytes = 0;           // plan_sample: bytes of the sample state x (n_vars * n_samples)
    // plan_sample_batch: sample_bytes = n_vars * rows * K; draw rows with an input that carries B, and without
    int n_draw_b = 0, n_draw_nob = 0;
    int batch_ev_table = -1;            // plan_batch: the evidence table (-1: no gather step)
    std::vector<int> batch_mask_factor; // per evidence variable: the factor whose gather step carries its mask (-1: none)
    int batch_lam_table = -1;           // soft evidence: the likelihood table T[Ws][rows] (-1: no soft variable)
    std::vector<int> batch_lam_factor;  // per soft variable: the factor whose gather step carries its weights
    // plan_counts: the per-launch weights (double[rows]) and the first
    // accumulate step's scratch (3 x 8 bytes per row; one per step), raw tables; per factor the
    // variables of its belief table (B = cards.size() last when carried);
    // the last level of the forward pass (plan_batch's own buckets)
    int counts_w_table = -1, counts_scratch_table = -1;
    std::vector<std::vector<int>> counts_belief_vars;
    int counts_fwd_levels = 0;
    // plan_marginals_batch: belief, evidence and free column blocks of the emit step, of the beliefs those
    // whose table carries B, W = the columns of a row, and the bytes of the output table (rows * W * 8)
    int n_marg_belief = 0, n_marg_belief_b = 0, n_marg_ev = 0, n_marg_free = 0;
    int64_t marg_width = 0, marg_out_bytes = 0;
    int n_xchg = 0;                     // message exchanges (all-to-all / all-gather)
    double xchg_elems = 0;              // entries this rank sends to other ranks
};

// canonical: lay messages out with variables sorted by elimination rank
// (earlier-eliminated slower) instead of the reference's chain order; values
// are identical, only the storage permutation differs.  Buckets with more than
// kMaxIn inputs are split into materialised pure-product prefixes exactly like
// the reference's left-to-right chain.
VEPlan plan_ve(const std::vector<int> &cards, const std::vector<View> &sources, const std::vector<int> &order,
               bool canonical, int chain_eb = 0);

// Most probable explanation: plan_ve(canonical) over `order` (every
// non-evidence variable) with each eliminating bucket maximising (max_out) and
// recording its argmax in a table of its own, then one traceback step
// (BucketSpec::decode) that reads every arg table.  results = {the maximum (a
// scalar), the assignment (int32 per variable, sized in whole elements of
// elem_bytes)}.  Pure-product prefixes of buckets with more than kMaxIn inputs
// stay ordinary products.  ev_val: per variable, -1 = no evidence.  Returns
// false (msg) when a maximised variable has more than kMaxOutCard values.
bool plan_mpe(const std::vector<int> &cards, const std::vector<View> &sources, const std::vector<int> &order,
              const std::vector<int> &ev_val, int elem_bytes, VEPlan &out, std::string *msg);

// Posterior sampling: plan_ve(canonical) over `order` (every non-evidence
// variable) with no fused chain runs -- every eliminating bucket's inputs must
// exist as tables -- then one sampling step (BucketSpec::sample) that draws
// each variable from its bucket's inputs in reverse elimination order, for
// n_samples samples.  The step names every table its rows read as an input, so
// the lifetime analysis keeps all messages to the end (no checkpointing).
// results = {the partition function (a scalar)}; x is the step's out_table.
// ev_val: per variable, -1 = no evidence.  Returns false (msg) when a sampled
// variable has more than kMaxOutCard values (x holds one byte per value).
bool plan_sample(const std::vector<int> &cards, const std::vector<View> &sources, const std::vector<int> &order,
                 const std::vector<int> &ev_val, int elem_bytes, int64_t n_samples, VEPlan &out, std::string *msg);

// Missing values (all batched planners): partial[i] != 0 marks ev_vars[i] as
// PARTIAL -- it may be missing (-1) in any row.  A partial variable is not
// conditioned away: it is an ordinary variable of `order`, and exactly one
// gather step that holds it carries its mask (BucketSpec::mask_rows), chosen
// by batch_mask_factors.  Empty `partial`: none.
//
// Soft evidence (all batched planners): `soft` lists the SOFT variables -- row b
// carries a likelihood per value of each.  A soft variable is no evidence
// variable: it is an ordinary variable of `order`, and exactly one gather step
// that holds it multiplies its weights in (BucketSpec::soft_rows), chosen by
// batch_lam_factors.  The weights of a launch are a raw table T[Ws][rows]
// (VEPlan::batch_lam_table), variable-major in the order of `soft`, Ws the sum
// of the soft cards.  Empty `soft`: none, and nothing of the plan changes.
//
// Batched evidence: one plan for `rows` evidence assignments over the evidence
// variables ev_vars.  `sources` are the NATURAL views of the model's factors.
// A virtual variable B (id cards.size(), card = rows) stands for "which row":
// every source that mentions an evidence variable gets one gather step
// (BucketSpec::cond_batch, level 0) whose table over (the source's other
// variables, B) takes exactly the place the conditioned view of that source has
// in the single call's plan; then plan_ve(canonical)'s elimination over `order`
// with cards_ext = cards + {rows}.  B is never eliminated, so it is the fastest
// dimension of every message that evidence reaches; messages that no evidence
// reaches carry no B and are computed once.  No fused chain runs (as the
// per-target plans of bnpp_marginals): a gathered table is a message, not a
// source, to the chain matcher, and the unfused buckets perform the same
// arithmetic in the same order.  target >= 0: kept (never in `order`), the
// result is a table over (target, B); else over (B); a result that evidence
// does not reach lacks B.  The evidence table is the last raw table of the
// plan (VEPlan::batch_ev_table).  Returns false (msg) when a source has more
// than kCondMaxRest runs of non-evidence variables between evidence variables.
bool plan_batch(const std::vector<int> &cards, const std::vector<View> &sources, const std::vector<int> &order,
                const std::vector<int> &ev_vars, int64_t rows, int target, int elem_bytes, VEPlan &out,
                std::string *msg, const std::vector<char> &partial = std::vector<char>(),
                const std::vector<int> &soft = std::vector<int>());

// The factor that carries the mask of each evidence variable (-1: hard, or in no factor): 1. a factor that
// holds a hard evidence variable (it has a gather step anyway); 2. among those, else among all factors that
// hold it, the fewest entries after conditioning on the hard variables; 3. the lowest factor index
std::vector<int> batch_mask_factors(const std::vector<int> &cards, const std::vector<View> &sources,
                                    const std::vector<int> &ev_vars, const std::vector<char> &partial);
// The factor that carries the weights of each soft variable (-1: in no factor), by the same rule
std::vector<int> batch_lam_factors(const std::vector<int> &cards, const std::vector<View> &sources,
                                   const std::vector<int> &ev_vars, const std::vector<char> &partial,
                                   const std::vector<int> &soft);

// Batched MPE: plan_batch's gather steps (level 0), evidence table and cards_ext
// = cards + {rows}, then plan_mpe's elimination over them: every eliminating
// bucket maximises (max_out) and records its argmax in a table over its output
// scope -- B the fastest dimension exactly where the message has it; a bucket
// that no evidence reaches has neither.  No fused chain runs; pure-product
// prefixes stay products.  Then one traceback step (BucketSpec::decode_batch)
// over R rows at once.  results = {the maxima, a table over (B) or a scalar
// when no evidence reaches it; x = uint8[n_vars][rows]}.  `order` covers every
// non-evidence variable.  Returns false (msg) as plan_batch and plan_mpe do.
bool plan_mpe_batch(const std::vector<int> &cards, const std::vector<View> &sources, const std::vector<int> &order,
                    const std::vector<int> &ev_vars, int64_t rows, int elem_bytes, VEPlan &out, std::string *msg, const std::vector<char> &partial = std::vector<char>(),
                 const std::vector<int> &soft = std::vector<int>());

// Batched sampling: plan_batch's gather steps (level 0), evidence table and
// cards_ext = cards + {rows}, then plan_sample's loop over the placed views: no
// fused chain runs, one SampleRow per variable of `order` in reverse
// elimination order with the eliminating bucket's own views as emitted (B among
// them exactly where evidence reaches the view), an input-less row for a
// variable in no remaining factor.  The result is plan_batch's, a table over
// (B) or a scalar.  One draw step (BucketSpec::sample_batch) of K = n_per_row
// draws for each of `rows` rows ends the plan; it names every table its rows
// read.  results = {the partition function per row; x and the per-row
// degenerate counts}.  `order` covers every non-evidence variable.  Returns
// false (msg) as plan_batch and plan_sample do.
bool plan_sample_batch(const std::vector<int> &cards, const std::vector<View> &sources, const std::vector<int> &order,
                       const std::vector<int> &ev_vars, int64_t rows, int64_t n_per_row, int elem_bytes, VEPlan &out,
                       std::string *msg, const std::vector<char> &partial = std::vector<char>(),
                 const std::vector<int> &soft = std::vector<int>());

// Expected sufficient statistics: a batched bucket tree.  plan_batch's gather
// steps (level 0) and forward pass -- the same buckets in the same order, the
// final product of the root messages included: the plan's result is plan_batch's
// table over (B) -- then plan_bucket_tree's backward pass over cards_ext =
// cards + {rows}, at levels after the forward pass.  B is never in `order`
// (rank -1) and is never summed: it is kept by every reduction one of whose
// inputs carries it, so a pi gains B even where its separator has none, and it
// enters no composite variable.  For every factor the belief of its bucket is
// summed down to (scope minus evidence, B) and one BucketSpec::counts step
// folds it into the factor's accumulator; the steps share the
// plan's last level and have scratch of their own, so they run in one launch.  A factor with no
// variable left is its own belief (the gathered table over (B), or the source).
// No fused chain runs, no checkpointing: every forward message stays resident.
// Returns false (msg) as plan_batch does, when a factor scope holds more than
// kCountsMaxDims evidence (or other) variables, or when `order` leaves out a
// non-evidence variable of a factor.
bool plan_counts(const std::vector<int> &cards, const std::vector<View> &sources, const std::vector<int> &order,
                 const std::vector<int> &ev_vars, int64_t rows, int elem_bytes, VEPlan &out, std::string *msg, const std::vector<char> &partial = std::vector<char>(),
                 const std::vector<int> &soft = std::vector<int>());

// Batched marginals: plan_counts's batched bucket tree -- the same gather
// steps, forward pass (plan_batch's, so the first result is its table over (B))
// and backward pass with B kept wherever an input carries it -- then, for every
// target that is no evidence variable and sits in a factor, the smallest of its
// bucket's belief and the separator beliefs lam_c * pi_c of the bucket's
// children (plan_bucket_tree's choice, by sizes without B so that it does not
// depend on `rows`), times what never enters the target's tree (a factor over
// evidence variables only, the root message of another component: a row one of
// them makes impossible then has an all-zero column), summed down to
// (target, B) -- (target) alone where no evidence reaches it -- and one emit step
// (BucketSpec::marg_rows) at a last level of its own that normalises every
// target's table row by row into out = double[rows][W].  results =
// {plan_batch's table; out}.  No fused chain runs, no checkpointing.  Returns
// false (msg) as plan_counts does, or on a target out of range or listed twice.
bool plan_marginals_batch(const std::vector<int> &cards, const std::vector<View> &sources, const std::vector<int> &order,
                          const std::vector<int> &ev_vars, int64_t rows, const std::vector<int> &targets, int elem_bytes,
                          VEPlan &out, std::string *msg, const std::vector<char> &partial = std::vector<char>(),
                 const std::vector<int> &soft = std::vector<int>());

// All marginals of `targets` from one two-pass bucket tree over `order`
// (Shafer-Shenoy on the VE bucket tree; replaces the N independent VEs of
// BN::marginals, model.cpp:326-334).  Forward messages are plan_ve's; each
// bucket then sends every child the product of its factors, its own incoming
// message and its other children's messages, summed down to the child's
// separator; each target's marginal (unnormalised) is the smallest belief that
// contains it summed down to the target.  results[i] -> targets[i].
// part / n_parts: marginals of targets i with i % n_parts == part only (the
// forward and backward passes are computed in full by every part).
VEPlan plan_bucket_tree(const std::vector<int> &cards, const std::vector<View> &sources,
                        const std::vector<int> &order, const std::vector<int> &targets, int part = 0,
                        int n_parts = 1);

// The same marginals in bounded memory when the bucket tree is a chain (a
// column-sweep order on a grid): forward messages are recomputed from `slots`
// checkpoints by binomial checkpointing (revolve), buckets run in program order
// (one level each) so the arena holds about slots + 5 messages.  Returns false
// (msg) when the tree is not a chain.  part / n_parts: this part owns the
// marginals of one contiguous segment of the chain; it streams the forward
// messages up to the segment, runs the backward messages (which need no
// forward message) down to it, and checkpoints only inside it.  chain_eb > 0:
// runs of consecutive buckets are fused into chain kernels for that element
// size (bnpp_device.h, ChainForm).
// n_slices = 2^b > 1: message slicing over n_slices ranks (this plan is rank
// slice_rank's).  The chain is cut into windows in which b binary variables
// stay in every separator; inside a window each rank holds the messages (and
// computes the buckets) conditioned on those variables = the bits of its
// rank, 1/n_slices of the work and memory; between windows a message is
// re-sliced by one all-to-all (kXchg* steps), at the chain's ends
// all-gathered or conditioned.  Every rank computes a partial (unnormalised)
// marginal of every target: the marginals are the sum over ranks.  lanes:
// the two-front schedule (forward and backward messages on two concurrent
// lanes, no recomputation; `slots` unused), else binomial checkpointing.
// elem_bytes: the dtype's (the kept-set size of a delivery depends on it).
bool plan_bucket_tree_chain(const std::vector<int> &cards, const std::vector<View> &sources,
                            const std::vector<int> &order, const std::vector<int> &targets, int slots,
                            int part, int n_parts, VEPlan &out, std::string *msg, int chain_eb = 0,
                            int n_slices = 1, int slice_rank = 0, bool lanes = false, int elem_bytes = 4);

// Flattened, level-ordered launch schedule over one or more plans sharing the
// same sources.  Tables: [0, n_src) sources, then every plan's messages.
// vector allocator that default-initialises (no zero fill before the
// parallel copy that fills a schedule's descriptor and pool arrays)
template <typename T>
struct DefaultInit : std::allocator<T> {
    template <typename U>
    struct rebind {
        using other = DefaultInit<U>;
    };
    DefaultInit() = default;
    template <typename U>
    DefaultInit(const DefaultInit<U> &) noexcept {}
    template <typename U>
    void construct(U *p) noexcept {
        ::new ((void *)p) U;
    }
    template <typename U, typename... A>
    void construct(U *p, A &&...a) {
        ::new ((void *)p) U(std::forward<A>(a)...);
    }
};

struct Schedule {
    int n_src = 0;
    int n_tables = 0;
    std::vector<int64_t> table_size;        // entries, per table (sources included)
    std::vector<int64_t> table_offset;      // bytes into the arena (messages only; -1 for sources)
    std::vector<BucketDesc, DefaultInit<BucketDesc>> descs;   // grouped by level, vblk_begin relative to the level
    std::vector<int64_t, DefaultInit<int64_t>> pool;
    struct Group {                          // one launch: buckets of one level and one kernel variant
        int level, variant, begin, end;
        int64_t vblocks;
        int small_elems;                    // stream kernels: LDS elements for small inputs
        int lane;                           // BucketSpec::lane (all buckets of a group share it)
    };
    std::vector<Group> groups;
    int n_levels = 0;
    std::vector<int> plan_result_table;     // per plan (-1: constant 1)
    std::vector<std::vector<int>> plan_result_vars;
    std::vector<char> plan_result_owned;     // per result: 0 = another part computes it
    std::vector<int> plan_result_slice_bit;  // per result: VEPlan::results_slice_bit (-1: none)
    int64_t arena_bytes = 0;
    double entries = 0;
    double elems_moved = 0;
    int width = 0;
    int n_lanes = 1;                        // concurrent stream lanes (Group::lane)
};

// Peak bytes of live messages when the plan runs level by level (arena estimate).
int64_t plan_peak_bytes(const VEPlan &p, int elem_bytes);
// Bytes of the arena build_schedule allocates for this plan alone (the same
// best-fit allocator, so fragmentation included).
int64_t plan_arena_bytes(const VEPlan &p, int elem_bytes);

// arena_cap: the most device memory the schedule's arena may take; several
// plans get arenas of their own (placed in parallel) when their sum fits it,
// else one shared arena
bool build_schedule(const std::vector<const VEPlan *> &plans, const std::vector<int> &cards,
                    const std::vector<int64_t> &src_sizes, int elem_bytes, int max_vec, Schedule &s,
                    std::string *msg, int64_t arena_cap = INT64_MAX);

}  // namespace bnpp
