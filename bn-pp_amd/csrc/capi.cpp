// extern "C" boundary (include/bnpp.h).  No exception crosses it: every entry
// point catches, records bnpp_last_error() and returns a status code.
#include "../../include/bnpp.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <fstream>
#include <string>
#include <utility>
#include <thread>
#include <unistd.h>
#include <vector>

#include "model_io.hpp"
#include "order.hpp"
#include "plan.hpp"
#include "runtime.hpp"

using namespace bnpp;

constexpr int kTimingPhases = 9;

struct bnpp_ctx {
    Context c;
    std::mutex cache_mu;            // one one-shot call at a time uses c.arena_cache
    // uploaded sources of recent models, per dtype (a model is read-only after
    // creation, so its pre-scaled tables stay valid): a repeated call skips
    // the host pre-scaling and the copy (1.5 of Mildew's 2.2-ms PR).  Keyed on
    // the model's uid, never reused; most recent last
    struct Src {
        uint64_t uid;
        int dtype;
        std::shared_ptr<DeviceSources> s;
    };
    std::mutex src_mu;
    std::vector<Src> srcs;
    // the last one-shot partition / marginals job (plan, schedule, device
    // program on the cached arena), relaunched as is by an identical call
    // (same model, evidence, order, targets, dtype, part, memory budget and
    // BNPP_* environment): a serving caller's repeated query skips ordering
    // and planning.  Guarded by cache_mu, like the arena it runs in
    bnpp_job *job_cached = nullptr;
    uint64_t job_key = 0;
    int64_t job_budget = 0;             // the memory budget the cached job was planned under
    // bnpp_mstep_dv: the per-factor words of the last model it refitted, on the device
    std::mutex mstep_mu;
    void *mstep_words = nullptr;
    size_t mstep_cap = 0;
    uint64_t mstep_uid = 0;
    int64_t mstep_cfg = 0;              // its parent configurations in all
    hipStream_t mstep_stream = nullptr; // the stream of the last M step (it may still read the words)
    bool mstep_launched = false;
};
// live contexts: bnpp_model_free releases what they cache for the model
std::mutex g_ctxs_mu;
std::vector<bnpp_ctx *> g_ctxs;
// live table sets: bnpp_ctx_destroy releases those of its context, which then only remain to be freed
struct bnpp_tables;
std::mutex g_tables_mu;
std::vector<bnpp_tables *> g_tables;

struct bnpp_model {
    ModelData d;
    uint64_t uid = next_uid();
    static uint64_t next_uid() {
        static std::atomic<uint64_t> n{1};
        return n++;
    }
};
struct bnpp_job {
    bnpp_ctx *ctx = nullptr;
    int kind = 0;
    uint64_t model_uid = 0;            // the model it was planned for (bnpp_model_free evicts a cached job of it)
    std::shared_ptr<DeviceSources> src;
    Program pg;
    std::vector<int> targets;
    std::vector<int> ev_val;          // per variable, -1 = no evidence
    std::vector<int> cards;
    int n_slices = 1, slice_rank = 0;  // message-sliced bucket tree (bnpp_marginals_tree_sliced)
    double stats[10] = {0};            // bnpp_job_stats [0..8), then n_xchg, exchange bytes sent
    int64_t batch_rows = 0;            // batched evidence (kind 6): rows per launch
    uint64_t tables_uid = 0;           // the table set it reads instead of the model's own (bnpp_tables_free evicts it)
};
// The tables of one model on one context in one dtype, rewritten in place on the device (bnpp_tables_set_dv).
// One block holds the factors' device TableMeta, the shift and the tops, stage_tables' descriptor words and
// its status word; src is the layout upload_sources makes, whose buffer never moves
struct bnpp_tables {
    bnpp_ctx *ctx = nullptr;
    uint64_t uid = bnpp_model::next_uid(), model_uid = 0;
    int dtype = BNPP_F64;
    bool log_form = false;
    std::shared_ptr<DeviceSources> src;
    std::vector<int64_t> sizes;                         // per factor, and the flat array's length
    int64_t total = 0;
    void *block = nullptr;
    size_t block_cap = 0;
    TableMeta *d_meta = nullptr;
    double *d_shift = nullptr;                          // [1 + n_factors]: the shift, the factors' tops
    int64_t *d_words = nullptr, *d_status = nullptr;
};

namespace {

thread_local std::string g_err;
// phase split of this thread's last partition / marginals call (bnpp_last_timing)
thread_local double g_timing[kTimingPhases] = {0};

int set_err(int status, const std::string &msg) {
    g_err = msg;
    return status;
}
int from_ctx(bnpp_ctx *ctx, int rc) {
    if (rc == 0) return BNPP_OK;
    g_err = ctx->c.last_error;
    return rc == -3 ? BNPP_ERR_OOM : rc == -1 ? BNPP_ERR_INVALID : BNPP_ERR_HIP;
}
hipStream_t pick_stream(bnpp_ctx *ctx, void *stream) {
    return stream ? static_cast<hipStream_t>(stream) : ctx->c.stream;
}
double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

#define BNPP_GUARD_BEGIN try {
#define BNPP_GUARD_END                                                       \
    }                                                                        \
    catch (const std::bad_alloc &) {                                         \
        return set_err(BNPP_ERR_OOM, "host out of memory");                  \
    }                                                                        \
    catch (const std::exception &e) {                                        \
        return set_err(BNPP_ERR_INVALID, e.what());                          \
    }                                                                        \
    catch (...) {                                                            \
        return set_err(BNPP_ERR_INVALID, "unknown error");                   \
    }

// every id in [0, n_cards) with a positive cardinality, no repeats
bool valid_scope(int ndims, const int *vars, const int *cards, int n_cards) {
    if (ndims < 0 || (ndims > 0 && !vars)) return false;
    for (int i = 0; i < ndims; ++i) {
        if (vars[i] < 0 || vars[i] >= n_cards || cards[vars[i]] < 1) return false;
        for (int j = 0; j < i; ++j)
            if (vars[j] == vars[i]) return false;
    }
    return true;
}

int max_vec_for(int dtype) { return dtype == BNPP_F32 ? 4 : 2; }

// Plan one single-op call: the descriptor, its dims pool and the entries each
// view can reach, all a launch needs but the table addresses.  run_single
// launches what this fills and bnpp_plan_single reports it.
int plan_single(int dtype, const std::vector<int> &cards, const BucketSpec &b, SingleArgs &a) {
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32");
    std::memset(&a, 0, sizeof a);
    std::vector<int64_t> pool;
    std::string msg;
    if (!build_desc(b, cards, max_vec_for(dtype), a.d, pool, &msg, false)) return set_err(BNPP_ERR_INVALID, msg);
    if (pool.size() > (size_t)kMaxPool)
        return set_err(BNPP_ERR_UNSUPPORTED, "too many non-mergeable output dims for a single-op call");
    std::copy(pool.begin(), pool.end(), a.pool);
    a.d.dim_off = 0;
    // entries the view can reach (the launcher picks 32-bit offsets by it)
    for (size_t i = 0; i < b.in.size(); ++i) a.meta[i].size = view_span(b.in[i], cards);
    // BNPP_NO_O32=1 (tests): claim a span that rules out the 32-bit-offset kernels
    if (const char *no32 = std::getenv("BNPP_NO_O32"); no32 && *no32 == '1')
        for (size_t i = 0; i < b.in.size(); ++i) a.meta[i].size = (int64_t)1 << 40;
    return BNPP_OK;
}

// Launch one bucket with the descriptor in the kernel-argument segment.
int run_single(bnpp_ctx *ctx, void *stream, int dtype, const std::vector<int> &cards, const BucketSpec &b,
               const std::vector<const void *> &in_ptrs, void *out) {
    SingleArgs a;
    if (int rc = plan_single(dtype, cards, b, a)) return rc;
    for (size_t i = 0; i < in_ptrs.size(); ++i) a.meta[i].ptr = const_cast<void *>(in_ptrs[i]);
    a.meta[in_ptrs.size()].ptr = out;
    if (a.d.big >= 0) {
        const int eb = dtype == BNPP_F32 ? 4 : 8;
        a.big_ptr = static_cast<const unsigned char *>(in_ptrs[a.d.big]) + a.d.in_base[a.d.big] * eb;
        a.big_es = a.d.elim_stride[a.d.big];
    }
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_single(dtype == BNPP_F32, a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
}

// The bucket of a single-op max call (bnpp_bucket_max, bnpp_plan_max_single):
// validated like bnpp_bucket_eliminate's, with elim_var required and its card
// checked here, on the host, before anything is planned or launched.
int max_single_spec(int n_cards, const int *cards, int n_in, const int *in_ndims, const int *const *in_vars,
                    int elim_var, int out_ndims, const int *out_vars, BucketSpec &b, std::vector<int> &cv) {
    if (!cards || n_in < 1 || !in_ndims || !in_vars) return set_err(BNPP_ERR_INVALID, "null argument");
    if (n_in > kMaxIn) return set_err(BNPP_ERR_UNSUPPORTED, "at most 8 inputs per fused call");
    if (n_cards < 0 || elim_var < 0 || elim_var >= n_cards || cards[elim_var] < 1 || (out_ndims > 0 && !out_vars))
        return set_err(BNPP_ERR_INVALID, "variable id outside cards[0, n_cards)");
    for (int i = 0; i < n_in; ++i)
        if (!valid_scope(in_ndims[i], in_vars[i], cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad input scope");
    if (!valid_scope(out_ndims, out_vars, cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad output scope");
    cv.assign(cards, cards + n_cards);
    b = BucketSpec{};
    bool has_elim = false;
    for (int i = 0; i < n_in; ++i) {
        std::vector<int> s(in_vars[i], in_vars[i] + in_ndims[i]);
        for (int x : s) has_elim = has_elim || x == elim_var;
        b.in.push_back(natural_view(i, s, cv));
    }
    if (has_elim && cv[elim_var] > kMaxOutCard)
        return set_err(BNPP_ERR_UNSUPPORTED, "max bucket: the maximised variable has more than 256 values (the arg is one byte)");
    b.elim_var = elim_var;
    std::vector<int> u = remove_var(chain_scope(b.in), elim_var);
    std::vector<int> ov(out_vars, out_vars + out_ndims), us = u, os = ov;
    std::sort(us.begin(), us.end());
    std::sort(os.begin(), os.end());
    if (us != os) return set_err(BNPP_ERR_INVALID, "output scope must be the union of the inputs minus elim_var");
    b.out_vars = ov;
    b.out_table = n_in;
    b.max_out = true;
    return BNPP_OK;
}

// Factor::_partition of a single-op call (seqsum.hip), enqueued after the op
// on the same stream: the terms of the inputs' chain product (or in[0] /
// in[1]) over `dims` -- the reference's output scope order, last fastest --
// with elim_var's values inner, added one at a time in that order.
// checked before the op is launched, so an unsupported out_sum never leaves
// an op that ran behind an error status
int seq_sum_supported(const double *out_sum, size_t n_dims, size_t n_in) {
    if (out_sum && (n_dims > (size_t)kSeqMaxDims || n_in > (size_t)kMaxIn))
        return set_err(BNPP_ERR_UNSUPPORTED, "out_sum: at most 32 output variables");
    return BNPP_OK;
}

int run_seq_sum(bnpp_ctx *ctx, void *stream, int dtype, const std::vector<int> &cards, const std::vector<View> &in,
                const std::vector<const void *> &ptrs, const std::vector<int> &dims, int elim_var, bool divide,
                double *out_sum) {
    if (!out_sum) return BNPP_OK;
    if (int rc = seq_sum_supported(out_sum, dims.size(), in.size())) return rc;
    SeqSumArgs a;
    std::memset(&a, 0, sizeof a);
    const int64_t eb = dtype == BNPP_F32 ? 4 : 8;
    bool has_elim = false;
    for (const View &v : in)
        for (int x : v.vars) has_elim = has_elim || (elim_var >= 0 && x == elim_var);
    a.k = has_elim ? cards[elim_var] : 1;
    a.n_terms = a.k;
    for (int x : dims) a.n_terms = sat_mul(a.n_terms, cards[x]);
    a.n_in = (int)in.size();
    a.n_dims = (int)dims.size();
    a.divide = divide ? 1 : 0;
    a.out = out_sum;
    for (size_t d = 0; d < dims.size(); ++d) a.card[d] = cards[dims[d]];
    for (size_t n = 0; n < in.size(); ++n) {
        a.in[n] = static_cast<const unsigned char *>(ptrs[n]) + in[n].base * eb;
        for (size_t j = 0; j < in[n].vars.size(); ++j) {
            const int x = in[n].vars[j];
            if (has_elim && x == elim_var) a.stride[n][kSeqMaxDims] = in[n].strides[j];
            for (size_t d = 0; d < dims.size(); ++d)
                if (dims[d] == x) a.stride[n][d] = in[n].strides[j];
        }
    }
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_seq_sum(dtype == BNPP_F32, a, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("partition sum launch: ") + hipGetErrorString(e));
    return BNPP_OK;
}

// evidence as a per-variable array (-1: none); validates ids and values
bool evidence_array(const ModelData &d, int n_ev, const int *ev_vars, const int *ev_vals, std::vector<int> &ev,
                    std::string &msg) {
    ev.assign(d.cards.size(), -1);
    if (n_ev < 0 || (n_ev > 0 && (!ev_vars || !ev_vals))) {
        msg = "bad evidence arrays";
        return false;
    }
    for (int i = 0; i < n_ev; ++i) {
        int v = ev_vars[i], x = ev_vals[i];
        if (v < 0 || v >= (int)d.cards.size() || x < 0 || x >= d.cards[v]) {
            msg = "evidence out of range";
            return false;
        }
        ev[v] = x;                          // evidence[id] = val (io.cpp:171)
    }
    return true;
}

std::vector<std::vector<int>> conditioned_scopes(const ModelData &d, const std::vector<int> &ev) {
    std::vector<std::vector<int>> sc(d.scopes.size());
    for (size_t f = 0; f < d.scopes.size(); ++f)
        for (int v : d.scopes[f])
            if (ev[v] < 0) sc[f].push_back(v);
    return sc;
}

std::vector<View> source_views(const ModelData &d, const std::vector<int> &ev) {
    std::vector<View> views;
    for (size_t f = 0; f < d.scopes.size(); ++f) views.push_back(conditioned_view((int)f, d.scopes[f], d.cards, ev));
    return views;
}

// Checkpoint-slot counts chosen by the bucket-tree search below, keyed on
// everything the plan's arena size depends on except the budget.  The search evaluates ~6 chain
// plans (≈60 ms on the 32x32 grid); a repeated MAR call on the same model then
// builds one plan.
// An entry holds for every budget in [need_ok, need_fail): the arena need of
// the chosen count and of the smallest count found not to fit.
struct SlotMemo {
    struct Entry {
        uint64_t key;
        int slots;
        int64_t need_ok, need_fail;
    };
    std::mutex mu;
    std::vector<Entry> entries;
};
SlotMemo &slot_memo() {
    static SlotMemo m;
    return m;
}
// the plan-changing switches (kPlanKnobs); a tuning build (BNPP_TUNING_KNOBS)
// keys on the whole BNPP_* environment, its knobs included
template <typename Mix>
void mix_plan_knobs(Mix &&mix) {
#ifdef BNPP_TUNING_KNOBS
    for (char **e = environ; e && *e; ++e)
        if (std::strncmp(*e, "BNPP_", 5) == 0)
            for (const char *c = *e; *c; ++c) mix((unsigned char)*c);
#else
    for (const char *k : kPlanKnobs) {
        const char *v = std::getenv(k);
        mix(0x9e37u);
        for (const char *c = v ? v : ""; *c; ++c) mix((unsigned char)*c);
    }
#endif
}

uint64_t slot_key(const std::vector<int> &cards, const std::vector<std::vector<int>> &scopes, const std::vector<int> &ord,
                  const std::vector<int> &targets, int eb, int chain_eb, int part, int n_parts, int n_slices) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t x) { h = (h ^ x) * 1099511628211ull; };
    auto mixv = [&](const std::vector<int> &v) {
        mix(v.size());
        for (int x : v) mix((uint32_t)x);
    };
    mixv(cards);
    mix(scopes.size());
    for (const auto &sc : scopes) mixv(sc);
    mixv(ord);
    mixv(targets);
    mix((uint64_t)eb);                    // the dtype: arena bytes scale with it
    mix((uint64_t)chain_eb);              // fused runs on/off change the plan
    mix((uint64_t)part);
    mix((uint64_t)n_parts);
    mix((uint64_t)n_slices);              // the slice rank does not change the arena need
    mix_plan_knobs(mix);                  // switches that change the plan and its arena need
    return h;
}

// Build the VE plans for a job: kind 0 = partition, kind 1 = marginals of
// targets, 2 = caller-chosen variables, 3 = bucket-tree marginals, 4 = MPE,
// 5 = posterior sampling of n_samples samples (internal: no public plan or job
// call takes it, bnpp_sample and bnpp_plan_sample do).
constexpr int kKindSample = 5;
int build_plans(const ModelData &d, const std::vector<int> &ev, int kind, int heuristic, const int *order,
                int n_order, const std::vector<int> &targets, std::vector<VEPlan> &plans, int &max_width,
                int64_t budget, int eb, int part = 0, int n_parts = 1, int n_slices = 1, int slice_rank = 0,
                int64_t n_samples = 0) {
    const int nv = (int)d.cards.size();
    auto scopes = conditioned_scopes(d, ev);
    auto views = source_views(d, ev);
    max_width = 0;
    const char *nc = std::getenv("BNPP_NO_CHAIN");                 // A/B: one launch per bucket
    const int chain_eb = nc && *nc == '1' ? 0 : eb;
    if (heuristic < BNPP_ORDER_GIVEN || heuristic > BNPP_MIN_DEGREE)
        return set_err(BNPP_ERR_INVALID, "unknown heuristic");
    if (kind == 2) {                                     // caller-chosen variables
        std::vector<int> vars(order, order + n_order), ord;
        for (int v : vars)
            if (v < 0 || v >= nv) return set_err(BNPP_ERR_INVALID, "bad variable");
        max_width = elimination_order(nv, d.cards, scopes, vars, (Heuristic)heuristic, ord);
        // BNPP_VE_CHAIN=1 (tests): fused runs as in kind 0, so that a run's message is
        // seen entry by entry; the result keeps the reference's scope order either way
        const char *vc = std::getenv("BNPP_VE_CHAIN");
        plans.push_back(plan_ve(d.cards, views, ord, true, vc && *vc == '1' ? chain_eb : 0));
    } else if (kind == 0) {
        std::vector<int> vars, ord;
        if (order) {
            std::vector<char> seen(nv, 0);
            for (int i = 0; i < n_order; ++i) {
                int v = order[i];
                if (v < 0 || v >= nv || seen[v]) return set_err(BNPP_ERR_INVALID, "bad explicit order");
                seen[v] = 1;
                if (ev[v] < 0) vars.push_back(v);
            }
            ord = vars;
            max_width = order_width(nv, scopes, ord);
        } else {
            for (int v = 0; v < nv; ++v)
                if (ev[v] < 0) vars.push_back(v);        // model.cpp:277-282
            max_width = elimination_order(nv, d.cards, scopes, vars, (Heuristic)heuristic, ord);
        }
        plans.push_back(plan_ve(d.cards, views, ord, true, chain_eb));
    } else if (kind == 4 || kind == kKindSample) {
        // most probable explanation: max-product over every non-evidence variable;
        // posterior sampling: the sum pass over the same order, then the draws
        std::vector<int> vars, ord;
        if (order) {
            std::vector<char> seen(nv, 0);
            for (int i = 0; i < n_order; ++i) {
                int v = order[i];
                if (v < 0 || v >= nv || seen[v]) return set_err(BNPP_ERR_INVALID, "bad explicit order");
                seen[v] = 1;
                if (ev[v] < 0) vars.push_back(v);
            }
            for (int v = 0; v < nv; ++v)
                if (!seen[v] && ev[v] < 0) return set_err(BNPP_ERR_INVALID, "explicit order must cover every non-evidence variable");
            ord = vars;
            max_width = order_width(nv, scopes, ord);
        } else {
            for (int v = 0; v < nv; ++v)
                if (ev[v] < 0) vars.push_back(v);
            max_width = elimination_order(nv, d.cards, scopes, vars, (Heuristic)heuristic, ord);
        }
        VEPlan mp;
        std::string msg;
        if (kind == kKindSample ? !plan_sample(d.cards, views, ord, ev, eb, n_samples, mp, &msg)
                                : !plan_mpe(d.cards, views, ord, ev, eb, mp, &msg))
            return set_err(BNPP_ERR_UNSUPPORTED, msg);
        plans.push_back(std::move(mp));
    } else if (kind == 3) {
        // all marginals from one two-pass bucket tree over the PR ordering
        std::vector<int> vars, ord;
        if (order) {
            std::vector<char> seen(nv, 0);
            for (int i = 0; i < n_order; ++i) {
                int v = order[i];
                if (v < 0 || v >= nv || seen[v]) return set_err(BNPP_ERR_INVALID, "bad explicit order");
                seen[v] = 1;
                if (ev[v] < 0) vars.push_back(v);
            }
            for (int v = 0; v < nv; ++v)
                if (!seen[v] && ev[v] < 0) return set_err(BNPP_ERR_INVALID, "explicit order must cover every non-evidence variable");
            ord = vars;
            max_width = order_width(nv, scopes, ord);
        } else {
            for (int v = 0; v < nv; ++v)
                if (ev[v] < 0) vars.push_back(v);
            max_width = elimination_order(nv, d.cards, scopes, vars, (Heuristic)heuristic, ord);
        }
        const bool tt = std::getenv("BNPP_TIMING") != nullptr;
        double tq = now_ms();
        auto need = [&](const VEPlan &p) { return sat_add(plan_arena_bytes(p, eb), (int64_t)p.buckets.size() * 512); };
        std::string msg;
        const char *force = std::getenv("BNPP_TREE_SLOTS");     // testing / tuning: chain mode, fixed slots
        if (force && std::atoi(force) > 0) {
            VEPlan cp;
            if (!plan_bucket_tree_chain(d.cards, views, ord, targets, std::atoi(force), part, n_parts, cp, &msg, chain_eb,
                                        n_slices, slice_rank, false, eb))
                return set_err(BNPP_ERR_UNSUPPORTED, msg);
            plans.push_back(std::move(cp));
            return BNPP_OK;
        }
        // plans the search leaves behind (the whole tree when it does not fit,
        // unused probes: ~2 ms each to free) are freed off the call's path
        std::vector<VEPlan> dead;
        struct Burial {
            std::vector<VEPlan> &d;
            ~Burial() {
                if (!d.empty()) std::thread([x = std::move(d)]() mutable { x.clear(); }).detach();
            }
        } burial{dead};
        // when the forward messages do not all fit, they are recomputed from
        // checkpoints (chain-shaped trees), with as many checkpoint slots as fit.
        // The slot search needs only the order, so its memo's plan or its first
        // probe round is planned beside the whole tree, which is used if it fits
        int lo = 1, hi = n_slices > 1 ? 256 : 64, best_s = 0;
        VEPlan best;
        const uint64_t key = slot_key(d.cards, scopes, ord, targets, eb, chain_eb, part, n_parts, n_slices);
        int memo_s = 0;
        {
            std::lock_guard<std::mutex> g(slot_memo().mu);
            for (const SlotMemo::Entry &e : slot_memo().entries)
                if (e.key == key && e.need_ok <= budget && budget < e.need_fail) memo_s = e.slots;
        }
        // first probe round: eight consecutive counts ending at the estimate
        // budget / largest message (a checkpoint slot holds one message; the
        // answer sits a few below it), so that one round usually brackets it
        int first_hi = 0;
        if (n_slices == 1 && memo_s == 0) {
            const double est = (double)budget / (order_max_table(nv, d.cards, scopes, ord) * eb);
            if (est >= 1 && est < hi) first_hi = (int)est;
        }
        std::vector<int> pre;                                // planned beside the whole tree
        if (n_slices == 1 && memo_s > 0) {
            pre.push_back(memo_s);
        } else if (first_hi > 0) {
            const int k = std::min(8, first_hi);             // first_hi - k + 1 .. first_hi (>= 1)
            for (int i = 0; i < k; ++i) pre.push_back(first_hi - (k - 1) + i);
            first_hi = 0;
        }
        const int npre = (int)pre.size();
        std::vector<VEPlan> pre_cps(npre);
        std::vector<int64_t> pre_nb(npre, 0);
        std::vector<char> pre_ok(npre, 0);
        std::vector<std::string> pre_msgs(npre);
        VEPlan tree;
        int64_t tree_need = 0;
        parallel_for((int64_t)npre + 1, [&](int64_t i) {
            if (i == 0) {
                tree = plan_bucket_tree(d.cards, views, ord, targets, part, n_parts);
                tree_need = need(tree);
                return;
            }
            pre_ok[i - 1] = plan_bucket_tree_chain(d.cards, views, ord, targets, pre[i - 1], part, n_parts, pre_cps[i - 1],
                                                   &pre_msgs[i - 1], chain_eb, n_slices, slice_rank, false, eb) ? 1 : 0;
            if (pre_ok[i - 1]) pre_nb[i - 1] = need(pre_cps[i - 1]);
        });
        if (tt) std::fprintf(stderr, "[bnpp] bucket tree: whole tree beside %d checkpointed plans %.1f ms\n", npre, now_ms() - tq);
        if (tree_need <= budget && n_parts == 1 && n_slices == 1) {
            plans.push_back(std::move(tree));
            for (VEPlan &c : pre_cps) dead.push_back(std::move(c));
            return BNPP_OK;
        }
        dead.push_back(std::move(tree));
        // sliced runs: the two-front schedule (two concurrent lanes, no
        // recomputation) when its arena fits, else checkpointing on one lane
        if (n_slices > 1 && !(tuning_knob("BNPP_SLICE_LANES") && *tuning_knob("BNPP_SLICE_LANES") == '0')) {
            VEPlan cp;
            if (plan_bucket_tree_chain(d.cards, views, ord, targets, 1, part, n_parts, cp, &msg, chain_eb, n_slices,
                                       slice_rank, true, eb)) {
                if (need(cp) <= budget) {
                    plans.push_back(std::move(cp));
                    return BNPP_OK;
                }
            } else {
                return set_err(BNPP_ERR_UNSUPPORTED, msg);
            }
        }
        if (memo_s > 0) {                                    // the search would land on the same count
            if (n_slices == 1) {
                if (pre_ok[0] && pre_nb[0] <= budget) {
                    best_s = memo_s;
                    best = std::move(pre_cps[0]);
                    lo = hi + 1;
                } else {
                    // the memo's count no longer fits this budget: search below
                    // it, the first round ending at the budget's estimate
                    if (pre_ok[0]) hi = std::min(hi, memo_s - 1);
                    const double est = (double)budget / (order_max_table(nv, d.cards, scopes, ord) * eb);
                    if (est >= 1 && est < hi) first_hi = (int)est;
                }
            } else {
                VEPlan cp;
                if (plan_bucket_tree_chain(d.cards, views, ord, targets, memo_s, part, n_parts, cp, &msg, chain_eb,
                                           n_slices, slice_rank, false, eb) &&
                    need(cp) <= budget) {
                    best_s = memo_s;
                    best = std::move(cp);
                    lo = hi + 1;
                }
            }
        }
        int64_t need_ok = 0, need_fail = INT64_MAX;
        bool exact = true;                                   // every probe planned: the bracket is valid
        // one probe round's results (probes ascending): the need grows with the slot count
        auto absorb = [&](const std::vector<int> &probe, std::vector<VEPlan> &cps, const std::vector<char> &planned,
                          const std::vector<int64_t> &nb, const std::vector<std::string> &msgs) {
            int new_lo = lo, new_hi = hi;
            for (size_t i = 0; i < probe.size(); ++i) {
                if (!planned[i]) {                           // as a bisection that stops at its first failure
                    exact = false;
                    if (msg.empty()) msg = msgs[i];
                    new_hi = std::min(new_hi, probe[i] - 1);
                    break;
                }
                if (nb[i] <= budget) {
                    if (probe[i] > best_s) {
                        if (best_s > 0) dead.push_back(std::move(best));
                        best_s = probe[i];
                        best = std::move(cps[i]);
                    }
                    need_ok = std::max(need_ok, nb[i]);      // valid for budgets >= every fitting probe's need
                    new_lo = std::max(new_lo, probe[i] + 1);
                } else {
                    need_fail = std::min(need_fail, nb[i]);
                    new_hi = std::min(new_hi, probe[i] - 1);
                    break;                                   // larger probes need more still
                }
            }
            lo = new_lo;
            hi = new_hi;
            for (VEPlan &c : cps) dead.push_back(std::move(c));
        };
        if (lo <= hi && memo_s == 0 && npre > 0) absorb(pre, pre_cps, pre_ok, pre_nb, pre_msgs);
        else
            for (VEPlan &c : pre_cps) dead.push_back(std::move(c));
        // further rounds: a k-ary search, up to 8 probes planned in parallel per
        // round (two rounds for 64 counts instead of six bisection steps)
        while (lo <= hi && exact) {
            tq = now_ms();
            const int m = hi - lo + 1;
            int n = std::min(8, m);
            std::vector<int> probe(n);                       // ascending, inside [lo, hi]
            for (int i = 0; i < n; ++i) probe[i] = m <= 8 ? lo + i : lo + (int)((int64_t)m * (i + 1) / (n + 1));
            if (first_hi > 0 && m > 8) {                     // (a memo plan that no longer fit)
                const int k = std::min(n, first_hi);
                probe.resize(k);
                n = k;
                for (int i = 0; i < k; ++i) probe[i] = first_hi - (k - 1) + i;
                first_hi = 0;
            }
            std::vector<VEPlan> cps(n);
            std::vector<int64_t> nb(n, 0);
            std::vector<char> planned(n, 0);
            std::vector<std::string> msgs(n);
            parallel_for((int64_t)n, [&](int64_t i) {
                planned[i] = plan_bucket_tree_chain(d.cards, views, ord, targets, probe[i], part, n_parts, cps[i],
                                                    &msgs[i], chain_eb, n_slices, slice_rank, false, eb) ? 1 : 0;
                if (planned[i]) nb[i] = need(cps[i]);
            });
            absorb(probe, cps, planned, nb, msgs);
            if (tt) std::fprintf(stderr, "[bnpp] bucket tree: %d slot probes %.1f ms\n", n, now_ms() - tq);
        }
        if (best_s > 0) {
            if (best_s != memo_s && exact) {
                std::lock_guard<std::mutex> g(slot_memo().mu);
                auto &en = slot_memo().entries;
                if (en.size() >= 64) en.erase(en.begin());
                en.push_back({key, best_s, need_ok, need_fail});
            }
            if (tt) std::fprintf(stderr, "[bnpp] bucket tree: %d checkpoint slots\n", best_s);
            plans.push_back(std::move(best));
        } else if (n_slices > 1) {
            return set_err(msg.empty() ? BNPP_ERR_OOM : BNPP_ERR_UNSUPPORTED,
                           msg.empty() ? "sliced bucket tree: no checkpoint count fits the memory budget" : msg);
        } else {
            // no checkpoint count fits (or the tree is not a chain): the whole
            // tree, which plan_schedules reports as over the budget
            plans.push_back(std::move(dead.front()));
            dead.erase(dead.begin());
        }
    } else {
        // one independent VE per target (model.cpp:326-334), planned in parallel
        plans.resize(targets.size());
        std::vector<int> widths(targets.size(), 0);
        std::vector<double> to(targets.size()), tp(targets.size());
        const double T0 = now_ms();
        parallel_for((int64_t)targets.size(), [&](int64_t i) {
            const int t = targets[i];
            std::vector<int> vars, ord;
            for (int v = 0; v < nv; ++v)                 // model.cpp:327-332 (evidence vars are no-ops)
                if (v != t && ev[v] < 0) vars.push_back(v);
            double a = now_ms();
            widths[i] = elimination_order(nv, d.cards, scopes, vars, (Heuristic)heuristic, ord);
            double b = now_ms();
            plans[i] = plan_ve(d.cards, views, ord, true);
            to[i] = b - a; tp[i] = now_ms() - b;
        });
        if (std::getenv("BNPP_TIMING")) {
            double so = 0, sp = 0;
            for (size_t i = 0; i < to.size(); ++i) {
                so += to[i];
                sp += tp[i];
            }
            std::fprintf(stderr, "[bnpp] per-target plans: wall %.1f ms, ordering %.1f ms, plan_ve %.1f ms (thread sums)\n",
                         now_ms() - T0, so, sp);
        }
        for (int w : widths) max_width = std::max(max_width, w);
    }
    return BNPP_OK;
}

// Analysis aid (BNPP_ARENA_PROFILE=path, host only): for every 1-GiB chunk of
// the arena, the algorithmic bytes the schedule has moved before its first
// launch touching the chunk -- how early a cold call needs each part of its
// arena mapped.  One line per chunk: "chunk cum_bytes group".
void arena_profile(const Schedule &s, int eb, const char *path) {
    FILE *f = std::fopen(path, "w");
    if (!f) return;
    const int64_t G = (int64_t)1 << 30;
    const int64_t nch = (s.arena_bytes + G - 1) / G;
    std::vector<double> first(nch, -1);
    std::vector<int> first_g(nch, -1);
    double cum = 0;
    for (size_t gi = 0; gi < s.groups.size(); ++gi) {
        const Schedule::Group &g = s.groups[gi];
        double moved = 0;
        for (int k = g.begin; k < g.end; ++k) {
            const BucketDesc &d = s.descs[k];
            int tabs[kMaxDescIn + 2];
            int nt = 0;
            const int n_read = d.n_in + ((d.flags & kChainBel) ? 1 : 0);
            for (int i = 0; i < n_read && i < kMaxDescIn; ++i) tabs[nt++] = d.in_table[i];
            tabs[nt++] = d.out_table;
            if (d.flags & kChainBel) tabs[nt++] = d.aux_out;
            for (int i = 0; i < nt; ++i) {
                const int t = tabs[i];
                if (t < 0) continue;
                moved += (double)s.table_size[t] * eb;
                if (t < (int)s.table_offset.size() && s.table_offset[t] >= 0) {
                    const int64_t a = s.table_offset[t] / G, b = (s.table_offset[t] + s.table_size[t] * eb - 1) / G;
                    for (int64_t c = a; c <= b && c < nch; ++c)
                        if (first[c] < 0) {
                            first[c] = cum;
                            first_g[c] = (int)gi;
                        }
                }
            }
        }
        cum += moved;
    }
    std::fprintf(f, "# arena %lld bytes, %zu groups, %.6g bytes moved\n", (long long)s.arena_bytes, s.groups.size(), cum);
    for (int64_t c = 0; c < nch; ++c) std::fprintf(f, "%lld %.6g %d\n", (long long)c, first[c], first_g[c]);
    std::fclose(f);
}

// Plans -> schedules.  MAR targets are split into batches whose estimated
// arenas fit `budget` bytes; a batch runs as one level-aligned schedule.
int plan_schedules(const ModelData &d, const std::vector<int> &ev, int kind, int heuristic, const int *order,
                   int n_order, const std::vector<int> &targets, int dtype, int64_t budget,
                   std::vector<Schedule> &out, double *stats, int part = 0, int n_parts = 1, int n_slices = 1,
                   int slice_rank = 0, int64_t n_samples = 0, double *sample_stats = nullptr) {
    std::vector<VEPlan> plans;
    int width = 0;
    const bool timing = std::getenv("BNPP_TIMING") != nullptr;
    double t0 = now_ms();
    const int eb = dtype == BNPP_F32 ? 4 : 8;
    int rc = build_plans(d, ev, kind, heuristic, order, n_order, targets, plans, width, budget, eb, part, n_parts,
                         n_slices, slice_rank, n_samples);
    if (rc) return rc;
    if (sample_stats && !plans.empty() && !plans[0].buckets.empty()) {
        sample_stats[0] = (double)plans[0].buckets.back().sample_rows.size();
        sample_stats[1] = (double)plans[0].sample_bytes;
    }
    if (timing) std::fprintf(stderr, "[bnpp] plans %.1f ms\n", now_ms() - t0);
    std::vector<int64_t> src_sizes;
    for (auto &v : d.values) src_sizes.push_back((int64_t)v.size());
    std::vector<std::vector<const VEPlan *>> batches(1);
    std::vector<int64_t> needs(plans.size());
    parallel_for((int64_t)plans.size(), [&](int64_t i) {
        const VEPlan &p = plans[i];
        needs[i] = sat_add(kind == 3 || kind == 4 || kind == kKindSample ? plan_arena_bytes(p, eb) : plan_peak_bytes(p, eb),
                           (int64_t)p.buckets.size() * 512);
    });
    int64_t acc = 0;
    for (size_t i = 0; i < plans.size(); ++i) {
        const VEPlan &p = plans[i];
        const int64_t need = needs[i];
        if (kind == 3 && need > budget) {
            char m[256];
            std::snprintf(m, sizeof m, "bucket-tree marginals need %.2f GB, budget %.2f GB: the tree is not a "
                          "chain or no checkpoint count fits (per-target marginals or a narrower order)", need / 1e9, budget / 1e9);
            return set_err(BNPP_ERR_OOM, m);
        }
        if (kind == 4 && need > budget) {
            // every arg table stays resident until the traceback (no checkpointing)
            char m[256];
            std::snprintf(m, sizeof m, "MPE needs %.3f GB (messages %.3f GB + arg tables %.3f GB, all resident until the "
                          "traceback), budget %.3f GB", need / 1e9, std::max<int64_t>(need - p.arg_bytes, 0) / 1e9,
                          p.arg_bytes / 1e9, budget / 1e9);
            return set_err(BNPP_ERR_OOM, m);
        }
        if (kind == kKindSample && need > budget) {
            // every message stays resident until the draws (no checkpointing), beside the samples
            char m[256];
            std::snprintf(m, sizeof m, "sampling needs %.3f GB (messages %.3f GB + samples %.3f GB, all resident until "
                          "the draws), budget %.3f GB", need / 1e9, std::max<int64_t>(need - p.sample_bytes, 0) / 1e9,
                          p.sample_bytes / 1e9, budget / 1e9);
            return set_err(BNPP_ERR_OOM, m);
        }
        if (!batches.back().empty() && sat_add(acc, need) > budget) {
            batches.emplace_back();
            acc = 0;
        }
        batches.back().push_back(&p);
        acc = sat_add(acc, need);
    }
    out.clear();
    std::string msg;
    double entries = 0, moved = 0, arena = 0, levels = 0, buckets = 0;
    for (auto &bp : batches) {
        Schedule s;
        const double tb = now_ms();
        if (!build_schedule(bp, d.cards, src_sizes, eb, max_vec_for(dtype), s, &msg, budget))
            return set_err(s.arena_bytes >= kSatMax ? BNPP_ERR_OOM : BNPP_ERR_INVALID, msg);
        if (timing) std::fprintf(stderr, "[bnpp] build_schedule call %.1f ms\n", now_ms() - tb);
        entries += s.entries;
        moved += s.elems_moved;
        arena = std::max(arena, (double)s.arena_bytes);
        if (timing) {
            int64_t ideal = 0;
            for (const VEPlan *pp : bp) ideal += plan_peak_bytes(*pp, eb);
            std::fprintf(stderr, "[bnpp] schedule: %zu buckets, %zu launches, ideal live peak %.2f GB, arena %.2f GB\n",
                         s.descs.size(), s.groups.size(), ideal / 1e9, s.arena_bytes / 1e9);
        }
        levels += s.n_levels;
        buckets += (double)s.descs.size();
        if (const char *prof = std::getenv("BNPP_ARENA_PROFILE")) arena_profile(s, eb, prof);
        out.push_back(std::move(s));
    }
    if (timing) std::fprintf(stderr, "[bnpp] schedules %.1f ms total\n", now_ms() - t0);
    stats[0] = entries;
    stats[1] = arena;
    stats[2] = levels;
    stats[3] = buckets;
    stats[4] = width;
    int64_t mx = 0;
    for (auto &p : plans) mx = std::max(mx, p.max_table);
    stats[5] = (double)mx;
    stats[6] = moved * eb;
    stats[7] = (double)out.size();
    double nx = 0, xe = 0;
    for (auto &p : plans) {
        nx += p.n_xchg;
        xe += p.xchg_elems;
    }
    stats[8] = nx;
    stats[9] = xe * eb;
    // the plans hold millions of small vectors (per-target MAR: one plan per
    // target, ~25 ms to free): a background thread frees them while the call
    // goes on to upload and launch (plans of one bucket tree: here)
    const double tf = now_ms();
    if (plans.size() > 1) {
        std::thread([dead = std::move(plans)]() mutable {
            parallel_for((int64_t)dead.size(), [&](int64_t i) { VEPlan d = std::move(dead[i]); });
        }).detach();
    } else {
        plans.clear();
    }
    if (timing) std::fprintf(stderr, "[bnpp] plans freed in %.1f ms\n", now_ms() - tf);
    return BNPP_OK;
}

// use_cache: the caller holds ctx->cache_mu and may reuse the cached arena, so
// its bytes count as free; a call that could not take the lock must not plan
// against memory another call is holding
int64_t memory_budget(bnpp_ctx *ctx, bool use_cache = false) {
    if (const char *e = std::getenv("BNPP_MEM_BUDGET_GB")) return (int64_t)(std::atof(e) * 1e9);
    if (ctx) {
        size_t fr = 0, tot = 0;
        (void)hipSetDevice(ctx->c.device);
        // 92 % of the free memory: an idle MI355X reports ~303 GB free, so
        // the 32x32 bucket tree plans 275-GB arenas -- fp64 five checkpoint
        // slots instead of four (30.2 against 31.9 TB), fp32 thirteen instead
        // of eleven (12.1 against 12.3 TB); 85 % until round 6
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0)
            return (int64_t)((fr + (use_cache ? ctx->c.arena_cache_bytes : 0)) * 0.92);
    }
    return (int64_t)64e9;
}

// the model's sources on the device in `dtype`, from the context's cache or
// uploaded now (and cached: at most 8 models, 512 MB)
int cached_sources(bnpp_ctx *ctx, const bnpp_model *m, int dtype, std::shared_ptr<DeviceSources> &out) {
    {
        std::lock_guard<std::mutex> g(ctx->src_mu);
        for (size_t i = 0; i < ctx->srcs.size(); ++i)
            if (ctx->srcs[i].uid == m->uid && ctx->srcs[i].dtype == dtype) {
                bnpp_ctx::Src e = ctx->srcs[i];
                ctx->srcs.erase(ctx->srcs.begin() + i);
                ctx->srcs.push_back(e);
                out = e.s;
                return BNPP_OK;
            }
    }
    Context *c = &ctx->c;
    std::shared_ptr<DeviceSources> s(new DeviceSources, [c](DeviceSources *p) {
        free_sources(*c, *p);
        delete p;
    });
    int rc = upload_sources(ctx->c, m->d.values, dtype == BNPP_F32 ? kF32 : kF64, *s);
    if (rc) return from_ctx(ctx, rc);
    out = s;
    std::lock_guard<std::mutex> g(ctx->src_mu);
    ctx->srcs.push_back({m->uid, dtype, s});
    size_t bytes = 0;
    for (const auto &e : ctx->srcs) bytes += e.s->buf_cap;
    while (ctx->srcs.size() > 8 || (ctx->srcs.size() > 1 && bytes > ((size_t)512 << 20))) {
        bytes -= ctx->srcs.front().s->buf_cap;
        ctx->srcs.erase(ctx->srcs.begin());
    }
    return BNPP_OK;
}

void evict_cached_job(bnpp_ctx *ctx);

int create_job(bnpp_ctx *ctx, const bnpp_model *m, int kind, int n_ev, const int *ev_vars, const int *ev_vals,
               int heuristic, const int *order, int n_order, int n_targets, const int *targets, int dtype,
               std::unique_ptr<bnpp_job> &job, int part = 0, int n_parts = 1, bool use_cache = false, int n_slices = 1,
               int slice_rank = 0, int64_t budget = 0, int64_t n_samples = 0) {
    if (!ctx || !m) return set_err(BNPP_ERR_INVALID, "null context or model");
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "bad dtype");
    const ModelData &d = m->d;
    job.reset(new bnpp_job);
    job->ctx = ctx;
    job->kind = kind;
    job->model_uid = m->uid;
    job->cards = d.cards;
    job->n_slices = n_slices;
    job->slice_rank = slice_rank;
    std::string msg;
    if (!evidence_array(d, n_ev, ev_vars, ev_vals, job->ev_val, msg)) return set_err(BNPP_ERR_INVALID, msg);
    if (kind == 1 || kind == 3) {
        if (targets) {
            for (int i = 0; i < n_targets; ++i) {
                if (targets[i] < 0 || targets[i] >= (int)d.cards.size()) return set_err(BNPP_ERR_INVALID, "bad target");
                job->targets.push_back(targets[i]);
            }
        } else {
            for (int v = 0; v < (int)d.cards.size(); ++v) job->targets.push_back(v);
        }
    }
    std::vector<Schedule> batches;
    if (n_parts < 1 || part < 0 || part >= n_parts) return set_err(BNPP_ERR_INVALID, "bad part / n_parts");
    if (use_cache) evict_cached_job(ctx);          // it runs in the arena this job may replace
    const double tp = now_ms();
    int rc = plan_schedules(d, job->ev_val, kind, heuristic, order, n_order, job->targets, dtype,
                            budget > 0 ? budget : memory_budget(ctx, use_cache), batches, job->stats, part, n_parts,
                            n_slices, slice_rank, n_samples);
    if (rc) return rc;
    const double t0 = now_ms();
    rc = cached_sources(ctx, m, dtype, job->src);
    if (rc) return rc;
    const double t1 = now_ms();
    rc = make_program(ctx->c, *job->src, std::move(batches), job->pg, use_cache);
    if (rc) return from_ctx(ctx, rc);
    g_timing[0] = t0 - tp;
    g_timing[1] = t1 - t0;
    g_timing[2] = now_ms() - t1;
    g_timing[7] = job->pg.arena_reused ? 1.0 : 0.0;
    g_timing[8] = job->pg.arena_alloc_ms;
    if (std::getenv("BNPP_TIMING"))
        std::fprintf(stderr, "[bnpp] job: upload %.1f ms, program (arena %.2f GB at %p) %.1f ms\n", t1 - t0,
                     job->pg.arena_bytes / 1e9, job->pg.arena, now_ms() - t1);
    return BNPP_OK;
}

void destroy_job(bnpp_job *job) {
    if (!job) return;
    (void)hipSetDevice(job->ctx->c.device);
    // the buffers go back to the context's cache for the next call: nothing
    // may still run on them (a job may have been launched on any stream; a
    // hipFree would wait the same way)
    (void)hipDeviceSynchronize();
    free_program(job->ctx->c, job->pg);
    job->src.reset();                               // the context's source cache may keep it
    delete job;
}

void evict_cached_job(bnpp_ctx *ctx) {
    if (ctx && ctx->job_cached) {
        destroy_job(ctx->job_cached);
        ctx->job_cached = nullptr;
        ctx->job_key = 0;
    }
}

// key of a one-shot call for the job cache (0: do not cache)
uint64_t call_key(const bnpp_model *m, int kind, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                  const int *order, int n_order, int n_targets, const int *targets, int dtype, int part, int n_parts) {
    if (std::getenv("BNPP_NO_JOB_CACHE")) return 0;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t x) { h = (h ^ x) * 1099511628211ull; };
    mix(m->uid);
    mix((uint64_t)kind);
    // evidence as a per-variable array; invalid evidence is never cached, so the
    // call goes on to create_job and fails there with BNPP_ERR_INVALID
    std::vector<int> ev;
    std::string msg;
    if (!evidence_array(m->d, n_ev, ev_vars, ev_vals, ev, msg)) return 0;
    for (int x : ev) mix((uint32_t)x);
    mix((uint64_t)heuristic);
    mix((uint64_t)n_order);
    for (int i = 0; i < n_order && order; ++i) mix((uint32_t)order[i]);
    mix((uint64_t)(targets ? n_targets : -1));
    for (int i = 0; i < n_targets && targets; ++i) mix((uint32_t)targets[i]);
    mix((uint64_t)dtype);
    mix((uint64_t)part);
    mix((uint64_t)n_parts);
    mix_plan_knobs(mix);
    return h ? h : 1;
}

// results of a launched job: partition -> out[0] = log10 Z (z_out: Z);
// marginals -> sum(card) normalised values; MPE -> out[0] = log10 of the
// maximum, then the assignment (n_vars values)
int job_results(bnpp_job *job, hipStream_t stream, double *out, double *z_out, int *owned = nullptr) {
    std::vector<std::vector<double>> vals;
    std::vector<int64_t> exp2;
    int rc = fetch_program(job->ctx->c, job->pg, stream, vals, exp2);
    if (rc) return from_ctx(job->ctx, rc);
    std::vector<const std::vector<int> *> rvars;
    std::vector<char> mine;
    for (auto &ex : job->pg.parts) {
        for (auto &v : ex.sched.plan_result_vars) rvars.push_back(&v);
        for (char c : ex.sched.plan_result_owned) mine.push_back(c);
    }
    if (job->kind == 4) {
        // the maximum (a scalar, scaled) and the traceback's assignment: int32
        // per variable in the program's results buffer, behind the scalar
        const double p = vals[0].empty() ? 0.0 : vals[0][0];
        out[0] = p > 0 ? std::log10(p) + (double)exp2[0] * std::log10(2.0) : -INFINITY;
        const size_t nv = job->cards.size();
        std::vector<int32_t> x(nv ? nv : 1, 0);
        const Program &pg = job->pg;
        if (pg.res_off.empty() || pg.res_off[0].size() < 2 || pg.res_off[0][1] < 0)
            return set_err(BNPP_ERR_INVALID, "MPE job without an assignment table");
        if (nv) {
            hipError_t e = hipMemcpy(x.data(), static_cast<const unsigned char *>(pg.results) + pg.res_off[0][1],
                                     nv * sizeof(int32_t), hipMemcpyDeviceToHost);
            if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("hipMemcpy(assignment): ") + hipGetErrorString(e));
        }
        for (size_t v = 0; v < nv; ++v) out[1 + v] = (double)x[v];
        return BNPP_OK;
    }
    if (job->kind == 0) {
        double p = 0;                                   // part.partition(): sequential sum
        for (double v : vals[0]) p += v;
        out[0] = p > 0 ? std::log10(p) + (double)exp2[0] * std::log10(2.0) : -INFINITY;
        if (z_out) *z_out = std::ldexp(p, (int)std::max<int64_t>(std::min<int64_t>(exp2[0], 1 << 20), -(1 << 20)));
        return BNPP_OK;
    }
    size_t o = 0;
    for (size_t i = 0; i < job->targets.size(); ++i) {
        int t = job->targets[i];
        int k = job->cards[t];
        const std::vector<double> &r = vals[i];
        const bool own = i >= mine.size() || mine[i];
        if (owned) owned[i] = own ? 1 : 0;
        if (!own) {                                     // another part computes it
            for (int s = 0; s < k; ++s) out[o + s] = 0.0;
        } else if (job->ev_val[t] >= 0) {               // evidence variable: one-hot
            for (int s = 0; s < k; ++s) out[o + s] = s == job->ev_val[t] ? 1.0 : 0.0;
        } else if ((int)r.size() == k && k > 0 && rvars[i]->size() == 1) {
            double part = 0;                            // Factor::normalize (factor.cpp:244-255)
            for (double v : r) part += v;
            for (int s = 0; s < k; ++s) out[o + s] = r[s] / part;
        } else {                                        // variable in no factor
            for (int s = 0; s < k; ++s) out[o + s] = 1.0 / k;
        }
        o += (size_t)k;
    }
    return BNPP_OK;
}

// results of a launched sliced job: this rank's share of every target's
// unnormalised marginal, as mantissas (out, sum(card)) and a power-of-two
// scale per target (out_exp2; kNoExp when the share is zero).  Evidence
// variables and variables in no factor: rank 0 carries the one-hot / uniform
// table.  A target that is a slice variable where it is delivered has a
// scalar share, at the index its value (the rank's bit) selects.
constexpr int64_t kNoExp = -((int64_t)1 << 40);
int job_results_sliced(bnpp_job *job, hipStream_t stream, double *out, int64_t *out_exp2) {
    std::vector<std::vector<double>> vals;
    std::vector<int64_t> exp2;
    int rc = fetch_program(job->ctx->c, job->pg, stream, vals, exp2);
    if (rc) return from_ctx(job->ctx, rc);
    std::vector<const std::vector<int> *> rvars;
    std::vector<int> sbit;
    for (auto &ex : job->pg.parts) {
        for (auto &v : ex.sched.plan_result_vars) rvars.push_back(&v);
        for (int b : ex.sched.plan_result_slice_bit) sbit.push_back(b);
    }
    const bool lead = job->slice_rank == 0;
    size_t o = 0;
    for (size_t i = 0; i < job->targets.size(); ++i) {
        const int t = job->targets[i], k = job->cards[t];
        const std::vector<double> &r = vals[i];
        const int sb = i < sbit.size() ? sbit[i] : -1;
        int64_t e = exp2[i];
        for (int s = 0; s < k; ++s) out[o + s] = 0.0;
        if (job->ev_val[t] >= 0) {                      // evidence variable: one-hot
            if (lead) out[o + job->ev_val[t]] = 1.0;
            e = 0;
        } else if (sb >= 0 && r.size() == 1) {          // slice variable: the rank's value
            out[o + ((job->slice_rank >> sb) & 1)] = r[0];
        } else if ((int)r.size() == k && k > 0 && rvars[i]->size() == 1) {
            for (int s = 0; s < k; ++s) out[o + s] = r[s];
        } else {                                        // variable in no factor: uniform
            if (lead)
                for (int s = 0; s < k; ++s) out[o + s] = 1.0 / k;
            e = 0;
        }
        bool any = false;
        for (int s = 0; s < k; ++s) any = any || out[o + s] != 0.0;
        out_exp2[i] = any ? e : kNoExp;
        o += (size_t)k;
    }
    return BNPP_OK;
}

// The plan depends on the memory budget (free memory, the cached arena
// counted as free), which moves a little between identical calls as other
// allocations come and go: within 2 % of the budget the cached job was
// planned under it is relaunched (its arena is allocated already, and a
// checkpoint count planned for a slightly different budget gives the same
// results); beyond that the call plans afresh
bool same_budget(int64_t a, int64_t b) {
    const int64_t d = a > b ? a - b : b - a;
    return a > 0 && b > 0 && d * 50 <= (a > b ? a : b);
}

// A one-shot call's job: the context's cached one when the call is identical
// (its planning phases read 0), else a new one (create).  cache_ok: the call
// holds cache_mu (it runs in the cached arena)
template <typename Create>
int oneshot_job(bnpp_ctx *ctx, bool cache_ok, uint64_t key, int64_t budget, Create &&create, bnpp_job *&job) {
    job = nullptr;
    if (cache_ok && key && ctx->job_cached && ctx->job_key == key && same_budget(ctx->job_budget, budget)) {
        job = ctx->job_cached;
        ctx->job_cached = nullptr;
        ctx->job_key = 0;
        for (int i = 0; i < 3; ++i) g_timing[i] = 0;
        g_timing[7] = 1;
        g_timing[8] = 0;
        return BNPP_OK;
    }
    std::unique_ptr<bnpp_job> j;
    const int rc = create(j);
    job = j.release();
    return rc;
}

// after the call: keep a good job for the next identical call, free the rest
void oneshot_done(bnpp_ctx *ctx, bool cache_ok, uint64_t key, int64_t budget, bnpp_job *job, int rc) {
    if (!job) return;
    if (rc == BNPP_OK && cache_ok && key) {
        evict_cached_job(ctx);
        ctx->job_cached = job;
        ctx->job_key = key;
        ctx->job_budget = budget;
    } else {
        destroy_job(job);
    }
}

// launch / run+fetch / free / total of a call whose create_job filled phases 0-2
void record_call_timing(double t0, double t1, double t2, double t3) {
    g_timing[3] = t2 - t1;
    g_timing[4] = t3 - t2;
    g_timing[5] = now_ms() - t3;
    g_timing[6] = now_ms() - t0;
}

// ---- batched calls: batched evidence (bnpp_partition_batch, bnpp_posterior_batch), expected counts
// (bnpp_expected_counts), batched MPE (bnpp_mpe_batch), batched sampling (bnpp_sample_batch), batched marginals
// (bnpp_marginals_batch) ----
// Each plans once for R rows per launch, stages the evidence variable-major, runs ceil(n_rows / R) launches and
// reads a table over the row variable B back per launch.  The job kinds (internal, like kKindSample) name the
// planner: plan_batch, plan_counts (the batched bucket tree), plan_mpe_batch, plan_sample_batch (K draws per row),
// plan_marginals_batch (the batched bucket tree handed out per row)
enum BatchKind { kKindBatch = 6, kKindCounts = 7, kKindMpeBatch = 8, kKindSampleBatch = 9, kKindMarginalsBatch = 10 };
constexpr int64_t kBatchAutoRows = (int64_t)1 << 16;   // the automatic R's cap

// what a batched call asks for (the plan entry points: no rows)
struct BatchCall {
    const bnpp_model *m;
    int kind;                                           // BatchKind
    int n_ev;
    const int *ev_vars;
    int heuristic;
    const int *order;
    int n_order;
    int dtype;
    int64_t rows_per_launch;
    int target = -1;                                    // kKindBatch: the posterior's variable, or -1 for Z
    int64_t K = 1;                                      // kKindSampleBatch: draws per row
    std::vector<int> targets;                           // kKindMarginalsBatch: the column blocks' variables, in order
    int64_t n_rows = 0;
    const int *ev_vals = nullptr;
    const unsigned char *partial = nullptr;             // [n_ev] or null: the evidence variables that may be missing (-1)
    bool is_partial(int j) const { return partial && partial[j]; }
    bool any_partial() const {
        for (int j = 0; j < n_ev && partial; ++j)
            if (partial[j]) return true;
        return false;
    }
    // soft evidence: the soft variables, and lik = double[n_rows][Ws], the variables' blocks in the listed order
    int n_soft = 0;
    const int *soft_vars = nullptr;
    const double *lik = nullptr;
    const bnpp_tables *tables = nullptr;                // the table set the plan reads (null: the model's own)
};

// the soft variable set (no values): ids in range, no duplicates, none an evidence variable or the target, each in
// a factor (its likelihoods need a table to carry them)
int batch_check_soft_vars(const BatchCall &c, bool posterior) {
    const ModelData &d = c.m->d;
    const int nv = (int)d.cards.size();
    if (c.n_soft < 0 || (c.n_soft > 0 && !c.soft_vars)) return set_err(BNPP_ERR_INVALID, "bad soft evidence arrays");
    std::vector<char> seen(nv, 0), is_ev(nv, 0);
    for (int j = 0; j < c.n_ev; ++j) is_ev[c.ev_vars[j]] = 1;
    for (int i = 0; i < c.n_soft; ++i) {
        const int v = c.soft_vars[i];
        if (v < 0 || v >= nv) return set_err(BNPP_ERR_INVALID, "soft variable " + std::to_string(v) + " out of range");
        if (seen[v]) return set_err(BNPP_ERR_INVALID, "soft variable " + std::to_string(v) + " is listed twice");
        if (is_ev[v])
            return set_err(BNPP_ERR_INVALID, "variable " + std::to_string(v) + " is both an evidence and a soft variable");
        if (posterior && v == c.target)
            return set_err(BNPP_ERR_INVALID, "the target " + std::to_string(v) + " is a soft variable");
        seen[v] = 1;
    }
    for (int i = 0; i < c.n_soft; ++i) {
        bool in_factor = false;
        for (const auto &sc : d.scopes) in_factor = in_factor || std::find(sc.begin(), sc.end(), c.soft_vars[i]) != sc.end();
        if (!in_factor)
            return set_err(BNPP_ERR_UNSUPPORTED, "soft variable " + std::to_string(c.soft_vars[i]) +
                                                     " is in no factor: no table can carry its likelihoods");
    }
    return BNPP_OK;
}

// the likelihoods of a batched call: finite and not negative
int batch_check_lik(const BatchCall &c) {
    if (c.n_soft <= 0) return BNPP_OK;
    if (!c.lik) return set_err(BNPP_ERR_INVALID, "bad soft evidence arrays");
    const ModelData &d = c.m->d;
    int64_t ws = 0;
    for (int i = 0; i < c.n_soft; ++i) ws += d.cards[c.soft_vars[i]];
    for (int64_t r = 0; r < c.n_rows; ++r) {
        const double *row = c.lik + r * ws;
        for (int i = 0; i < c.n_soft; ++i) {
            const int k = d.cards[c.soft_vars[i]];
            for (int x = 0; x < k; ++x)
                if (!(row[x] >= 0) || !std::isfinite(row[x]))
                    return set_err(BNPP_ERR_INVALID, "evidence row " + std::to_string(r) + ": the likelihood of value " +
                                                         std::to_string(x) + " of soft variable " +
                                                         std::to_string(c.soft_vars[i]) + " must be finite and not negative");
            row += k;
        }
    }
    return BNPP_OK;
}

// the evidence variable set (no values) and the target: ids in range, no duplicates
int batch_check_vars(const ModelData &d, int n_ev, const int *ev_vars, int target, bool posterior) {
    const int nv = (int)d.cards.size();
    if (n_ev < 0 || (n_ev > 0 && !ev_vars)) return set_err(BNPP_ERR_INVALID, "bad evidence arrays");
    std::vector<char> seen(nv, 0);
    for (int j = 0; j < n_ev; ++j) {
        const int v = ev_vars[j];
        if (v < 0 || v >= nv) return set_err(BNPP_ERR_INVALID, "evidence variable " + std::to_string(v) + " out of range");
        if (seen[v]) return set_err(BNPP_ERR_INVALID, "evidence variable " + std::to_string(v) + " is listed twice");
        seen[v] = 1;
    }
    if (posterior) {
        if (target < 0 || target >= nv) return set_err(BNPP_ERR_INVALID, "bad target");
        if (seen[target]) return set_err(BNPP_ERR_INVALID, "the target " + std::to_string(target) + " is an evidence variable");
    }
    return BNPP_OK;
}

// the rows of a batched call, checked before the context is looked at: a bad row fails the same with or without a device
int batch_check_rows(const BatchCall &c, bool posterior = false) {
    const ModelData &d = c.m->d;
    if (c.n_rows < 1) return set_err(BNPP_ERR_INVALID, "n_rows must be at least 1");
    if (int rc = batch_check_vars(d, c.n_ev, c.ev_vars, c.target, posterior)) return rc;
    if (c.n_soft != 0)
        if (int rc = batch_check_soft_vars(c, posterior)) return rc;
    if (c.n_ev > 0 && !c.ev_vals) return set_err(BNPP_ERR_INVALID, "bad evidence arrays");
    for (int64_t r = 0; r < c.n_rows; ++r)
        for (int j = 0; j < c.n_ev; ++j) {
            const int x = c.ev_vals[r * c.n_ev + j];
            if (x == BNPP_MISSING && c.is_partial(j)) continue;
            if (x < 0 || x >= d.cards[c.ev_vars[j]])
                return set_err(BNPP_ERR_INVALID, "evidence row " + std::to_string(r) + ": value " + std::to_string(x) +
                                                     " of variable " + std::to_string(c.ev_vars[j]) + " is outside [0, " +
                                                     std::to_string(d.cards[c.ev_vars[j]]) + ")");
        }
    return batch_check_lik(c);
}

// a null context.  say_no_device (batched MPE and sampling): no context can exist without a device, so say which it is
int batch_null_ctx(bool say_no_device) {
    int c = 0;
    if (say_no_device && (hipGetDeviceCount(&c) != hipSuccess || c <= 0))
        return set_err(BNPP_ERR_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    return set_err(BNPP_ERR_INVALID, "null context or model");
}

// Plan one launch: the elimination order the single call uses for this
// evidence variable set, then the kind's planner for R rows.  rows_per_launch 0:
// the largest power of two <= auto_cap (kBatchAutoRows, or less for a call of
// fewer rows: batch_auto_cap) whose arena fits `budget`.  plan_out: where the VEPlan goes, or null
int plan_batch_schedule(const BatchCall &c, int64_t budget, int64_t auto_cap, Schedule &out, double *stats, int64_t &R,
                        VEPlan *plan_out) {
    const ModelData &d = c.m->d;
    const int target = c.target, dtype = c.dtype, heuristic = c.heuristic;
    const bool counts = c.kind == kKindCounts, mpe = c.kind == kKindMpeBatch, smp = c.kind == kKindSampleBatch;
    const bool mar = c.kind == kKindMarginalsBatch;
    const int nv = (int)d.cards.size();
    const int eb = dtype == BNPP_F32 ? 4 : 8;
    int width = 0;
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "bad dtype");
    if (heuristic < BNPP_ORDER_GIVEN || heuristic > BNPP_MIN_DEGREE) return set_err(BNPP_ERR_INVALID, "unknown heuristic");
    if (c.rows_per_launch < 0 || c.rows_per_launch > (int64_t)INT32_MAX)
        return set_err(BNPP_ERR_INVALID, "rows_per_launch must be 0 (automatic) or in [1, 2^31)");
    std::vector<int> ev(nv, -1), evv(c.ev_vars, c.ev_vars + c.n_ev);
    std::vector<char> part;                                 // empty: no partial variable, the planners' own default
    if (c.any_partial()) part.assign(c.partial, c.partial + c.n_ev);
    const std::vector<int> soft(c.soft_vars, c.soft_vars + (c.soft_vars ? c.n_soft : 0));   // not evidence: eliminated
    // the order depends on which variables are observed in every row only: a partial variable is eliminated
    for (int j = 0; j < c.n_ev; ++j)
        if (!c.is_partial(j)) ev[evv[j]] = 0;
    auto scopes = conditioned_scopes(d, ev);
    std::vector<int> vars, ord;
    if (target < 0 && c.order) {                            // as build_plans, kind 0
        std::vector<char> seen(nv, 0);
        for (int i = 0; i < c.n_order; ++i) {
            int v = c.order[i];
            if (v < 0 || v >= nv || seen[v]) return set_err(BNPP_ERR_INVALID, "bad explicit order");
            seen[v] = 1;
            if (ev[v] < 0) vars.push_back(v);
        }
        if (mpe || smp || mar)                              // as build_plans, kind 4 and sampling
            for (int v = 0; v < nv; ++v)
                if (!seen[v] && ev[v] < 0)
                    return set_err(BNPP_ERR_INVALID, "explicit order must cover every non-evidence variable");
        ord = vars;
        width = order_width(nv, scopes, ord);
    } else {                                                // kind 0 / kind 1 (every variable but the target)
        for (int v = 0; v < nv; ++v)
            if (v != target && ev[v] < 0) vars.push_back(v);
        width = elimination_order(nv, d.cards, scopes, vars, (Heuristic)heuristic, ord);
    }
    if (smp)                                                // `out` holds one byte per variable, evidence included
        for (int v : evv)
            if (d.cards[v] > 256)
                return set_err(BNPP_ERR_UNSUPPORTED, "sampling: evidence variable " + std::to_string(v) + " has " +
                                                         std::to_string(d.cards[v]) +
                                                         " values; the samples hold one byte per variable (at most 256)");
    std::vector<View> views;
    for (size_t f = 0; f < d.scopes.size(); ++f) views.push_back(natural_view((int)f, d.scopes[f], d.cards));
    VEPlan plan;
    std::string msg;
    auto need_of = [&](const VEPlan &p) { return sat_add(plan_arena_bytes(p, eb), (int64_t)p.buckets.size() * 512); };
    int64_t need = 0;
    // counts: the batched bucket tree (plan_counts), every forward message resident through the backward pass
    auto make = [&](int64_t rows) {
        return counts ? plan_counts(d.cards, views, ord, evv, rows, eb, plan, &msg, part, soft)
               : mpe  ? plan_mpe_batch(d.cards, views, ord, evv, rows, eb, plan, &msg, part, soft)
               : smp  ? plan_sample_batch(d.cards, views, ord, evv, rows, c.K, eb, plan, &msg, part, soft)
               : mar  ? plan_marginals_batch(d.cards, views, ord, evv, rows, c.targets, eb, plan, &msg, part, soft)
                      : plan_batch(d.cards, views, ord, evv, rows, target, eb, plan, &msg, part, soft);
    };
    if (c.rows_per_launch > 0) {
        R = c.rows_per_launch;
        if (!make(R)) return set_err(BNPP_ERR_UNSUPPORTED, msg);
        need = need_of(plan);
    } else {
        for (R = auto_cap; R >= 1; R /= 2) {
            if (!make(R)) return set_err(BNPP_ERR_UNSUPPORTED, msg);
            need = need_of(plan);
            if (need <= budget || R == 1) break;
        }
    }
    if (need > budget && mpe) {
        // every arg table stays resident until the traceback (no checkpointing)
        char m[320];
        std::snprintf(m, sizeof m, "batched MPE needs %.6f GB (messages %lld bytes + arg tables %lld bytes, all resident "
                      "until the traceback) for %lld row%s per launch, budget %.6f GB", need / 1e9,
                      (long long)std::max<int64_t>(need - plan.arg_bytes, 0), (long long)plan.arg_bytes, (long long)R,
                      R == 1 ? "" : "s", budget / 1e9);
        return set_err(BNPP_ERR_OOM, m);
    }
    if (need > budget && smp) {
        // every message stays resident until the draws (no checkpointing), beside the state
        char m[320];
        std::snprintf(m, sizeof m, "batched sampling needs %.6f GB (messages %lld bytes + state %lld bytes, all resident "
                      "until the draws) for %lld row%s per launch of %lld draw%s each, budget %.6f GB", need / 1e9,
                      (long long)std::max<int64_t>(need - plan.sample_bytes, 0), (long long)plan.sample_bytes, (long long)R,
                      R == 1 ? "" : "s", (long long)c.K, c.K == 1 ? "" : "s", budget / 1e9);
        return set_err(BNPP_ERR_OOM, m);
    }
    if (need > budget && mar) {
        // every forward message stays resident through the backward pass, beside the output table
        char m[320];
        std::snprintf(m, sizeof m, "batched marginals need %.6f GB (messages %lld bytes + output %lld bytes) for %lld "
                      "row%s per launch, budget %.6f GB", need / 1e9,
                      (long long)std::max<int64_t>(need - plan.marg_out_bytes, 0), (long long)plan.marg_out_bytes,
                      (long long)R, R == 1 ? "" : "s", budget / 1e9);
        return set_err(BNPP_ERR_OOM, m);
    }
    if (need > budget) {
        char m[256];
        std::snprintf(m, sizeof m, "%s %.6f GB for %lld row%s per launch, budget %.6f GB",
                      counts ? "expected counts need" : "batched evidence needs", need / 1e9,
                      (long long)R, R == 1 ? "" : "s", budget / 1e9);
        return set_err(BNPP_ERR_OOM, m);
    }
    std::vector<int64_t> src_sizes;
    for (auto &v : d.values) src_sizes.push_back((int64_t)v.size());
    if (!build_schedule({&plan}, d.cards, src_sizes, eb, max_vec_for(dtype), out, &msg, budget))
        return set_err(out.arena_bytes >= kSatMax ? BNPP_ERR_OOM : BNPP_ERR_INVALID, msg);
    int64_t n_gather = 0;
    for (const Schedule::Group &g : out.groups) n_gather += cond_form_of_key(g.variant) >= 0;
    stats[0] = out.entries;
    stats[1] = (double)out.arena_bytes;
    stats[2] = out.n_levels;
    stats[3] = (double)out.descs.size();
    stats[4] = width;
    stats[5] = (double)plan.max_table;
    stats[6] = out.elems_moved * eb;
    stats[7] = 1;
    stats[8] = (double)R;
    stats[9] = (double)n_gather;
    if (plan_out) *plan_out = std::move(plan);
    return BNPP_OK;
}

// the automatic R never exceeds the smallest power of two that holds the
// call's rows: a launch should not work on padding mostly
int64_t batch_auto_cap(int64_t n_rows) {
    int64_t c = 1;
    while (c < n_rows && c < kBatchAutoRows) c *= 2;
    return c;
}

// what decides a batched call's plan: the evidence variable set and its column order (never the values), R or,
// for an automatic R, minus its cap (so calls of 2^16 rows or more, or of one size, share a job), the kind and K.
// Seed, first_sample and row_stride are launch data: other ones relaunch the cached job
uint64_t batch_call_key(const BatchCall &c, int64_t auto_cap) {
    if (std::getenv("BNPP_NO_JOB_CACHE")) return 0;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t x) { h = (h ^ x) * 1099511628211ull; };
    mix(c.tables ? c.tables->uid : c.m->uid);           // a table set has a job of its own: the model's is untouched
    mix((uint64_t)c.kind);
    mix((uint64_t)c.n_ev);
    for (int i = 0; i < c.n_ev; ++i) mix((uint32_t)c.ev_vars[i]);
    mix((uint64_t)c.heuristic);
    mix((uint64_t)c.n_order);
    for (int i = 0; i < c.n_order && c.order; ++i) mix((uint32_t)c.order[i]);
    mix((uint64_t)(int64_t)c.target);
    mix((uint64_t)c.dtype);
    mix((uint64_t)(c.rows_per_launch > 0 ? c.rows_per_launch : -auto_cap));
    mix((uint64_t)c.K);
    mix((uint64_t)c.targets.size());
    for (int t : c.targets) mix((uint32_t)t);
    if (c.any_partial())                                    // none: the key of the call without the argument
        for (int i = 0; i < c.n_ev; ++i) mix(0x9e3779b9ull + (c.partial[i] ? 1 : 0));
    if (c.n_soft > 0) {                                     // the variables, never the values; none: nothing
        mix(0x51f7ull + (uint64_t)c.n_soft);
        for (int i = 0; i < c.n_soft; ++i) mix((uint32_t)c.soft_vars[i]);
    }
    mix_plan_knobs(mix);
    return h ? h : 1;
}

// a batched call from its job to its epilogue: batch_open, batch_stage, batch_launches, batch_close
struct BatchRun {
    bnpp_ctx *ctx;
    const BatchCall &c;
    const double t0;                                    // the call's start
    std::unique_lock<std::mutex> lk;                    // cache_mu, where nobody else holds it
    bool cache_ok = false;
    int64_t budget = 0;
    uint64_t key = 0;
    bnpp_job *job = nullptr;
    double t1 = 0, launch_ms = 0, fetch_ms = 0;
    int64_t R = 0, n_launch = 0;
    int32_t *d_ev = nullptr;                            // the evidence table of the gather steps
    std::vector<int32_t> hev;
    // soft evidence: the likelihood table of the weighted gather steps, every launch's block T[Ws][R] (scaled, in the
    // call's dtype), per row the sum of its blocks' exponents (empty: no soft variable), the time the staging took
    void *d_lam = nullptr;
    std::vector<unsigned char> hlam;
    std::vector<int64_t> e_row;
    int64_t lam_bytes = 0;
    double lam_ms = 0;
    int64_t e_of(int64_t row) const { return e_row.empty() ? 0 : e_row[(size_t)row]; }
    bool has_b = false;                                 // the result table is over B (else: one value for every row)
    BatchRun(bnpp_ctx *x, const BatchCall &call, double start) : ctx(x), c(call), t0(start) {}
};

// the context's cached job when the call is identical, else a new one: plan, sources, program
int batch_open(BatchRun &run) {
    bnpp_ctx *ctx = run.ctx;
    const BatchCall &c = run.c;
    run.lk = std::unique_lock<std::mutex>(ctx->cache_mu, std::try_to_lock);
    const bool cache_ok = run.cache_ok = run.lk.owns_lock();
    const int64_t budget = run.budget = memory_budget(ctx, true);
    const int64_t auto_cap = batch_auto_cap(c.n_rows);
    run.key = cache_ok ? batch_call_key(c, auto_cap) : 0;
    const int rc = oneshot_job(ctx, cache_ok, run.key, budget, [&](std::unique_ptr<bnpp_job> &j) {
        j.reset(new bnpp_job);
        j->ctx = ctx;
        j->kind = c.kind;
        j->model_uid = c.m->uid;
        j->tables_uid = c.tables ? c.tables->uid : 0;
        j->cards = c.m->d.cards;
        if (cache_ok) evict_cached_job(ctx);       // it runs in the arena this job may replace
        const double tp = now_ms();
        std::vector<Schedule> batches(1);
        int rc2 = plan_batch_schedule(c, budget, auto_cap, batches[0], j->stats, j->batch_rows, nullptr);
        if (rc2) return rc2;
        const double ta = now_ms();
        if (c.tables) j->src = c.tables->src;       // the planner reads scopes and cards only: one plan for every set
        else rc2 = cached_sources(ctx, c.m, c.dtype, j->src);
        if (rc2) return rc2;
        const double tb = now_ms();
        rc2 = from_ctx(ctx, make_program(ctx->c, *j->src, std::move(batches), j->pg, cache_ok));
        if (rc2) return rc2;
        g_timing[0] = ta - tp;
        g_timing[1] = tb - ta;
        g_timing[2] = now_ms() - tb;
        g_timing[7] = j->pg.arena_reused ? 1.0 : 0.0;
        g_timing[8] = j->pg.arena_alloc_ms;
        return (int)BNPP_OK;
    }, run.job);
    run.t1 = now_ms();
    return rc;
}

// the job's R and launches, the tables its launches read their rows from (the evidence table, the likelihood
// table; none: no step reads one) and whether its result table is over B
void batch_bind(BatchRun &run) {
    const BatchCall &c = run.c;
    Executable &ex = run.job->pg.parts[0];
    const Schedule &sc = ex.sched;
    const int64_t R = run.R = run.job->batch_rows;
    run.n_launch = (c.n_rows + R - 1) / R;
    for (const Schedule::Group &g : sc.groups)
        if (cond_form_of_key(g.variant) >= 0 && sc.descs[g.begin].in_table[1] >= 0)
            run.d_ev = static_cast<int32_t *>(ex.h_meta[sc.descs[g.begin].in_table[1]].ptr);
        else if (g.variant == kMargRowsKey && sc.pool[sc.descs[g.begin].dim_off + 3] >= 0)   // an evidence block's, gather step or not
            run.d_ev = static_cast<int32_t *>(ex.h_meta[sc.pool[sc.descs[g.begin].dim_off + 3]].ptr);
    for (const Schedule::Group &g : sc.groups)
        if (cond_form_of_key(g.variant) == kCondWeighted && sc.descs[g.begin].in_table[2] >= 0)
            run.d_lam = ex.h_meta[sc.descs[g.begin].in_table[2]].ptr;
    const std::vector<int> &rv = sc.plan_result_vars[0];
    run.has_b = std::find(rv.begin(), rv.end(), (int)c.m->d.cards.size()) != rv.end();
}

// every launch's rows, variable-major, the last launch padded with its last row; kept to the end of
// the call (the copies are enqueued).  No evidence table: no factor mentions an evidence variable
void batch_stage(BatchRun &run) {
    const BatchCall &c = run.c;
    batch_bind(run);
    const int64_t R = run.R, n_launch = run.n_launch;
    if (run.d_ev) {
        const int n_ev = c.n_ev;                        // locals: the stores below could alias the call's fields
        const int64_t n_rows = c.n_rows;
        const int *ev_vals = c.ev_vals;
        run.hev.resize((size_t)(n_launch * n_ev * R));
        int32_t *hev = run.hev.data();
        for (int64_t L = 0; L < n_launch; ++L)
            for (int j = 0; j < n_ev; ++j)
                for (int64_t b = 0; b < R; ++b)
                    hev[(size_t)((L * n_ev + j) * R + b)] = ev_vals[std::min(L * R + b, n_rows - 1) * n_ev + j];
    }
    if (run.d_lam && c.n_soft > 0) {
        // per (row, variable) block an exact power of two brings the largest entry into [0.5, 1): every weight is at
        // most 1 (a gathered table keeps its source's bound), and rows of any magnitude share a launch's scale.  The
        // exponents go back to the row's log10 Z and Z.  Then T[Ws][R], padding rows copying the last row
        const double ts = now_ms();
        const int n_soft = c.n_soft;
        const int64_t n_rows = c.n_rows;
        const double *lik = c.lik;
        const bool f32 = c.dtype == BNPP_F32;
        std::vector<int> k(n_soft);
        int64_t ws = 0;
        for (int i = 0; i < n_soft; ++i) ws += (k[i] = c.m->d.cards[c.soft_vars[i]]);
        run.lam_bytes = ws * R * (f32 ? 4 : 8);
        run.hlam.resize((size_t)(n_launch * run.lam_bytes));
        run.e_row.assign((size_t)n_rows, 0);
        float *lf = reinterpret_cast<float *>(run.hlam.data());
        double *ld = reinterpret_cast<double *>(run.hlam.data());
        for (int64_t L = 0; L < n_launch; ++L)
            for (int64_t b = 0; b < R; ++b) {
                const int64_t row = std::min(L * R + b, n_rows - 1);
                const double *src = lik + row * ws;
                int64_t w = 0, e_sum = 0;
                for (int i = 0; i < n_soft; ++i) {
                    double top = 0;
                    for (int x = 0; x < k[i]; ++x) top = std::max(top, src[w + x]);
                    int e = 0;
                    if (top > 0) (void)std::frexp(top, &e);
                    e_sum += e;
                    for (int x = 0; x < k[i]; ++x) {
                        const double v = std::ldexp(src[w + x], -e);
                        const size_t at = (size_t)((L * ws + w + x) * R + b);
                        if (f32) lf[at] = (float)v;
                        else ld[at] = v;
                    }
                    w += k[i];
                }
                if (L * R + b < n_rows) run.e_row[(size_t)row] = e_sum;
            }
        run.lam_ms = now_ms() - ts;
        if (std::getenv("BNPP_TIMING"))
            std::fprintf(stderr, "[bnpp] soft evidence: staging %.3f ms for %lld rows x %lld likelihoods\n", run.lam_ms,
                         (long long)n_rows, (long long)ws);
    }
}

int no_hook(int64_t, int64_t) { return BNPP_OK; }

// The launches: per launch the evidence copy, before(L, rows) (what else the launch reads), the launch, and
// after(L, rows) (the fetch and the rows' unpacking); rows: the launch's rows that are the call's (the rest
// is padding).  Stops at the first error, and starts nothing on the device after it
template <typename Before, typename After>
int batch_launches(BatchRun &run, Before &&before, After &&after) {
    bnpp_ctx *ctx = run.ctx;
    const int64_t R = run.R, per = run.c.n_ev * R;
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    for (int64_t L = 0; L < run.n_launch; ++L) {
        const double ta = now_ms();
        const int64_t rows = std::min(R, run.c.n_rows - L * R);
        if (run.d_lam && run.lam_bytes > 0) {
            e = hipMemcpyAsync(run.d_lam, run.hlam.data() + (size_t)(L * run.lam_bytes), (size_t)run.lam_bytes,
                               hipMemcpyHostToDevice, ctx->c.stream);
            if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("hipMemcpyAsync(likelihoods): ") + hipGetErrorString(e));
        }
        if (run.d_ev && per > 0) {
            e = hipMemcpyAsync(run.d_ev, run.hev.data() + (size_t)(L * per), (size_t)per * sizeof(int32_t),
                               hipMemcpyHostToDevice, ctx->c.stream);
            if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("hipMemcpyAsync(evidence): ") + hipGetErrorString(e));
        }
        int rc = before(L, rows);
        if (rc) return rc;
        rc = from_ctx(ctx, launch_program(ctx->c, run.job->pg, ctx->c.stream));
        const double tb = now_ms();
        run.launch_ms += tb - ta;
        if (rc) return rc;
        rc = after(L, rows);
        if (rc) return rc;
        run.fetch_ms += now_ms() - tb;
    }
    return BNPP_OK;
}

// a launch's result table as doubles and its scale (batched evidence, counts); waits for the stream
int batch_fetch_doubles(BatchRun &run, std::vector<double> &r, int64_t &exp2) {
    std::vector<std::vector<double>> vals;
    std::vector<int64_t> e2;
    if (int rc = from_ctx(run.ctx, fetch_program(run.ctx->c, run.job->pg, run.ctx->c.stream, vals, e2))) return rc;
    r = std::move(vals[0]);
    exp2 = e2[0];
    return BNPP_OK;
}

// a launch's results buffer (the result table, then what the last step wrote) in one copy, and the result
// table's scale (batched MPE, sampling); synced_at: when the wait for the stream ended
int batch_fetch_raw(BatchRun &run, const char *what, std::vector<unsigned char> &raw, TableMeta &tm,
                    double *synced_at = nullptr) {
    const Program &pg = run.job->pg;
    const int rt = pg.parts[0].sched.plan_result_table[0];
    hipError_t e = hipStreamSynchronize(run.ctx->c.stream);
    if (synced_at) *synced_at = now_ms();
    if (e != hipSuccess ||
        (e = hipMemcpy(raw.data(), pg.results, (size_t)pg.results_bytes, hipMemcpyDeviceToHost)) != hipSuccess ||
        (rt >= 0 && (e = hipMemcpy(&tm, pg.parts[0].d_meta + rt, sizeof tm, hipMemcpyDeviceToHost)) != hipSuccess))
        return set_err(BNPP_ERR_HIP, std::string(what) + " fetch: " + hipGetErrorString(e));
    return BNPP_OK;
}

// element c of a raw table of floats (eb 4) or doubles; no table (no factor at all): the empty product
double raw_elem(const unsigned char *vals, int64_t c, int64_t eb) {
    double p = 1.0;
    if (vals && eb == 4) {
        float f;
        std::memcpy(&f, vals + c * 4, 4);
        p = f;
    } else if (vals) {
        std::memcpy(&p, vals + c * 8, 8);
    }
    return p;
}

// log10(p * 2^exp2).  The table's scale is shared by the rows of a launch, so p * 2^exp2 splits the same value
// differently at another R: take the logarithm of the split frexp gives, which the value alone decides
double log10_scaled(double p, int64_t exp2) {
    int pe = 0;
    const double pm = std::frexp(p, &pe);
    return p > 0 ? std::log10(pm) + (double)(exp2 + pe) * std::log10(2.0) : -INFINITY;
}

// after the call: keep a good job for the next identical call, and the call's phases
int batch_close(BatchRun &run, int rc, double *uptime_ms) {
    const double t3 = now_ms();
    oneshot_done(run.ctx, run.cache_ok, run.key, run.budget, run.job, rc);
    record_call_timing(run.t0, run.t1, run.t1 + run.launch_ms, t3);
    g_timing[4] = run.fetch_ms;
    if (rc) return rc;
    if (uptime_ms) *uptime_ms = now_ms() - run.t0;
    return BNPP_OK;
}

// what the _mv and _sv plan entries return last: per evidence variable the factor whose gather step carries its mask,
// per soft variable the one that carries its weights (-1: none); either array may be null
void report_evidence_factors(const VEPlan &plan, int n_ev, int *mask_factor, int n_soft, int *lam_factor) {
    for (int j = 0; mask_factor && j < n_ev; ++j)
        mask_factor[j] = j < (int)plan.batch_mask_factor.size() ? plan.batch_mask_factor[j] : -1;
    for (int j = 0; lam_factor && j < n_soft; ++j)
        lam_factor[j] = j < (int)plan.batch_lam_factor.size() ? plan.batch_lam_factor[j] : -1;
}

BatchCall batch_call(const bnpp_model *m, int kind, int n_ev, const int *ev_vars, int heuristic, const int *order,
                     int n_order, int dtype, int64_t rows_per_launch, const unsigned char *partial, int n_soft,
                     const int *soft_vars, const double *lik) {
    BatchCall c{};
    c.m = m;
    c.kind = kind;
    c.n_ev = n_ev;
    c.ev_vars = ev_vars;
    c.heuristic = heuristic;
    c.order = order;
    c.n_order = n_order;
    c.dtype = dtype;
    c.rows_per_launch = rows_per_launch;
    c.partial = partial;
    c.n_soft = n_soft;
    c.soft_vars = soft_vars;
    c.lik = lik;
    return c;
}

// target < 0: log10 Z and Z per row; else the posterior of target per row
int run_batch(bnpp_ctx *ctx, BatchCall &c, bool posterior, double *log10_z, double *z, double *post, double *uptime_ms) {
    const double t0 = now_ms();
    if (!c.m) return set_err(BNPP_ERR_INVALID, "null context or model");
    const ModelData &d = c.m->d;
    if (c.n_rows < 1) return set_err(BNPP_ERR_INVALID, "n_rows must be at least 1");
    if (posterior ? !post : !log10_z) return set_err(BNPP_ERR_INVALID, "null output");
    if (int rc = batch_check_rows(c, posterior)) return rc;
    if (!posterior) c.target = -1;
    if (c.dtype != BNPP_F32 && c.dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "bad dtype");
    if (!ctx) return batch_null_ctx(false);
    BatchRun run(ctx, c, t0);
    int rc = batch_open(run);
    if (rc == BNPP_OK && (run.job->pg.parts.size() != 1 || run.job->batch_rows < 1))
        rc = set_err(BNPP_ERR_INVALID, "batch job without a plan");
    if (rc == BNPP_OK) {
        batch_stage(run);
        const std::vector<int> &rv = run.job->pg.parts[0].sched.plan_result_vars[0];
        const bool has_b = run.has_b, has_t = posterior && std::find(rv.begin(), rv.end(), c.target) != rv.end();
        const int k = posterior ? d.cards[c.target] : 1;
        const int64_t R = run.R, nb = has_b ? R : 1;
        std::vector<double> r;
        int64_t exp2 = 0;
        rc = batch_launches(run, no_hook, [&](int64_t L, int64_t rows) {
            if (int rc2 = batch_fetch_doubles(run, r, exp2)) return rc2;
            if ((int64_t)r.size() != nb * (has_t ? k : 1))
                return set_err(BNPP_ERR_INVALID, "batch result table of an unexpected size");
            for (int64_t b = 0; b < rows; ++b) {
                const int64_t row = L * R + b, cb = has_b ? b : 0;
                if (!posterior) {                           // job_results, kind 0
                    double p = 0;
                    p += r[cb];
                    log10_z[row] = log10_scaled(p, exp2 + run.e_of(row));
                    if (z) z[row] = std::ldexp(p, (int)std::max<int64_t>(std::min<int64_t>(exp2 + run.e_of(row), 1 << 20), -(1 << 20)));
                } else if (has_t && k > 0) {                // Factor::normalize (factor.cpp:244-255), as job_results
                    double part = 0;
                    for (int s = 0; s < k; ++s) part += r[s * nb + cb];
                    for (int s = 0; s < k; ++s) post[row * k + s] = r[s * nb + cb] / part;
                } else {                                    // variable in no factor
                    for (int s = 0; s < k; ++s) post[row * k + s] = 1.0 / k;
                }
            }
            return (int)BNPP_OK;
        });
    }
    return batch_close(run, rc, uptime_ms);
}

// the last step of a batched MPE or sampling job (the traceback, the draws), or null: not such a job
const BucketDesc *batch_last_step(const bnpp_job *job, int32_t variant) {
    const Program &pg = job->pg;
    if (pg.parts.size() == 1 && job->batch_rows >= 1 && !pg.parts[0].sched.groups.empty() &&
        pg.parts[0].sched.groups.back().variant == variant && pg.res_off.size() == 1 && pg.res_off[0].size() == 2 &&
        pg.res_off[0][1] >= 0)
        return &pg.parts[0].sched.descs[pg.parts[0].sched.groups.back().begin];
    return nullptr;
}

int run_mpe_batch(bnpp_ctx *ctx, const BatchCall &c, double *log10_value, int *assignment, double *uptime_ms) {
    const double t0 = now_ms();
    if (!c.m) return set_err(BNPP_ERR_INVALID, "null context or model");
    const ModelData &d = c.m->d;
    if (int rc = batch_check_rows(c)) return rc;
    if (!log10_value && !assignment) return set_err(BNPP_ERR_INVALID, "null output");
    if (c.dtype != BNPP_F32 && c.dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "bad dtype");
    if (!ctx) return batch_null_ctx(true);
    const int64_t nv = (int64_t)d.cards.size(), n_ev = c.n_ev;
    const int *ev_vals = c.ev_vals;
    BatchRun run(ctx, c, t0);
    int rc = batch_open(run);
    const BucketDesc *dd = nullptr;
    if (rc == BNPP_OK && !(dd = batch_last_step(run.job, kMpeDecodeBatchKey)))
        rc = set_err(BNPP_ERR_INVALID, "batched MPE job without a traceback step");
    if (rc == BNPP_OK) {
        batch_stage(run);
        const Program &pg = run.job->pg;
        const Schedule &sc = pg.parts[0].sched;
        const int64_t R = run.R, eb = c.dtype == BNPP_F32 ? 4 : 8;
        // the variables the traceback writes (the rest: evidence values, 0 for a variable in no factor)
        std::vector<char> decoded((size_t)nv, 0);
        {
            const int64_t *w = sc.pool.data() + dd->dim_off;
            const int64_t *row = w + kDecodeBatchPoolHead;
            for (int64_t r = 0; r < w[1]; ++r) {
                decoded[(size_t)row[1]] = 1;
                row += 4 + 2 * row[3];
            }
        }
        std::vector<int> ev_col((size_t)nv, -1);
        for (int j = 0; j < c.n_ev; ++j) ev_col[(size_t)c.ev_vars[j]] = j;
        const int rt = sc.plan_result_table[0];
        const bool has_b = run.has_b;
        if ((rt < 0 ? 1 : pg.res_size[0][0]) != (has_b ? R : 1))
            rc = set_err(BNPP_ERR_INVALID, "batched MPE result table of an unexpected size");
        std::vector<unsigned char> raw((size_t)std::max<int64_t>(pg.results_bytes, 1));
        if (rc == BNPP_OK) rc = batch_launches(run, no_hook, [&](int64_t L, int64_t rows) {
            // the maxima table and x, and the maxima table's scale
            TableMeta tm{};
            if (int rc2 = batch_fetch_raw(run, "batched MPE", raw, tm)) return rc2;
            const unsigned char *vals = rt >= 0 ? raw.data() + pg.res_off[0][0] : nullptr;
            const uint8_t *x = raw.data() + pg.res_off[0][1];
            for (int64_t b = 0; b < rows; ++b) {
                const int64_t row = L * R + b;
                if (log10_value) log10_value[row] = log10_scaled(raw_elem(vals, has_b ? b : 0, eb), tm.exp2 + run.e_of(row));
                if (assignment)
                    for (int64_t v = 0; v < nv; ++v)
                        assignment[row * nv + v] = ev_col[(size_t)v] >= 0 && ev_vals[row * n_ev + ev_col[(size_t)v]] >= 0
                                                       ? ev_vals[row * n_ev + ev_col[(size_t)v]]   // observed, partial or not
                                                   : decoded[(size_t)v] ? (int)x[v * R + b]
                                                                        : 0;
            }
            return (int)BNPP_OK;
        });
    }
    return batch_close(run, rc, uptime_ms);
}

int run_sample_batch(bnpp_ctx *ctx, const BatchCall &c, int64_t first_sample, int64_t row_stride, uint64_t seed,
                     uint8_t *out, double *log10_z, int64_t *n_degenerate, double *uptime_ms) {
    const double t0 = now_ms();
    if (!c.m) return set_err(BNPP_ERR_INVALID, "null context or model");
    const ModelData &d = c.m->d;
    if (int rc = batch_check_rows(c)) return rc;
    if (c.K < 1) return set_err(BNPP_ERR_INVALID, "n_per_row must be at least 1");
    if (row_stride < 0 || first_sample < 0)
        return set_err(BNPP_ERR_INVALID, "row_stride and first_sample must be at least 0");
    {
        int64_t g = 0;                                     // one past the last global sample index
        if (__builtin_mul_overflow(c.n_rows - 1, row_stride, &g) || __builtin_add_overflow(g, first_sample, &g) ||
            __builtin_add_overflow(g, c.K, &g))
            return set_err(BNPP_ERR_INVALID, "first_sample + (n_rows - 1) * row_stride + n_per_row overflows int64");
    }
    if (c.dtype != BNPP_F32 && c.dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "bad dtype");
    if (!ctx) return batch_null_ctx(true);
    const int64_t nv = (int64_t)d.cards.size(), K = c.K, n_ev = c.n_ev;
    const int *ev_vals = c.ev_vals;
    BatchRun run(ctx, c, t0);
    int rc = batch_open(run);
    double stage_ms = 0, wait_ms = 0, copy_ms = 0, transpose_ms = 0;   // the host's share, printed under BNPP_TIMING
    const BucketDesc *sd = nullptr;
    if (rc == BNPP_OK && !(sd = batch_last_step(run.job, kSampleBatchKey)))
        rc = set_err(BNPP_ERR_INVALID, "batched sampling job without a draw step");
    if (rc == BNPP_OK) {
        const double ts = now_ms();
        batch_stage(run);
        stage_ms = now_ms() - ts;
        const Program &pg = run.job->pg;
        Executable &ex = run.job->pg.parts[0];
        const Schedule &sc = ex.sched;
        const int64_t R = run.R, lanes = R * K, eb = c.dtype == BNPP_F32 ? 4 : 8;
        if (sc.pool[sd->dim_off + 2] != R || sc.pool[sd->dim_off + 3] != K)
            rc = set_err(BNPP_ERR_INVALID, "batched sampling job of another shape");
        // the variables the draw step writes (the rest are evidence variables: the host fills them in)
        std::vector<int> ev_col((size_t)nv, -1);
        for (int j = 0; j < c.n_ev; ++j) ev_col[(size_t)c.ev_vars[j]] = j;
        const int rt = sc.plan_result_table[0];
        const bool has_b = run.has_b;
        if (rc == BNPP_OK && (rt < 0 ? 1 : pg.res_size[0][0]) != (has_b ? R : 1))
            rc = set_err(BNPP_ERR_INVALID, "batched sampling result table of an unexpected size");
        std::vector<unsigned char> raw((size_t)std::max<int64_t>(pg.results_bytes, 1));
        std::vector<char> impossible;                      // per row of the launch: Z == 0 (or NaN)
        ex.sample_seed = seed;
        ex.sample_first = first_sample;
        ex.sample_row_stride = row_stride;
        auto before = [&](int64_t L, int64_t rows) {
            ex.sample_row0 = L * R;
            ex.sample_n_valid = rows;
            return (int)BNPP_OK;
        };
        if (rc == BNPP_OK) rc = batch_launches(run, before, [&](int64_t L, int64_t rows) {
            // the table over (B), the state and the per-row counts, and the table's scale
            TableMeta tm{};
            const double tb = now_ms();
            double tw = tb;
            const int rc2 = batch_fetch_raw(run, "batched sampling", raw, tm, &tw);
            wait_ms += tw - tb;
            if (rc2) return rc2;
            const unsigned char *vals = rt >= 0 ? raw.data() + pg.res_off[0][0] : nullptr;
            const uint8_t *x = raw.data() + pg.res_off[0][1];
            const unsigned char *deg = x + sample_counter_offset(nv, lanes);
            impossible.assign((size_t)rows, 0);
            for (int64_t b = 0; b < rows; ++b) {
                const int64_t row = L * R + b;
                const double p = raw_elem(vals, has_b ? b : 0, eb);
                if (log10_z) log10_z[row] = log10_scaled(p, tm.exp2 + run.e_of(row));
                // an impossible row, as the single call: every draw degenerate, every sampled value 0
                impossible[(size_t)b] = !(p > 0);
                if (n_degenerate) {
                    if (impossible[(size_t)b]) n_degenerate[row] = K * (int64_t)sd->k;
                    else std::memcpy(&n_degenerate[row], deg + b * 8, 8);
                }
            }
            const double tc = now_ms();
            copy_ms += tc - tw;
            // x = uint8[n_vars][K][R] to out = [row][s][n_vars], evidence values from the row: per s a byte
            // in chunks of 256 rows, whose samples stay in cache while every variable's runs of the chunk
            // (contiguous in b) are read.  (Walking 64 rows at a time per draw measured slower: 9.8 ms
            // against 3.7 ms on ising12x12 at 2^16 rows with K = 1)
            constexpr int64_t kChunk = 256;
            for (int64_t b0 = 0; out && b0 < rows; b0 += kChunk) {
                const int64_t b1 = std::min(b0 + kChunk, rows);
                for (int64_t v = 0; v < nv; ++v) {
                    const int col = ev_col[(size_t)v];
                    uint8_t *o = out + (L * R * K) * nv + v;
                    if (col >= 0 && c.is_partial(col)) {    // observed: the row's value; missing: the draws
                        for (int64_t b = b0; b < b1; ++b) {
                            const int val = ev_vals[(L * R + b) * n_ev + col];
                            for (int64_t s = 0; s < K; ++s)
                                o[(b * K + s) * nv] = val >= 0                  ? (uint8_t)val
                                                      : impossible[(size_t)b] ? (uint8_t)0
                                                                              : x[v * lanes + s * R + b];
                        }
                    } else if (col >= 0) {
                        for (int64_t b = b0; b < b1; ++b) {
                            const uint8_t val = (uint8_t)ev_vals[(L * R + b) * n_ev + col];
                            for (int64_t s = 0; s < K; ++s) o[(b * K + s) * nv] = val;
                        }
                    } else {
                        for (int64_t s = 0; s < K; ++s) {
                            const uint8_t *xs = x + v * lanes + s * R;
                            for (int64_t b = b0; b < b1; ++b) o[(b * K + s) * nv] = impossible[(size_t)b] ? (uint8_t)0 : xs[b];
                        }
                    }
                }
            }
            transpose_ms += now_ms() - tc;
            return (int)BNPP_OK;
        });
    }
    const double launch_ms = run.launch_ms;
    rc = batch_close(run, rc, uptime_ms);
    if (rc == BNPP_OK && std::getenv("BNPP_TIMING"))
        std::fprintf(stderr, "[bnpp] sample_batch: stage %.3f ms, enqueue %.3f ms, wait %.3f ms, copy %.3f ms, transpose %.3f ms\n",
                     stage_ms, launch_ms, wait_ms, copy_ms, transpose_ms);
    return rc;
}

int run_counts(bnpp_ctx *ctx, const BatchCall &c, const double *weights, double *counts, double *log10_z,
               int64_t *n_impossible, double *uptime_ms) {
    const double t0 = now_ms();
    if (!c.m) return set_err(BNPP_ERR_INVALID, "null context or model");
    const ModelData &d = c.m->d;
    const int64_t n_rows = c.n_rows;
    if (n_rows < 1) return set_err(BNPP_ERR_INVALID, "n_rows must be at least 1");
    if (!counts) return set_err(BNPP_ERR_INVALID, "null output");
    if (int rc = batch_check_rows(c)) return rc;
    for (int64_t r = 0; weights && r < n_rows; ++r)
        if (!(weights[r] >= 0) || !std::isfinite(weights[r]))
            return set_err(BNPP_ERR_INVALID, "evidence row " + std::to_string(r) + ": the weight must be finite and not negative");
    if (c.dtype != BNPP_F32 && c.dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "bad dtype");
    if (!ctx) return batch_null_ctx(false);
    int64_t total = 0;
    for (const auto &v : d.values) total += (int64_t)v.size();
    BatchRun run(ctx, c, t0);
    int rc = batch_open(run);
    if (rc == BNPP_OK && (run.job->pg.parts.size() != 1 || run.job->batch_rows < 1))
        rc = set_err(BNPP_ERR_INVALID, "counts job without a plan");
    void *d_acc = nullptr;
    size_t acc_cap = 0;
    if (rc == BNPP_OK) {
        batch_stage(run);
        Executable &ex = run.job->pg.parts[0];
        const Schedule &sc = ex.sched;
        const int64_t R = run.R, nb = run.has_b ? R : 1;
        // the weights table of the accumulate steps, and every launch's weights (padding: 0)
        double *d_w = nullptr;
        for (const Schedule::Group &g : sc.groups)
            if (g.variant == kCountsKey && sc.pool[sc.descs[g.begin].dim_off + 8] >= 0)
                d_w = static_cast<double *>(ex.h_meta[sc.pool[sc.descs[g.begin].dim_off + 8]].ptr);
        std::vector<double> hw((size_t)(run.n_launch * R), 0.0);
        for (int64_t r = 0; r < n_rows; ++r) hw[(size_t)r] = weights ? weights[r] : 1.0;
        if (n_impossible) *n_impossible = 0;
        hipError_t e = hipSetDevice(ctx->c.device);
        if (e == hipSuccess) e = get_buffer(ctx->c, (size_t)std::max<int64_t>(total, 1) * sizeof(double), &d_acc, &acc_cap);
        if (e == hipSuccess) e = hipMemsetAsync(d_acc, 0, (size_t)std::max<int64_t>(total, 1) * sizeof(double), ctx->c.stream);
        if (e != hipSuccess) rc = set_err(e == hipErrorOutOfMemory ? BNPP_ERR_OOM : BNPP_ERR_HIP,
                                          std::string("accumulators: ") + hipGetErrorString(e));
        ex.counts_acc = static_cast<double *>(d_acc);
        auto before = [&](int64_t L, int64_t rows) {
            if (d_w) {
                e = hipMemcpyAsync(d_w, hw.data() + (size_t)(L * R), (size_t)R * sizeof(double), hipMemcpyHostToDevice,
                                   ctx->c.stream);
                if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("hipMemcpyAsync(evidence): ") + hipGetErrorString(e));
            }
            ex.counts_rows = rows;
            return (int)BNPP_OK;
        };
        std::vector<double> r;
        int64_t exp2 = 0;
        if (rc == BNPP_OK) rc = batch_launches(run, before, [&](int64_t L, int64_t rows) {
            if (int rc2 = batch_fetch_doubles(run, r, exp2)) return rc2;
            if ((int64_t)r.size() != nb) return set_err(BNPP_ERR_INVALID, "counts result table of an unexpected size");
            for (int64_t b = 0; b < rows; ++b) {
                double p = 0;
                p += r[run.has_b ? b : 0];
                if (log10_z) log10_z[L * R + b] = log10_scaled(p, exp2 + run.e_of(L * R + b));
                if (n_impossible && !(p > 0)) ++*n_impossible;
            }
            return (int)BNPP_OK;
        });
        ex.counts_acc = nullptr;
        if (rc == BNPP_OK && total > 0) {
            e = hipMemcpy(counts, d_acc, (size_t)total * sizeof(double), hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = set_err(BNPP_ERR_HIP, std::string("hipMemcpy(counts): ") + hipGetErrorString(e));
        }
    }
    if (d_acc) {
        (void)hipStreamSynchronize(ctx->c.stream);
        put_buffer(ctx->c, d_acc, acc_cap);
    }
    return batch_close(run, rc, uptime_ms);
}

// the targets of a batched-marginals call (null: all variables): in range, none twice
int marginals_targets(const ModelData &d, int n_targets, const int *targets, std::vector<int> &out) {
    const int nv = (int)d.cards.size();
    out.clear();
    if (!targets) {
        for (int v = 0; v < nv; ++v) out.push_back(v);
        if (out.empty()) return set_err(BNPP_ERR_INVALID, "the model has no variable");
        return BNPP_OK;
    }
    if (n_targets < 1) return set_err(BNPP_ERR_INVALID, "n_targets must be at least 1");
    std::vector<char> seen(nv, 0);
    for (int i = 0; i < n_targets; ++i) {
        const int t = targets[i];
        if (t < 0 || t >= nv) return set_err(BNPP_ERR_INVALID, "target " + std::to_string(t) + " out of range");
        if (seen[t]) return set_err(BNPP_ERR_INVALID, "target " + std::to_string(t) + " is listed twice");
        seen[t] = 1;
        out.push_back(t);
    }
    return BNPP_OK;
}

// an explicit order of a batched-marginals call covers every non-evidence variable (n_ev and ev_vars are checked)
int marginals_order_covers(const BatchCall &c) {
    if (!c.order) return BNPP_OK;
    const int nv = (int)c.m->d.cards.size();
    std::vector<char> seen(nv, 0);
    for (int i = 0; i < c.n_order; ++i) {
        const int v = c.order[i];
        if (v < 0 || v >= nv || seen[v]) return set_err(BNPP_ERR_INVALID, "bad explicit order");
        seen[v] = 1;
    }
    for (int j = 0; j < c.n_ev; ++j)
        if (!c.is_partial(j)) seen[c.ev_vars[j]] = 1;
    for (int v = 0; v < nv; ++v)
        if (!seen[v]) return set_err(BNPP_ERR_INVALID, "explicit order must cover every non-evidence variable");
    return BNPP_OK;
}

int run_marginals_batch(bnpp_ctx *ctx, const BatchCall &c, double *out, double *log10_z, double *uptime_ms) {
    const double t0 = now_ms();
    if (!c.m) return set_err(BNPP_ERR_INVALID, "null context or model");
    if (c.n_rows < 1) return set_err(BNPP_ERR_INVALID, "n_rows must be at least 1");
    if (!out) return set_err(BNPP_ERR_INVALID, "null output");
    if (int rc = batch_check_rows(c)) return rc;
    if (int rc = marginals_order_covers(c)) return rc;
    if (c.dtype != BNPP_F32 && c.dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "bad dtype");
    if (!ctx) return batch_null_ctx(false);
    BatchRun run(ctx, c, t0);
    int rc = batch_open(run);
    double stage_ms = 0, wait_ms = 0, copy_ms = 0;         // the host's share, printed under BNPP_TIMING
    const BucketDesc *ed = nullptr;
    if (rc == BNPP_OK && !(ed = batch_last_step(run.job, kMargRowsKey)))
        rc = set_err(BNPP_ERR_INVALID, "batched marginals job without an emit step");
    if (rc == BNPP_OK) {
        const double ts = now_ms();
        batch_stage(run);
        stage_ms = now_ms() - ts;
        const Program &pg = run.job->pg;
        Executable &ex = run.job->pg.parts[0];
        const Schedule &sc = ex.sched;
        const int64_t R = run.R, eb = c.dtype == BNPP_F32 ? 4 : 8, W = ed->out_size;
        int64_t w_call = 0;
        for (int t : c.targets) w_call += c.m->d.cards[t];
        if (sc.pool[ed->dim_off + 1] != R || W != w_call || pg.res_size[0][1] * eb < R * W * 8)
            rc = set_err(BNPP_ERR_INVALID, "batched marginals job of another shape");
        const int rt = sc.plan_result_table[0];
        const bool has_b = run.has_b;
        const int64_t nb = has_b ? R : 1;
        if (rc == BNPP_OK && (rt < 0 ? 1 : pg.res_size[0][0]) != nb)
            rc = set_err(BNPP_ERR_INVALID, "batched marginals result table of an unexpected size");
        std::vector<unsigned char> zr((size_t)(nb * eb));
        const unsigned char *res = static_cast<const unsigned char *>(pg.results);
        auto before = [&](int64_t, int64_t rows) {
            ex.marg_rows_live = rows;
            return (int)BNPP_OK;
        };
        if (rc == BNPP_OK) rc = batch_launches(run, before, [&](int64_t L, int64_t rows) {
            const double tb = now_ms();
            hipError_t e = hipStreamSynchronize(ctx->c.stream);
            const double tw = now_ms();
            wait_ms += tw - tb;
            // the launch's rows are contiguous in the caller's array: one copy, no host loop over entries
            if (e == hipSuccess)
                e = hipMemcpy(out + L * R * W, res + pg.res_off[0][1], (size_t)(rows * W * 8), hipMemcpyDeviceToHost);
            TableMeta tm{};
            if (e == hipSuccess && rt >= 0) e = hipMemcpy(zr.data(), res + pg.res_off[0][0], zr.size(), hipMemcpyDeviceToHost);
            if (e == hipSuccess && rt >= 0) e = hipMemcpy(&tm, ex.d_meta + rt, sizeof tm, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("batched marginals fetch: ") + hipGetErrorString(e));
            for (int64_t b = 0; log10_z && b < rows; ++b) {
                double p = 0;                                   // as run_batch
                p += raw_elem(rt >= 0 ? zr.data() : nullptr, has_b ? b : 0, eb);
                log10_z[L * R + b] = log10_scaled(p, tm.exp2 + run.e_of(L * R + b));
            }
            copy_ms += now_ms() - tw;
            return (int)BNPP_OK;
        });
    }
    const double launch_ms = run.launch_ms;
    rc = batch_close(run, rc, uptime_ms);
    if (rc == BNPP_OK && std::getenv("BNPP_TIMING"))
        std::fprintf(stderr, "[bnpp] marginals_batch: stage %.3f ms, enqueue %.3f ms, wait %.3f ms, copy %.3f ms\n", stage_ms,
                     launch_ms, wait_ms, copy_ms);
    return rc;
}

// ---- device-resident batched calls (_dv): rows and likelihoods from device memory, results to device memory ----

enum DvCall { kDvPartition, kDvMarginals, kDvMpe, kDvSample, kDvCounts };
const char *const kDvName[] = {"partition_batch_dv", "marginals_batch_dv", "mpe_batch_dv", "sample_batch_dv",
                               "expected_counts_dv"};

// the caller's device arrays of a _dv call, and the launch data of a sampling call
struct DvIo {
    int lik_dtype = BNPP_F64;
    bool log_only = false;                                 // bnpp_log_partition_dv: lik_dtype must be a log form
    double *log10_z = nullptr, *z = nullptr, *out = nullptr, *ln_z = nullptr;
    int32_t *assignment = nullptr;
    uint8_t *samples = nullptr;
    int64_t *n_degenerate = nullptr;
    int64_t first_sample = 0, row_stride = 0;
    uint64_t seed = 0;
    // bnpp_expected_counts_dv: the rows' weights (null: 1), the accumulators (kDvCounts), whether the fold goes on
    // from their values, and the counter of impossible rows (also with the batch plan, counts == NULL)
    const double *weights = nullptr;
    double *counts = nullptr;
    bool accumulate = false;
    int64_t *n_impossible = nullptr;
};

// batch_check_rows without the values (they are on the device: the staging steps check them)
int batch_check_rows_dv(const BatchCall &c, int lik_dtype, bool log_only = false) {
    if (c.n_rows < 1) return set_err(BNPP_ERR_INVALID, "n_rows must be at least 1");
    if (int rc = batch_check_vars(c.m->d, c.n_ev, c.ev_vars, c.target, false)) return rc;
    if (c.n_soft != 0)
        if (int rc = batch_check_soft_vars(c, false)) return rc;
    if (c.n_ev > 0 && !c.ev_vals) return set_err(BNPP_ERR_INVALID, "bad evidence arrays");
    if (c.n_soft > 0 && !c.lik) return set_err(BNPP_ERR_INVALID, "bad soft evidence arrays");
    if (c.n_soft > 0 && (lik_dtype < 0 || lik_dtype > (BNPP_F32 | BNPP_LIK_LOG))) return set_err(BNPP_ERR_INVALID, "bad lik_dtype");
    if (log_only && lik_dtype != (BNPP_F64 | BNPP_LIK_LOG) && lik_dtype != (BNPP_F32 | BNPP_LIK_LOG))
        return set_err(BNPP_ERR_INVALID, "bad lik_dtype: log likelihoods (BNPP_LIK_LOG) are required");
    return BNPP_OK;
}

// the sibling's message for the first invalid cell the staging steps found (st: the status block), or BNPP_OK
int dv_status_error(const BatchCall &c, const int64_t st[3], bool log_form) {
    const ModelData &d = c.m->d;
    if (st[0] != INT64_MAX) {
        int32_t x = 0;
        hipError_t e = hipMemcpy(&x, c.ev_vals + st[0], sizeof x, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("hipMemcpy(evidence cell): ") + hipGetErrorString(e));
        const int64_t r = st[0] / c.n_ev;
        const int v = c.ev_vars[st[0] % c.n_ev];
        return set_err(BNPP_ERR_INVALID, "evidence row " + std::to_string(r) + ": value " + std::to_string(x) +
                                             " of variable " + std::to_string(v) + " is outside [0, " +
                                             std::to_string(d.cards[v]) + ")");
    }
    if (st[1] != INT64_MAX) {
        int64_t ws = 0;
        for (int i = 0; i < c.n_soft; ++i) ws += d.cards[c.soft_vars[i]];
        const int64_t r = st[1] / ws;
        int64_t x = st[1] % ws;
        int i = 0;
        while (i + 1 < c.n_soft && x >= d.cards[c.soft_vars[i]]) x -= d.cards[c.soft_vars[i++]];
        return set_err(BNPP_ERR_INVALID, "evidence row " + std::to_string(r) + ": the likelihood of value " +
                                             std::to_string(x) + " of soft variable " + std::to_string(c.soft_vars[i]) +
                                             (log_form ? " must not be NaN or +inf" : " must be finite and not negative"));
    }
    if (st[2] != INT64_MAX)
        return set_err(BNPP_ERR_INVALID, "evidence row " + std::to_string(st[2]) + ": the weight must be finite and not negative");
    return BNPP_OK;
}

// One _dv call.  Per launch: the two staging steps from the caller's arrays at row0, the program, the emit steps
// into the caller's arrays at row0; everything on the context's stream, in order, with no host wait between
// launches.  One wait at the end, then the status block.  A log lik_dtype: stage_loglik for stage_lik, the blocks'
// tops in the scratch block, and the log emit form, which restores the rows' shifts (also taken for ln_z alone)
int run_batch_dv(bnpp_ctx *ctx, int call, BatchCall &c, const DvIo &io, double *uptime_ms) {
    const double t0 = now_ms();
    if (!c.m) return set_err(BNPP_ERR_INVALID, "null context or model");
    const ModelData &d = c.m->d;
    // the sibling's checks, in the sibling's order, the values left out
    if (call == kDvPartition || call == kDvMarginals) {
        if (c.n_rows < 1) return set_err(BNPP_ERR_INVALID, "n_rows must be at least 1");
        if (call == kDvPartition ? !io.log10_z && !io.ln_z : !io.out) return set_err(BNPP_ERR_INVALID, "null output");
    }
    if (call == kDvCounts && !io.counts) return set_err(BNPP_ERR_INVALID, "null output");
    // a table set belongs to one model and one dtype (and, once there is a context to compare, to it)
    if (c.tables && (c.tables->model_uid != c.m->uid || c.tables->dtype != c.dtype))
        return set_err(BNPP_ERR_INVALID, c.tables->model_uid != c.m->uid ? "the tables are those of another model"
                                                                         : "the tables are of another dtype than the call");
    if (int rc = batch_check_rows_dv(c, io.lik_dtype, io.log_only)) return rc;
    if (call == kDvMarginals)
        if (int rc = marginals_order_covers(c)) return rc;
    if (call == kDvMpe && !io.log10_z && !io.assignment) return set_err(BNPP_ERR_INVALID, "null output");
    if (call == kDvSample) {
        if (c.K < 1) return set_err(BNPP_ERR_INVALID, "n_per_row must be at least 1");
        if (io.row_stride < 0 || io.first_sample < 0)
            return set_err(BNPP_ERR_INVALID, "row_stride and first_sample must be at least 0");
        int64_t g = 0;                                     // one past the last global sample index
        if (__builtin_mul_overflow(c.n_rows - 1, io.row_stride, &g) || __builtin_add_overflow(g, io.first_sample, &g) ||
            __builtin_add_overflow(g, c.K, &g))
            return set_err(BNPP_ERR_INVALID, "first_sample + (n_rows - 1) * row_stride + n_per_row overflows int64");
    }
    if (c.dtype != BNPP_F32 && c.dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "bad dtype");
    if (!ctx) return batch_null_ctx(call == kDvMpe || call == kDvSample);
    if (c.tables && c.tables->ctx != ctx) return set_err(BNPP_ERR_INVALID, "the tables are those of another context");
    const int64_t nv = (int64_t)d.cards.size(), K = c.K;
    BatchRun run(ctx, c, t0);
    int rc = batch_open(run);
    const BucketDesc *last = nullptr;                      // the traceback, the draw step or the marginals' emit step
    if (rc == BNPP_OK && (call == kDvPartition || call == kDvCounts) &&
        (run.job->pg.parts.size() != 1 || run.job->batch_rows < 1))
        rc = set_err(BNPP_ERR_INVALID, call == kDvCounts ? "counts job without a plan" : "batch job without a plan");
    if (rc == BNPP_OK && call == kDvMpe && !(last = batch_last_step(run.job, kMpeDecodeBatchKey)))
        rc = set_err(BNPP_ERR_INVALID, "batched MPE job without a traceback step");
    if (rc == BNPP_OK && call == kDvSample && !(last = batch_last_step(run.job, kSampleBatchKey)))
        rc = set_err(BNPP_ERR_INVALID, "batched sampling job without a draw step");
    if (rc == BNPP_OK && call == kDvMarginals && !(last = batch_last_step(run.job, kMargRowsKey)))
        rc = set_err(BNPP_ERR_INVALID, "batched marginals job without an emit step");
    double stage_ms = 0, wait_ms = 0;
    void *scratch = nullptr;
    size_t scratch_cap = 0;
    if (rc == BNPP_OK) {
        const double ts = now_ms();
        batch_bind(run);
        const Program &pg = run.job->pg;
        Executable &ex = run.job->pg.parts[0];
        const Schedule &sc = ex.sched;
        const int64_t R = run.R, eb = c.dtype == BNPP_F32 ? 4 : 8, n_ev = c.n_ev, n_soft = c.n_soft;
        const int rt = sc.plan_result_table[0];
        const bool has_b = run.has_b;
        if ((rt < 0 ? 1 : pg.res_size[0][0]) != (has_b ? R : 1))
            rc = set_err(BNPP_ERR_INVALID, "batch result table of an unexpected size");
        int64_t W = 0;
        if (rc == BNPP_OK && call == kDvMarginals) {
            W = last->out_size;
            int64_t w_call = 0;
            for (int t : c.targets) w_call += d.cards[t];
            if (sc.pool[last->dim_off + 1] != R || W != w_call || pg.res_size[0][1] * eb < R * W * 8)
                rc = set_err(BNPP_ERR_INVALID, "batched marginals job of another shape");
        }
        if (rc == BNPP_OK && call == kDvSample && (sc.pool[last->dim_off + 2] != R || sc.pool[last->dim_off + 3] != K))
            rc = set_err(BNPP_ERR_INVALID, "batched sampling job of another shape");
        // the host block: the status words, then the three steps' descriptor words
        int64_t ws = 0;
        constexpr int kStatusWords = 3;                    // the first invalid evidence cell, likelihood, weight
        std::vector<int64_t> host(kStatusWords, INT64_MAX);
        for (int j = 0; j < n_ev; ++j) host.push_back((int64_t)d.cards[c.ev_vars[j]] | ((int64_t)(c.is_partial(j) ? 1 : 0) << 32));
        for (int i = 0; i < n_soft; ++i) {
            host.push_back((int64_t)d.cards[c.soft_vars[i]] | (ws << 32));
            ws += d.cards[c.soft_vars[i]];
        }
        if (call == kDvMpe || call == kDvSample) {
            std::vector<int> ev_col((size_t)nv, -1);
            for (int j = 0; j < n_ev; ++j) ev_col[(size_t)c.ev_vars[j]] = j;
            // the variables the last step writes: the traceback's rows; every variable the draws can reach
            std::vector<char> written((size_t)nv, 0);
            if (call == kDvMpe) {
                const int64_t *w = sc.pool.data() + last->dim_off;
                const int64_t *row = w + kDecodeBatchPoolHead;
                for (int64_t r = 0; r < w[1]; ++r) {
                    written[(size_t)row[1]] = 1;
                    row += 4 + 2 * row[3];
                }
            } else {
                for (int64_t v = 0; v < nv; ++v) written[(size_t)v] = ev_col[(size_t)v] < 0 || c.is_partial(ev_col[(size_t)v]);
            }
            for (int64_t v = 0; v < nv; ++v)
                host.push_back((int64_t)(uint32_t)ev_col[(size_t)v] |
                               ((int64_t)(ev_col[(size_t)v] >= 0 && c.is_partial(ev_col[(size_t)v]) ? 1 : 0) << 32) |
                               ((int64_t)written[(size_t)v] << 33));
        }
        // the device block: the host block, e_row, and a table of its own where the plan reads none (the values
        // are still checked, and the emit steps read the evidence)
        auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
        const int64_t host_bytes = (int64_t)host.size() * 8, o_erow = up(host_bytes), o_ev = o_erow + up(R * 8);
        const bool log_form = n_soft > 0 && (io.lik_dtype & BNPP_LIK_LOG);
        const int64_t o_lam = o_ev + (run.d_ev ? 0 : up(n_ev * R * 4)), o_top = o_lam + (run.d_lam ? 0 : up(ws * R * eb));
        const int64_t total = o_top + (log_form ? up(n_soft * R * 8) : 0);
        hipError_t e = hipSetDevice(ctx->c.device);
        if (rc == BNPP_OK && e == hipSuccess) e = get_buffer(ctx->c, (size_t)total, &scratch, &scratch_cap);
        if (rc == BNPP_OK && e == hipSuccess)
            e = hipMemcpyAsync(scratch, host.data(), (size_t)host_bytes, hipMemcpyHostToDevice, ctx->c.stream);
        if (rc == BNPP_OK && e != hipSuccess)
            rc = set_err(e == hipErrorOutOfMemory ? BNPP_ERR_OOM : BNPP_ERR_HIP, std::string("row staging buffer: ") + hipGetErrorString(e));
        char *base = static_cast<char *>(scratch);
        int64_t *d_status = reinterpret_cast<int64_t *>(base), *d_words = d_status + kStatusWords;
        int64_t *d_erow = reinterpret_cast<int64_t *>(base + o_erow);
        int32_t *d_ev = run.d_ev ? run.d_ev : n_ev > 0 ? reinterpret_cast<int32_t *>(base + o_ev) : nullptr;
        void *d_lam = run.d_lam ? run.d_lam : static_cast<void *>(base + o_lam);
        double *d_top = log_form ? reinterpret_cast<double *>(base + o_top) : nullptr;
        const bool scaled = run.d_lam && n_soft > 0;       // the rows' exponents go back to their results (batch_stage)
        const unsigned char *res = static_cast<const unsigned char *>(pg.results);
        const void *table = rt >= 0 ? res + pg.res_off[0][0] : nullptr;
        const TableMeta *tmeta = rt >= 0 ? ex.d_meta + rt : nullptr;
        if (call == kDvSample) {
            ex.sample_seed = io.seed;
            ex.sample_first = io.first_sample;
            ex.sample_row_stride = io.row_stride;
        }
        // expected counts: the weights table of the accumulate steps; the caller's array is the accumulator buffer,
        // zeroed on the stream unless the fold goes on from its values
        double *d_w = nullptr;
        if (rc == BNPP_OK && call == kDvCounts) {
            for (const Schedule::Group &g : sc.groups)
                if (g.variant == kCountsKey && sc.pool[sc.descs[g.begin].dim_off + 8] >= 0)
                    d_w = static_cast<double *>(ex.h_meta[sc.pool[sc.descs[g.begin].dim_off + 8]].ptr);
            int64_t total = 0;
            for (const auto &v : d.values) total += (int64_t)v.size();
            if (!io.accumulate && total > 0) e = hipMemsetAsync(io.counts, 0, (size_t)total * sizeof(double), ctx->c.stream);
            ex.counts_acc = io.counts;
        }
        if (rc == BNPP_OK && e == hipSuccess && io.n_impossible)
            e = hipMemsetAsync(io.n_impossible, 0, sizeof(int64_t), ctx->c.stream);
        // a table set: its factors' metadata as they are now, into the pristine copy every launch restores.  The
        // source pointers were baked in when the job was made and never move; no exponent reaches the host
        if (rc == BNPP_OK && e == hipSuccess && c.tables && sc.n_src > 0)
            e = hipMemcpyAsync(ex.d_meta0, c.tables->d_meta, (size_t)sc.n_src * sizeof(TableMeta), hipMemcpyDeviceToDevice,
                               ctx->c.stream);
        if (rc == BNPP_OK && e != hipSuccess) rc = set_err(BNPP_ERR_HIP, std::string("call setup: ") + hipGetErrorString(e));
        const double *tshift = c.tables && c.tables->log_form ? c.tables->d_shift : nullptr;
        stage_ms = now_ms() - ts;
        for (int64_t L = 0; rc == BNPP_OK && L < run.n_launch; ++L) {
            const double ta = now_ms();
            const int64_t row0 = L * R, rows = std::min(R, c.n_rows - row0);
            if (n_ev > 0) {
                RowioSingle<StageRowsArgs> a;
                a.a = StageRowsArgs{d_words, c.ev_vals, d_ev, d_status, c.n_rows, row0, R, n_ev};
                e = launch_stage_rows(a, ctx->c.max_grid, ctx->c.stream);
            }
            if (e == hipSuccess && n_soft > 0) {
                RowioSingle<StageLikArgs> a;
                a.a = StageLikArgs{d_words + n_ev, c.lik, d_lam, d_erow, d_status, c.n_rows, row0, R, ws, n_soft,
                                   (io.lik_dtype & BNPP_F32) != 0, c.dtype == BNPP_F32, d_top};
                e = log_form ? launch_stage_loglik(a, ctx->c.max_grid, ctx->c.stream)
                             : launch_stage_lik(a, ctx->c.max_grid, ctx->c.stream);
            }
            if (e == hipSuccess && d_w) {
                const StageWeightsArgs a{io.weights, d_w, d_status, c.n_rows, row0, R};
                e = launch_stage_weights(a, ctx->c.max_grid, ctx->c.stream);
            }
            if (e != hipSuccess) {
                rc = set_err(BNPP_ERR_HIP, std::string("row staging: ") + hipGetErrorString(e));
                break;
            }
            ex.counts_rows = rows;
            ex.sample_row0 = row0;
            ex.sample_n_valid = rows;
            ex.marg_rows_live = rows;
            rc = from_ctx(ctx, launch_program(ctx->c, run.job->pg, ctx->c.stream));
            if (rc) break;
            {
                // the shifts go back with the exponents: both belong to the table the plan reads (`scaled`).  A soft
                // variable is in some factor's scope and that factor's gather is weighted, so n_soft > 0 implies
                // run.d_lam; were there a plan without one, it would ignore the likelihoods in either form
                const bool shifted = scaled && log_form;
                const EmitScalarsArgs a{table, tmeta, scaled ? d_erow : nullptr, io.log10_z, io.z, row0, rows,
                                        c.dtype == BNPP_F32, has_b, shifted ? d_top : nullptr, io.ln_z,
                                        shifted ? n_soft : 0, R, tshift, io.n_impossible};
                if (log_form || io.ln_z || tshift) {           // log-form tables: the shift goes back in the log emit
                    if (io.log10_z || io.ln_z || io.z || io.n_impossible) e = launch_emit_logs(a, ctx->c.max_grid, ctx->c.stream);
                } else if (io.log10_z || io.n_impossible) {
                    e = launch_emit_scalars(a, ctx->c.max_grid, ctx->c.stream);
                }
            }
            if (e == hipSuccess && (call == kDvMpe ? io.assignment != nullptr : call == kDvSample)) {
                const uint8_t *x = res + pg.res_off[0][1];
                RowioSingle<EmitStatesArgs> a;
                a.a = EmitStatesArgs{d_words + n_ev + n_soft, x, d_ev, table,
                                     reinterpret_cast<const unsigned long long *>(x + sample_counter_offset(nv, R * K)),
                                     call == kDvMpe ? static_cast<void *>(io.assignment) : static_cast<void *>(io.samples),
                                     io.n_degenerate, nv, call == kDvMpe ? 1 : K, R, row0, rows, (int64_t)last->k,
                                     call == kDvSample, c.dtype == BNPP_F32, has_b, 0};
                e = launch_emit_states(a, ctx->c.max_grid, ctx->c.stream);
            }
            if (e == hipSuccess && call == kDvMarginals)   // the launch's rows are contiguous in the caller's array
                e = hipMemcpyAsync(io.out + row0 * W, res + pg.res_off[0][1], (size_t)(rows * W * 8), hipMemcpyDeviceToDevice,
                                   ctx->c.stream);
            if (e != hipSuccess) rc = set_err(BNPP_ERR_HIP, std::string("row emit: ") + hipGetErrorString(e));
            run.launch_ms += now_ms() - ta;
        }
        // the call's one wait, then the status block
        const double tw = now_ms();
        e = hipStreamSynchronize(ctx->c.stream);
        wait_ms = now_ms() - tw;
        ex.counts_acc = nullptr;
        int64_t st[kStatusWords] = {INT64_MAX, INT64_MAX, INT64_MAX};
        if (e == hipSuccess && scratch) e = hipMemcpy(st, d_status, sizeof st, hipMemcpyDeviceToHost);
        if (rc == BNPP_OK && e != hipSuccess) rc = set_err(BNPP_ERR_HIP, std::string(kDvName[call]) + ": " + hipGetErrorString(e));
        if (rc == BNPP_OK) rc = dv_status_error(c, st, n_soft > 0 && (io.lik_dtype & BNPP_LIK_LOG));
        run.fetch_ms = now_ms() - tw;
    }
    if (scratch) put_buffer(ctx->c, scratch, scratch_cap);
    const double launch_ms = run.launch_ms;
    rc = batch_close(run, rc, uptime_ms);
    if (rc == BNPP_OK && std::getenv("BNPP_TIMING"))
        std::fprintf(stderr, "[bnpp] %s: stage %.3f ms, enqueue %.3f ms, wait %.3f ms\n", kDvName[call], stage_ms, launch_ms, wait_ms);
    return rc;
}

// the launch groups of schedule `batch`, from row n of the caller's rows on: the rows after them
int64_t copy_group_rows(const Schedule &s, int64_t batch, int64_t *rows, int64_t cap_rows, int64_t n) {
    for (const Schedule::Group &g : s.groups) {
        if (n < cap_rows) {
            const int64_t v[BNPP_PLAN_GROUP_FIELDS] = {batch, g.level, g.variant, g.end - g.begin, g.vblocks, g.lane};
            std::copy(v, v + BNPP_PLAN_GROUP_FIELDS, rows + n * BNPP_PLAN_GROUP_FIELDS);
        }
        ++n;
    }
    return n;
}

// a batched plan entry point: the null checks, the variable set, the schedule (and its plan), the
// group rows.  st: at least 10 stats, which plan_batch_schedule fills
int plan_batch_entry(const BatchCall &c, bool posterior, double *stats, int n_stats, int64_t *rows, int cap_rows,
                     int *n_rows, Schedule &s, VEPlan &plan, double *st) {
    if (!c.m || !n_rows || (cap_rows > 0 && !rows) || (n_stats > 0 && !stats)) return set_err(BNPP_ERR_INVALID, "null argument");
    if (int rc = batch_check_vars(c.m->d, c.n_ev, c.ev_vars, c.target, posterior)) return rc;
    if (c.n_soft != 0)
        if (int rc = batch_check_soft_vars(c, posterior)) return rc;
    if (c.K < 1) return set_err(BNPP_ERR_INVALID, "n_per_row must be at least 1");
    int64_t R = 0;
    if (int rc = plan_batch_schedule(c, memory_budget(nullptr), kBatchAutoRows, s, st, R, &plan)) return rc;
    *n_rows = (int)copy_group_rows(s, 0, rows, cap_rows, 0);
    return BNPP_OK;
}

}  // namespace

extern "C" {

int bnpp_counts_size(const bnpp_model *m, int64_t *n) {
    if (!m || !n) return set_err(BNPP_ERR_INVALID, "null argument");
    *n = 0;
    for (const auto &v : m->d.values) *n += (int64_t)v.size();
    return BNPP_OK;
}

int bnpp_expected_counts_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik, const double *weights, int heuristic,
                            const int *order, int n_order, int dtype, int64_t rows_per_launch, double *counts,
                            double *log10_z, int64_t *n_impossible, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindCounts, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, lik);
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    return run_counts(ctx, c, weights, counts, log10_z, n_impossible, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_expected_counts_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, const double *weights, int heuristic,
                            const int *order, int n_order, int dtype, int64_t rows_per_launch, double *counts,
                            double *log10_z, int64_t *n_impossible, double *uptime_ms) {
    return bnpp_expected_counts_sv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, partial, 0, nullptr, nullptr, weights, heuristic, order, n_order, dtype, rows_per_launch, counts, log10_z, n_impossible, uptime_ms);
}

int bnpp_expected_counts(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals, const double *weights, int heuristic, const int *order, int n_order,
                         int dtype, int64_t rows_per_launch, double *counts, double *log10_z, int64_t *n_impossible,
                         double *uptime_ms) {
    return bnpp_expected_counts_mv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, nullptr, weights, heuristic, order,
                                   n_order, dtype, rows_per_launch, counts, log10_z, n_impossible, uptime_ms);
}

int bnpp_plan_counts_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik,
                        int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                        double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *belief_off,
                        int *belief_vars, int cap_belief, int *n_belief, int *no_b_elim, int *mask_factor, int *lam_factor) {
    BNPP_GUARD_BEGIN
    Schedule s;
    VEPlan plan;
    double st[12] = {0};
    BatchCall c = batch_call(m, kKindCounts, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, lik);
    if (int rc = plan_batch_entry(c, false, stats, n_stats, rows, cap_rows, n_rows, s, plan, st)) return rc;
    for (const Schedule::Group &g : s.groups) st[10] += g.variant == kCountsKey;
    st[11] = plan.counts_fwd_levels;
    for (int i = 0; i < n_stats && i < 12; ++i) stats[i] = st[i];
    const int Bv = (int)m->d.cards.size();
    int nb = 0;
    for (size_t f = 0; f < plan.counts_belief_vars.size(); ++f) {
        if (belief_off) belief_off[f] = nb;
        for (int v : plan.counts_belief_vars[f]) {
            if (belief_vars && nb < cap_belief) belief_vars[nb] = v;
            ++nb;
        }
    }
    if (belief_off) belief_off[plan.counts_belief_vars.size()] = nb;
    if (n_belief) *n_belief = nb;
    if (no_b_elim) {
        // B is summed nowhere and enters no composite: a bucket one of whose input TABLES carries B keeps it
        *no_b_elim = 1;
        for (const BucketSpec &b : plan.buckets) {
            if (b.counts || b.cond_batch) continue;
            bool carries = false;
            for (const View &v : b.in)
                if (v.table >= plan.n_src) {
                    const std::vector<int> &tv = plan.msgs[v.table - plan.n_src].vars;
                    carries = carries || std::find(tv.begin(), tv.end(), Bv) != tv.end();
                }
            if (b.elim_var == Bv || (carries && std::find(b.out_vars.begin(), b.out_vars.end(), Bv) == b.out_vars.end()))
                *no_b_elim = 0;
        }
    }
    report_evidence_factors(plan, n_ev, mask_factor, n_soft, lam_factor);
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_plan_counts_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial,
                        int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                        double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *belief_off,
                        int *belief_vars, int cap_belief, int *n_belief, int *no_b_elim, int *mask_factor) {
    return bnpp_plan_counts_sv(m, n_ev, ev_vars, partial, 0, nullptr, nullptr, heuristic, order, n_order, dtype, rows_per_launch, stats, n_stats, rows, cap_rows, n_rows, belief_off, belief_vars, cap_belief, n_belief, no_b_elim, mask_factor, nullptr);
}

int bnpp_plan_counts(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order, int n_order,
                     int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows, int cap_rows,
                     int *n_rows, int *belief_off, int *belief_vars, int cap_belief, int *n_belief, int *no_b_elim) {
    return bnpp_plan_counts_mv(m, n_ev, ev_vars, nullptr, heuristic, order, n_order, dtype, rows_per_launch, stats,
                               n_stats, rows, cap_rows, n_rows, belief_off, belief_vars, cap_belief, n_belief,
                               no_b_elim, nullptr);
}

int bnpp_bucket_counts(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *table,
                       int n_scope, const int *scope, int n_ev, const int *ev_vars, int64_t n_rows, int64_t rows_live,
                       const int32_t *ev, const double *weights, const void *valid, int has_b, double *acc) {
    BNPP_GUARD_BEGIN
    if (!ctx || !cards || !table || !acc || (n_ev > 0 && !ev_vars)) return set_err(BNPP_ERR_INVALID, "null argument");
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32");
    if (n_cards < 0 || !valid_scope(n_scope, scope, cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad factor scope");
    if (n_ev < 0 || !valid_scope(n_ev, ev_vars, cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad evidence variables");
    if (n_rows < 1 || n_rows > (int64_t)INT32_MAX) return set_err(BNPP_ERR_INVALID, "n_rows must be in [1, 2^31)");
    if (rows_live < 0 || rows_live > n_rows) return set_err(BNPP_ERR_INVALID, "rows_live must be in [0, n_rows]");
    std::vector<int> cv(cards, cards + n_cards);
    cv.push_back((int)n_rows);                              // the row variable
    BucketSpec b;
    b.counts = true;
    b.counts_scope.assign(scope, scope + n_scope);
    std::vector<int> tv;
    bool any_ev = false;
    for (int j = 0; j < n_scope; ++j) {
        int row = -1;
        for (int e = 0; e < n_ev; ++e)
            if (ev_vars[e] == scope[j]) row = e;
        b.counts_rows.push_back(row);
        if (row < 0) tv.push_back(scope[j]);
        any_ev = any_ev || row >= 0;
    }
    if (any_ev && !ev) return set_err(BNPP_ERR_INVALID, "null argument");
    if (has_b) tv.push_back(n_cards);
    b.in.push_back(natural_view(0, tv, cv));
    b.out_vars = {n_cards};
    b.out_table = 1;
    b.counts_valid_b = true;
    BucketDesc d;
    std::vector<int64_t> pool;
    std::string msg;
    if (!build_desc(b, cv, max_vec_for(dtype), d, pool, &msg)) return set_err(BNPP_ERR_UNSUPPORTED, msg);
    hipError_t e = hipSetDevice(ctx->c.device);
    const size_t need = (size_t)(n_rows * kCountsScratchPerRow);
    if (e == hipSuccess && ctx->c.counts_scratch_cap < need) {
        if (ctx->c.counts_scratch) (void)hipFree(ctx->c.counts_scratch);   // waits for the kernels that use it
        ctx->c.counts_scratch = nullptr;
        ctx->c.counts_scratch_cap = 0;
        e = hipMalloc(&ctx->c.counts_scratch, need);
        if (e == hipSuccess) ctx->c.counts_scratch_cap = need;
    }
    if (e != hipSuccess) return set_err(e == hipErrorOutOfMemory ? BNPP_ERR_OOM : BNPP_ERR_HIP,
                                        std::string("scratch: ") + hipGetErrorString(e));
    CountsArgs a;
    if (!counts_args(pool.data(), n_rows, rows_live, table, ev, weights, valid, acc, ctx->c.counts_scratch, a))
        return set_err(BNPP_ERR_INVALID, "bad accumulate step");
    e = launch_counts(dtype == BNPP_F32, a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_marginals_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik, int heuristic, const int *order,
                            int n_order, int n_targets, const int *targets, int dtype, int64_t rows_per_launch,
                            double *out, double *log10_z, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindMarginalsBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, lik);
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    if (!m) return set_err(BNPP_ERR_INVALID, "null context or model");
    if (int rc = marginals_targets(m->d, n_targets, targets, c.targets)) return rc;
    return run_marginals_batch(ctx, c, out, log10_z, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_marginals_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int heuristic, const int *order,
                            int n_order, int n_targets, const int *targets, int dtype, int64_t rows_per_launch,
                            double *out, double *log10_z, double *uptime_ms) {
    return bnpp_marginals_batch_sv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, partial, 0, nullptr, nullptr, heuristic, order, n_order, n_targets, targets, dtype, rows_per_launch, out, log10_z, uptime_ms);
}

int bnpp_marginals_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals, int heuristic, const int *order, int n_order, int n_targets,
                         const int *targets, int dtype, int64_t rows_per_launch, double *out, double *log10_z,
                         double *uptime_ms) {
    return bnpp_marginals_batch_mv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, nullptr, heuristic, order, n_order,
                                   n_targets, targets, dtype, rows_per_launch, out, log10_z, uptime_ms);
}

int bnpp_plan_marginals_batch_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik,
                                 int heuristic, const int *order, int n_order, int n_targets, const int *targets,
                                 int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows,
                                 int cap_rows, int *n_rows, int *col_kind, int *mask_factor, int *lam_factor) {
    BNPP_GUARD_BEGIN
    Schedule s;
    VEPlan plan;
    double st[BNPP_PLAN_MARGINALS_BATCH_STATS] = {0};
    BatchCall c = batch_call(m, kKindMarginalsBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, lik);
    if (!m) return set_err(BNPP_ERR_INVALID, "null argument");
    if (int rc = marginals_targets(m->d, n_targets, targets, c.targets)) return rc;
    if (int rc = plan_batch_entry(c, false, stats, n_stats, rows, cap_rows, n_rows, s, plan, st)) return rc;
    for (const Schedule::Group &g : s.groups) st[10] += g.variant == kMargRowsKey;
    st[11] = plan.counts_fwd_levels;
    st[12] = plan.n_marg_belief;
    st[13] = plan.n_marg_ev;
    st[14] = plan.n_marg_free;
    st[15] = (double)plan.marg_width;
    st[16] = (double)plan.marg_out_bytes;
    st[17] = plan.n_marg_belief_b;
    for (int i = 0; i < n_stats && i < BNPP_PLAN_MARGINALS_BATCH_STATS; ++i) stats[i] = st[i];
    if (col_kind)
        for (const BucketSpec &b : plan.buckets)
            for (size_t j = 0; b.marg_rows && j < b.marg_cols.size(); ++j)
                col_kind[j] = b.marg_cols[j].table >= 0 ? (b.marg_cols[j].has_b ? 1 : 0) : b.marg_cols[j].ev_row >= 0 ? -1 : -2;
    report_evidence_factors(plan, n_ev, mask_factor, n_soft, lam_factor);
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_plan_marginals_batch_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial,
                                 int heuristic, const int *order, int n_order, int n_targets, const int *targets,
                                 int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows,
                                 int cap_rows, int *n_rows, int *col_kind, int *mask_factor) {
    return bnpp_plan_marginals_batch_sv(m, n_ev, ev_vars, partial, 0, nullptr, nullptr, heuristic, order, n_order, n_targets, targets, dtype, rows_per_launch, stats, n_stats, rows, cap_rows, n_rows, col_kind, mask_factor, nullptr);
}

int bnpp_plan_marginals_batch(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order,
                              int n_order, int n_targets, const int *targets, int dtype, int64_t rows_per_launch,
                              double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *col_kind) {
    return bnpp_plan_marginals_batch_mv(m, n_ev, ev_vars, nullptr, heuristic, order, n_order, n_targets, targets,
                                        dtype, rows_per_launch, stats, n_stats, rows, cap_rows, n_rows, col_kind,
                                        nullptr);
}

int bnpp_bucket_marginal_rows(bnpp_ctx *ctx, void *stream, int dtype, int n_targets, const int *cards,
                              const void *const *tables, const int *has_b, const int *ev_row, int64_t n_rows,
                              int64_t rows_live, const int32_t *ev, double *out) {
    BNPP_GUARD_BEGIN
    // the shape is checked before the context is looked at
    if (!cards || !tables || !has_b || !ev_row || !out) return set_err(BNPP_ERR_INVALID, "null argument");
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32");
    if (n_targets < 1) return set_err(BNPP_ERR_INVALID, "n_targets must be at least 1");
    if (n_rows < 1 || n_rows > (int64_t)INT32_MAX) return set_err(BNPP_ERR_INVALID, "n_rows must be in [1, 2^31)");
    if (rows_live < 0 || rows_live > n_rows) return set_err(BNPP_ERR_INVALID, "rows_live must be in [0, n_rows]");
    for (int j = 0; j < n_targets; ++j) {
        if (cards[j] < 1) return set_err(BNPP_ERR_INVALID, "target " + std::to_string(j) + ": the card must be at least 1");
        if (!tables[j] && ev_row[j] < 0 && has_b[j])
            return set_err(BNPP_ERR_INVALID, "target " + std::to_string(j) + ": has_b without a table");
        if (!tables[j] && ev_row[j] >= 0 && !ev)
            return set_err(BNPP_ERR_INVALID, "target " + std::to_string(j) + ": an evidence row without the evidence table");
    }
    if (n_targets > kMargRowsSingleMax)
        return set_err(BNPP_ERR_UNSUPPORTED, "at most " + std::to_string(kMargRowsSingleMax) + " targets per call");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    MargRowsSingleArgs a;
    std::memset(&a, 0, sizeof a);
    int64_t W = 0;
    for (int j = 0; j < n_targets; ++j) {
        int64_t *w = a.words + kMargRowsPoolHead + kMargRowsColWords * j;
        w[0] = (int64_t)reinterpret_cast<uintptr_t>(tables[j]);
        w[1] = cards[j];
        w[2] = tables[j] && has_b[j] ? 1 : 0;
        w[3] = tables[j] ? -1 : ev_row[j] >= 0 ? ev_row[j] : -1;
        w[4] = W;
        W += cards[j];
    }
    a.words[0] = n_targets;
    a.words[1] = n_rows;
    a.words[2] = W;
    a.words[3] = -1;
    a.ev = ev;
    a.out = out;
    a.rows_live = rows_live;
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_marg_rows_single(dtype == BNPP_F32, a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_partition_batch_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int32_t *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
                            const void *lik, int lik_dtype, int heuristic, const int *order, int n_order, int dtype,
                            int64_t rows_per_launch, double *log10_z, double *z, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch, partial,
                             n_soft, soft_vars, static_cast<const double *>(lik));
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    c.target = -1;
    DvIo io;
    io.lik_dtype = lik_dtype;
    io.log10_z = log10_z;
    io.z = z;
    return run_batch_dv(ctx, kDvPartition, c, io, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_marginals_batch_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int32_t *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
                            const void *lik, int lik_dtype, int heuristic, const int *order, int n_order,
                            int n_targets, const int *targets, int dtype, int64_t rows_per_launch, double *out,
                            double *log10_z, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindMarginalsBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, static_cast<const double *>(lik));
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    if (!m) return set_err(BNPP_ERR_INVALID, "null context or model");
    if (int rc = marginals_targets(m->d, n_targets, targets, c.targets)) return rc;
    DvIo io;
    io.lik_dtype = lik_dtype;
    io.out = out;
    io.log10_z = log10_z;
    return run_batch_dv(ctx, kDvMarginals, c, io, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_mpe_batch_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                      const int32_t *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
                      const void *lik, int lik_dtype, int heuristic, const int *order, int n_order, int dtype,
                      int64_t rows_per_launch, double *log10_value, int32_t *assignment, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindMpeBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch, partial,
                             n_soft, soft_vars, static_cast<const double *>(lik));
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    DvIo io;
    io.lik_dtype = lik_dtype;
    io.log10_z = log10_value;
    io.assignment = assignment;
    return run_batch_dv(ctx, kDvMpe, c, io, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_sample_batch_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int32_t *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
                         const void *lik, int lik_dtype, int heuristic, const int *order, int n_order, int dtype,
                         int64_t rows_per_launch, int64_t n_per_row, int64_t first_sample, int64_t row_stride,
                         uint64_t seed, uint8_t *out, double *log10_z, int64_t *n_degenerate, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindSampleBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, static_cast<const double *>(lik));
    c.K = n_per_row;
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    DvIo io;
    io.lik_dtype = lik_dtype;
    io.samples = out;
    io.log10_z = log10_z;
    io.n_degenerate = n_degenerate;
    io.first_sample = first_sample;
    io.row_stride = row_stride;
    io.seed = seed;
    return run_batch_dv(ctx, kDvSample, c, io, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_log_partition_dv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                          const int32_t *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
                          const void *loglik, int lik_dtype, int heuristic, const int *order, int n_order, int dtype,
                          int64_t rows_per_launch, double *ln_z, double *post, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    // post: the batched-marginals plan with the soft variables as targets (marginals_batch's job on them), ln_z
    // from its result table; no post, or nothing soft: the batch plan (partition_batch's job)
    const bool with_post = post && n_soft > 0;
    BatchCall c = batch_call(m, with_post ? kKindMarginalsBatch : kKindBatch, n_ev, ev_vars, heuristic, order, n_order,
                             dtype, rows_per_launch, partial, n_soft, soft_vars, static_cast<const double *>(loglik));
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    if (!with_post) c.target = -1;
    DvIo io;
    io.lik_dtype = lik_dtype;
    io.log_only = true;
    io.ln_z = ln_z;
    if (!m) return set_err(BNPP_ERR_INVALID, "null context or model");
    if (n_rows < 1) return set_err(BNPP_ERR_INVALID, "n_rows must be at least 1");
    if (!ln_z) return set_err(BNPP_ERR_INVALID, "null output");
    if (with_post) {
        if (int rc = batch_check_rows_dv(c, lik_dtype, true)) return rc;   // the soft variables, before they are targets
        if (int rc = marginals_targets(m->d, n_soft, soft_vars, c.targets)) return rc;
        io.out = post;
    }
    return run_batch_dv(ctx, with_post ? kDvMarginals : kDvPartition, c, io, uptime_ms);
    BNPP_GUARD_END
}

// ---- device-resident model tables: bnpp_tables, bnpp_expected_counts_dv, bnpp_mstep_dv (tables.cuh) ----

static int tables_check_dtypes(int dtype, int values_dtype) {
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32");
    if (values_dtype < 0 || values_dtype > (BNPP_F32 | BNPP_LIK_LOG))
        return set_err(BNPP_ERR_INVALID, "values_dtype must be BNPP_F64 or BNPP_F32, alone or with BNPP_LIK_LOG");
    return BNPP_OK;
}

int bnpp_tables_create(bnpp_ctx *ctx, const bnpp_model *m, int dtype, bnpp_tables **out) {
    BNPP_GUARD_BEGIN
    if (!out) return set_err(BNPP_ERR_INVALID, "null output");
    *out = nullptr;
    if (!m) return set_err(BNPP_ERR_INVALID, "null model");
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "bad dtype");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    std::unique_ptr<bnpp_tables> t(new bnpp_tables);
    t->ctx = ctx;
    t->model_uid = m->uid;
    t->dtype = dtype;
    Context *c = &ctx->c;
    t->src = std::shared_ptr<DeviceSources>(new DeviceSources, [c](DeviceSources *p) {
        free_sources(*c, *p);
        delete p;
    });
    // the layout, and the model's own values in it, are upload_sources'
    if (int rc = upload_sources(ctx->c, m->d.values, dtype == BNPP_F32 ? kF32 : kF64, *t->src)) return from_ctx(ctx, rc);
    const size_t n = m->d.values.size();
    std::vector<int64_t> words(3 * n + 1, 0);
    for (size_t f = 0; f < n; ++f) {
        words[3 * f] = t->total;
        words[3 * f + 1] = (int64_t)m->d.values[f].size();
        words[3 * f + 2] = static_cast<unsigned char *>(t->src->meta[f].ptr) - static_cast<unsigned char *>(t->src->buf);
        t->sizes.push_back((int64_t)m->d.values[f].size());
        t->total += (int64_t)m->d.values[f].size();
    }
    const size_t meta_b = n * sizeof(TableMeta), shift_b = (1 + n) * sizeof(double), words_b = words.size() * sizeof(int64_t);
    hipError_t e = get_buffer(ctx->c, meta_b + shift_b + words_b + sizeof(int64_t), &t->block, &t->block_cap);
    if (e != hipSuccess)
        return set_err(e == hipErrorOutOfMemory ? BNPP_ERR_OOM : BNPP_ERR_HIP, std::string("tables: ") + hipGetErrorString(e));
    char *base = static_cast<char *>(t->block);
    t->d_meta = reinterpret_cast<TableMeta *>(base);
    t->d_shift = reinterpret_cast<double *>(base + meta_b);
    t->d_words = reinterpret_cast<int64_t *>(base + meta_b + shift_b);
    t->d_status = reinterpret_cast<int64_t *>(base + meta_b + shift_b + words_b);
    if (meta_b) e = hipMemcpy(t->d_meta, t->src->meta.data(), meta_b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(t->d_shift, 0, shift_b);
    if (e == hipSuccess) e = hipMemcpy(t->d_words, words.data(), words_b, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        put_buffer(ctx->c, t->block, t->block_cap);
        return set_err(BNPP_ERR_HIP, std::string("tables: ") + hipGetErrorString(e));
    }
    {
        std::lock_guard<std::mutex> g(g_tables_mu);
        g_tables.push_back(t.get());
    }
    *out = t.release();
    return BNPP_OK;
    BNPP_GUARD_END
}

// what a table set holds of its context goes back to it (the caller holds g_tables_mu and has set the device)
static void tables_release(bnpp_tables *t) {
    put_buffer(t->ctx->c, t->block, t->block_cap);
    t->block = nullptr;
    t->src.reset();                                         // its deleter hands the buffer to the context
    t->ctx = nullptr;
}

int bnpp_tables_free(bnpp_tables *t) {
    if (!t) return BNPP_OK;
    std::lock_guard<std::mutex> g(g_tables_mu);             // against the context's destruction on another thread
    g_tables.erase(std::remove(g_tables.begin(), g_tables.end(), t), g_tables.end());
    bnpp_ctx *ctx = t->ctx;
    if (!ctx) {                                             // its context is gone, and took the buffers with it
        delete t;
        return BNPP_OK;
    }
    int dev = -1;
    const bool had = hipGetDevice(&dev) == hipSuccess;
    (void)hipSetDevice(ctx->c.device);
    {
        // a cached job planned for these tables reads their buffer: it goes first (as bnpp_model_free's)
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        if (ctx->job_cached && ctx->job_cached->tables_uid == t->uid) evict_cached_job(ctx);
    }
    (void)hipStreamSynchronize(ctx->c.stream);              // a staging step may still write the block
    tables_release(t);
    if (had) (void)hipSetDevice(dev);
    delete t;
    return BNPP_OK;
}

int bnpp_tables_set_dv(bnpp_tables *t, const void *values, int values_dtype) {
    BNPP_GUARD_BEGIN
    if (!t) return set_err(BNPP_ERR_INVALID, "null tables");
    if (!values && t->total > 0) return set_err(BNPP_ERR_INVALID, "null values");
    if (int rc = tables_check_dtypes(t->dtype, values_dtype)) return rc;
    bnpp_ctx *ctx = t->ctx;
    if (!ctx) return set_err(BNPP_ERR_INVALID, "the tables' context has been destroyed");
    const bool log_form = (values_dtype & BNPP_LIK_LOG) != 0;
    static const int64_t kClear = INT64_MAX;
    StageTablesSingle a;
    std::memset(&a, 0, sizeof a);
    a.a = StageTablesArgs{t->d_words, values, t->src->buf, t->d_meta, t->d_shift, t->d_status, (int64_t)t->sizes.size(),
                          (values_dtype & BNPP_F32) != 0, t->dtype == BNPP_F32};
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_status, &kClear, sizeof kClear, hipMemcpyHostToDevice, ctx->c.stream);
    if (e == hipSuccess) e = launch_stage_tables(a, log_form, ctx->c.max_grid, ctx->c.stream);
    if (e == hipSuccess) t->log_form = log_form;           // the buffer holds that form from here on, invalid entries as 0
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->c.stream);
    int64_t st = INT64_MAX;
    if (e == hipSuccess) e = hipMemcpy(&st, t->d_status, sizeof st, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("bnpp_tables_set_dv: ") + hipGetErrorString(e));
    if (st != INT64_MAX) {
        size_t f = 0;
        while (f + 1 < t->sizes.size() && st >= t->sizes[f]) st -= t->sizes[f++];
        return set_err(BNPP_ERR_INVALID, "factor " + std::to_string(f) + ": entry " + std::to_string(st) +
                                             (log_form ? " must not be NaN or +inf" : " must be finite and not negative"));
    }
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_stage_tables(bnpp_ctx *ctx, void *stream, int dtype, int values_dtype, int n_factors, const int64_t *sizes,
                      const void *values, void *out_buf, void *out_meta, double *out_shift, int64_t *status) {
    BNPP_GUARD_BEGIN
    if (n_factors < 0 || (n_factors > 0 && (!sizes || !values || !out_buf || !out_meta)) || !out_shift || !status)
        return set_err(BNPP_ERR_INVALID, "null argument");
    if (int rc = tables_check_dtypes(dtype, values_dtype)) return rc;
    for (int f = 0; f < n_factors; ++f)
        if (sizes[f] < 1) return set_err(BNPP_ERR_INVALID, "factor " + std::to_string(f) + ": the size must be at least 1");
    if (n_factors > kTablesSingleMax)
        return set_err(BNPP_ERR_UNSUPPORTED, "at most " + std::to_string(kTablesSingleMax) + " factors per call");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    StageTablesSingle a;
    std::memset(&a, 0, sizeof a);
    const int64_t eb = dtype == BNPP_F32 ? 4 : 8;
    int64_t in0 = 0, out_off = 0;
    for (int f = 0; f < n_factors; ++f) {                   // upload_sources' offsets: every factor on a 256-byte line
        a.single[3 * f] = in0;
        a.single[3 * f + 1] = sizes[f];
        a.single[3 * f + 2] = out_off;
        in0 += sizes[f];
        out_off += (sizes[f] * eb + 255) / 256 * 256;
    }
    a.a = StageTablesArgs{nullptr, values, out_buf, static_cast<TableMeta *>(out_meta), out_shift, status, n_factors,
                          (values_dtype & BNPP_F32) != 0, dtype == BNPP_F32};
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess)
        e = launch_stage_tables(a, (values_dtype & BNPP_LIK_LOG) != 0, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_expected_counts_dv(bnpp_ctx *ctx, const bnpp_model *m, const bnpp_tables *tables, int n_ev, const int *ev_vars,
                            int64_t n_rows, const int32_t *ev_vals, const unsigned char *partial, int n_soft,
                            const int *soft_vars, const void *lik, int lik_dtype, const double *weights, int flags,
                            int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                            double *counts, double *log10_z, double *ln_z, int64_t *n_impossible, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    // counts: the counts plan (the job and key of bnpp_expected_counts_sv); none: the batch plan (those of
    // bnpp_partition_batch_dv), the likelihood of the rows under the tables without the backward pass
    BatchCall c = batch_call(m, counts ? kKindCounts : kKindBatch, n_ev, ev_vars, heuristic, order, n_order, dtype,
                             rows_per_launch, partial, n_soft, soft_vars, static_cast<const double *>(lik));
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    c.tables = tables;
    if (!counts) c.target = -1;
    DvIo io;
    io.lik_dtype = lik_dtype;
    io.log10_z = log10_z;
    io.ln_z = ln_z;
    io.weights = weights;
    io.counts = counts;
    io.accumulate = (flags & BNPP_COUNTS_ACCUMULATE) != 0;
    io.n_impossible = n_impossible;
    if (!m) return set_err(BNPP_ERR_INVALID, "null context or model");
    if (n_rows < 1) return set_err(BNPP_ERR_INVALID, "n_rows must be at least 1");
    if (flags & ~BNPP_COUNTS_ACCUMULATE) return set_err(BNPP_ERR_INVALID, "bad flags");
    return run_batch_dv(ctx, counts ? kDvCounts : kDvPartition, c, io, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_mstep_dv(bnpp_ctx *ctx, void *stream, const bnpp_model *m, const double *counts, double prior,
                  const double *old_values, double *new_values) {
    BNPP_GUARD_BEGIN
    if (!m) return set_err(BNPP_ERR_INVALID, "null model");
    if (!counts || !old_values || !new_values) return set_err(BNPP_ERR_INVALID, "null argument");
    if (!(prior >= 0) || !std::isfinite(prior)) return set_err(BNPP_ERR_INVALID, "the prior must be finite and not negative");
    if (!m->d.is_bayes)
        return set_err(BNPP_ERR_UNSUPPORTED, "the M step fits the CPTs of a BAYES model; Markov networks need iterative fitting");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    const ModelData &d = m->d;
    const int64_t n = (int64_t)d.values.size();
    hipError_t e = hipSetDevice(ctx->c.device);
    std::lock_guard<std::mutex> g(ctx->mstep_mu);
    if (e == hipSuccess && ctx->mstep_uid != m->uid) {
        // per factor its first entry, k and first parent configuration: kept for the model (read-only, its uid never
        // reused), so a training loop uploads them once.  An earlier M step may still read the old words
        std::vector<int64_t> words((size_t)(3 * n + 1), 0);
        int64_t at = 0, cfg = 0;
        for (int64_t f = 0; f < n; ++f) {
            const int64_t k = d.scopes[(size_t)f].empty() ? 1 : d.cards[d.scopes[(size_t)f].back()];
            words[(size_t)(3 * f)] = at;
            words[(size_t)(3 * f + 1)] = k;
            words[(size_t)(3 * f + 2)] = cfg;
            at += (int64_t)d.values[(size_t)f].size();
            cfg += (int64_t)d.values[(size_t)f].size() / k;
        }
        words[(size_t)(3 * n)] = cfg;
        if (ctx->mstep_launched) e = hipStreamSynchronize(ctx->mstep_stream);
        if (e == hipSuccess && ctx->mstep_cap < words.size() * sizeof(int64_t)) {
            put_buffer(ctx->c, ctx->mstep_words, ctx->mstep_cap);
            ctx->mstep_words = nullptr;
            ctx->mstep_cap = 0;
            e = get_buffer(ctx->c, words.size() * sizeof(int64_t), &ctx->mstep_words, &ctx->mstep_cap);
        }
        if (e == hipSuccess) e = hipMemcpy(ctx->mstep_words, words.data(), words.size() * sizeof(int64_t), hipMemcpyHostToDevice);
        ctx->mstep_uid = e == hipSuccess ? m->uid : 0;
        ctx->mstep_cfg = cfg;
    }
    if (e == hipSuccess) {
        const MstepArgs a{static_cast<const int64_t *>(ctx->mstep_words), counts, old_values, new_values, prior, n};
        e = launch_mstep(a, ctx->mstep_cfg, ctx->c.max_grid, pick_stream(ctx, stream));
        ctx->mstep_stream = pick_stream(ctx, stream);
        ctx->mstep_launched = true;
    }
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("bnpp_mstep_dv: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

// the launch window of a single-step call: checked before the context is looked at
static int rowio_check_window(int64_t n_rows, int64_t row0, int64_t R) {
    if (n_rows < 1) return set_err(BNPP_ERR_INVALID, "n_rows must be at least 1");
    if (R < 1 || R > (int64_t)INT32_MAX) return set_err(BNPP_ERR_INVALID, "R must be in [1, 2^31)");
    if (row0 < 0 || row0 >= n_rows) return set_err(BNPP_ERR_INVALID, "row0 must be in [0, n_rows)");
    return BNPP_OK;
}

int bnpp_stage_evidence_rows(bnpp_ctx *ctx, void *stream, int n_ev, const int *cards, const unsigned char *partial,
                             int64_t n_rows, int64_t row0, int64_t R, const int32_t *ev, int32_t *out,
                             int64_t *status) {
    BNPP_GUARD_BEGIN
    if (n_ev < 0 || (n_ev > 0 && (!cards || !ev || !out)) || !status) return set_err(BNPP_ERR_INVALID, "null argument");
    if (int rc = rowio_check_window(n_rows, row0, R)) return rc;
    for (int j = 0; j < n_ev; ++j)
        if (cards[j] < 1) return set_err(BNPP_ERR_INVALID, "column " + std::to_string(j) + ": the card must be at least 1");
    if (n_ev > kRowioSingleMax)
        return set_err(BNPP_ERR_UNSUPPORTED, "at most " + std::to_string(kRowioSingleMax) + " columns per call");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    RowioSingle<StageRowsArgs> a;
    std::memset(&a, 0, sizeof a);
    for (int j = 0; j < n_ev; ++j) a.single[j] = (int64_t)cards[j] | ((int64_t)(partial && partial[j] ? 1 : 0) << 32);
    a.a = StageRowsArgs{nullptr, ev, out, status, n_rows, row0, R, n_ev};
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_stage_rows(a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_stage_likelihoods(bnpp_ctx *ctx, void *stream, int dtype, int lik_dtype, int n_soft, const int *cards,
                           int64_t n_rows, int64_t row0, int64_t R, const void *lik, void *out, int64_t *e_row,
                           int64_t *status) {
    BNPP_GUARD_BEGIN
    if (n_soft < 0 || (n_soft > 0 && (!cards || !lik || !out)) || !e_row || !status)
        return set_err(BNPP_ERR_INVALID, "null argument");
    if ((dtype != BNPP_F32 && dtype != BNPP_F64) || (lik_dtype != BNPP_F32 && lik_dtype != BNPP_F64))
        return set_err(BNPP_ERR_INVALID, "dtype and lik_dtype must be BNPP_F64 or BNPP_F32");
    if (int rc = rowio_check_window(n_rows, row0, R)) return rc;
    for (int i = 0; i < n_soft; ++i)
        if (cards[i] < 1) return set_err(BNPP_ERR_INVALID, "variable " + std::to_string(i) + ": the card must be at least 1");
    if (n_soft > kRowioSingleMax)
        return set_err(BNPP_ERR_UNSUPPORTED, "at most " + std::to_string(kRowioSingleMax) + " variables per call");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    RowioSingle<StageLikArgs> a;
    std::memset(&a, 0, sizeof a);
    int64_t ws = 0;
    for (int i = 0; i < n_soft; ++i) {
        a.single[i] = (int64_t)cards[i] | (ws << 32);
        ws += cards[i];
    }
    a.a = StageLikArgs{nullptr, lik, out, e_row, status, n_rows, row0, R, ws, n_soft, lik_dtype == BNPP_F32, dtype == BNPP_F32,
                       nullptr};
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_stage_lik(a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_stage_loglikelihoods(bnpp_ctx *ctx, void *stream, int dtype, int lik_dtype, int n_soft, const int *cards,
                              int64_t n_rows, int64_t row0, int64_t R, const void *loglik, void *out, int64_t *e_row,
                              double *top, int64_t *status) {
    BNPP_GUARD_BEGIN
    if (n_soft < 0 || (n_soft > 0 && (!cards || !loglik || !out || !top)) || !e_row || !status)
        return set_err(BNPP_ERR_INVALID, "null argument");
    if ((dtype != BNPP_F32 && dtype != BNPP_F64) ||
        (lik_dtype != (BNPP_F32 | BNPP_LIK_LOG) && lik_dtype != (BNPP_F64 | BNPP_LIK_LOG)))
        return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32, lik_dtype one of them with BNPP_LIK_LOG");
    if (int rc = rowio_check_window(n_rows, row0, R)) return rc;
    for (int i = 0; i < n_soft; ++i)
        if (cards[i] < 1) return set_err(BNPP_ERR_INVALID, "variable " + std::to_string(i) + ": the card must be at least 1");
    if (n_soft > kRowioSingleMax)
        return set_err(BNPP_ERR_UNSUPPORTED, "at most " + std::to_string(kRowioSingleMax) + " variables per call");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    RowioSingle<StageLikArgs> a;
    std::memset(&a, 0, sizeof a);
    int64_t ws = 0;
    for (int i = 0; i < n_soft; ++i) {
        a.single[i] = (int64_t)cards[i] | (ws << 32);
        ws += cards[i];
    }
    a.a = StageLikArgs{nullptr, loglik, out, e_row, status, n_rows, row0, R, ws, n_soft, (lik_dtype & BNPP_F32) != 0,
                       dtype == BNPP_F32, top};
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_stage_loglik(a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_emit_row_scalars(bnpp_ctx *ctx, void *stream, int dtype, const void *table, int has_b, const void *meta,
                          const int64_t *e_row, int64_t row0, int64_t rows_live, double *log10_z, double *z) {
    BNPP_GUARD_BEGIN
    if (!log10_z) return set_err(BNPP_ERR_INVALID, "null output");
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32");
    if (row0 < 0 || rows_live < 0) return set_err(BNPP_ERR_INVALID, "row0 and rows_live must be at least 0");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    const EmitScalarsArgs a{table, static_cast<const TableMeta *>(meta), e_row, log10_z, z, row0, rows_live,
                            dtype == BNPP_F32, table && has_b, nullptr, nullptr, 0, 0, nullptr, nullptr};
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_emit_scalars(a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_emit_row_logs(bnpp_ctx *ctx, void *stream, int dtype, const void *table, int has_b, const void *meta,
                       const int64_t *e_row, int n_soft, const double *top, int64_t R, int64_t row0, int64_t rows_live,
                       double *ln_z, double *log10_z, double *z) {
    BNPP_GUARD_BEGIN
    if (!ln_z && !log10_z && !z) return set_err(BNPP_ERR_INVALID, "null output");
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32");
    if (n_soft < 0 || (n_soft > 0 && !top)) return set_err(BNPP_ERR_INVALID, "null argument");
    if (R < 1 || R > (int64_t)INT32_MAX) return set_err(BNPP_ERR_INVALID, "R must be in [1, 2^31)");
    if (row0 < 0 || rows_live < 0 || rows_live > R) return set_err(BNPP_ERR_INVALID, "row0 must be at least 0 and rows_live in [0, R]");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    const EmitScalarsArgs a{table, static_cast<const TableMeta *>(meta), e_row, log10_z, z, row0, rows_live,
                            dtype == BNPP_F32, table && has_b, top, ln_z, n_soft, R, nullptr, nullptr};
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_emit_logs(a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_emit_row_states(bnpp_ctx *ctx, void *stream, int sampling, int n_vars, const int *ev_col,
                         const unsigned char *written, int64_t K, int64_t R, int64_t row0, int64_t rows_live,
                         const uint8_t *x, const int32_t *ev, int dtype, const void *table, int has_b,
                         const uint64_t *deg, int64_t n_drawn, void *out, int64_t *n_degenerate) {
    BNPP_GUARD_BEGIN
    if (!ev_col || !written || !x) return set_err(BNPP_ERR_INVALID, "null argument");
    if (!out && !(sampling && n_degenerate)) return set_err(BNPP_ERR_INVALID, "null output");
    if (n_vars < 1) return set_err(BNPP_ERR_INVALID, "n_vars must be at least 1");
    if (sampling ? K < 1 : K != 1) return set_err(BNPP_ERR_INVALID, sampling ? "K must be at least 1" : "K must be 1 without sampling");
    if (R < 1 || R > (int64_t)INT32_MAX) return set_err(BNPP_ERR_INVALID, "R must be in [1, 2^31)");
    if (row0 < 0 || rows_live < 0 || rows_live > R) return set_err(BNPP_ERR_INVALID, "row0 must be at least 0 and rows_live in [0, R]");
    if (sampling && dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32");
    if (sampling && n_degenerate && !deg) return set_err(BNPP_ERR_INVALID, "n_degenerate without the draw step's counters");
    for (int v = 0; v < n_vars; ++v)
        if (ev_col[v] >= 0 && !ev) return set_err(BNPP_ERR_INVALID, "variable " + std::to_string(v) + ": an evidence column without the evidence table");
    if (n_vars > kRowioSingleMax)
        return set_err(BNPP_ERR_UNSUPPORTED, "at most " + std::to_string(kRowioSingleMax) + " variables per call");
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    RowioSingle<EmitStatesArgs> a;
    std::memset(&a, 0, sizeof a);
    for (int v = 0; v < n_vars; ++v)
        a.single[v] = (int64_t)(uint32_t)(ev_col[v] >= 0 ? ev_col[v] : -1) | ((int64_t)(written[v] ? 1 : 0) << 33);
    a.a = EmitStatesArgs{nullptr, x, ev, sampling ? table : nullptr, reinterpret_cast<const unsigned long long *>(deg), out,
                         sampling ? n_degenerate : nullptr, n_vars, K, R, row0, rows_live, n_drawn, sampling != 0,
                         dtype == BNPP_F32, table && has_b, 0};
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_emit_states(a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

const char *bnpp_strerror(int status) {
    switch (status) {
        case BNPP_OK: return "ok";
        case BNPP_ERR_INVALID: return "invalid argument or shape";
        case BNPP_ERR_NO_DEVICE: return "no usable GPU device";
        case BNPP_ERR_OOM: return "out of memory";
        case BNPP_ERR_HIP: return "HIP runtime error";
        case BNPP_ERR_IO: return "cannot read or parse file";
        case BNPP_ERR_UNSUPPORTED: return "unsupported shape";
        default: return "unknown status";
    }
}

const char *bnpp_last_error(void) { return g_err.c_str(); }

int bnpp_last_timing(double *out, int n) {
    if (!out || n < 0) return set_err(BNPP_ERR_INVALID, "null output");
    for (int i = 0; i < n && i < kTimingPhases; ++i) out[i] = g_timing[i];
    return BNPP_OK;
}
int bnpp_version(void) { return BNPP_VERSION; }

int bnpp_device_count(int *n) {
    if (!n) return set_err(BNPP_ERR_INVALID, "null output");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = e == hipSuccess ? c : 0;
    return BNPP_OK;
}

int bnpp_ctx_create(int device, bnpp_ctx **out) {
    BNPP_GUARD_BEGIN
    if (!out) return set_err(BNPP_ERR_INVALID, "null output");
    *out = nullptr;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c <= 0) return set_err(BNPP_ERR_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= c) return set_err(BNPP_ERR_NO_DEVICE, "device index out of range");
    if ((e = hipSetDevice(device)) != hipSuccess) return set_err(BNPP_ERR_HIP, hipGetErrorString(e));
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return set_err(BNPP_ERR_HIP, hipGetErrorString(e));
    std::unique_ptr<bnpp_ctx> ctx(new bnpp_ctx);
    ctx->c.device = device;
    int per_cu = 3;          // measured: 3 workgroups per CU beat 4 and 8 on the bench bucket and the 32x32 sweep
    if (const char *g = tuning_knob("BNPP_GRID_PER_CU")) per_cu = std::max(0, std::min(64, std::atoi(g)));
    // 0: flat grid, one virtual block per workgroup (no grid-stride)
    ctx->c.max_grid = per_cu == 0 ? INT32_MAX : prop.multiProcessorCount * per_cu;
    ctx->c.default_max_grid = ctx->c.max_grid;
    if ((e = hipStreamCreateWithFlags(&ctx->c.stream, hipStreamNonBlocking)) != hipSuccess)
        return set_err(BNPP_ERR_HIP, hipGetErrorString(e));
    {
        std::lock_guard<std::mutex> g(g_ctxs_mu);
        g_ctxs.push_back(ctx.get());
    }
    *out = ctx.release();
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_ctx_destroy(bnpp_ctx *ctx) {
    if (!ctx) return BNPP_OK;
    {
        std::lock_guard<std::mutex> g(g_ctxs_mu);
        g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), ctx), g_ctxs.end());
    }
    (void)hipSetDevice(ctx->c.device);
    {
        // a bnpp_model_free on another thread may hold this lock while it
        // evicts the cached job (it collected the context before the erase
        // above): wait for it, so the job is destroyed once and the lock is
        // released before the context is deleted
        std::lock_guard<std::mutex> lk(ctx->cache_mu);
        evict_cached_job(ctx);
    }
    {
        // table sets that outlive the context keep nothing of it: they can still be freed, and nothing else
        std::lock_guard<std::mutex> g(g_tables_mu);
        (void)hipStreamSynchronize(ctx->c.stream);
        for (bnpp_tables *t : g_tables)
            if (t->ctx == ctx) tables_release(t);
    }
    if (ctx->c.stream) (void)hipStreamDestroy(ctx->c.stream);
    if (ctx->c.lane_stream) (void)hipStreamDestroy(ctx->c.lane_stream);
    if (ctx->c.counts_scratch) (void)hipFree(ctx->c.counts_scratch);
    put_buffer(ctx->c, ctx->mstep_words, ctx->mstep_cap);
    ctx->srcs.clear();
    drop_arena_cache(ctx->c);
    drop_buffer_cache(ctx->c);
    delete ctx;
    return BNPP_OK;
}

int bnpp_ctx_set_max_grid(bnpp_ctx *ctx, int n) {
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    if (n < 0) return set_err(BNPP_ERR_INVALID, "negative grid cap");
    // launches read both at enqueue time; plans and cached jobs do not depend on them
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    ctx->c.grid_cap = n;
    ctx->c.max_grid = n > 0 ? std::min(ctx->c.default_max_grid, n) : ctx->c.default_max_grid;
    return BNPP_OK;
}

int bnpp_ctx_trim(bnpp_ctx *ctx) {
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    std::unique_lock<std::mutex> lk(ctx->cache_mu, std::try_to_lock);
    if (!lk.owns_lock()) return set_err(BNPP_ERR_INVALID, "a call on this context is running");
    (void)hipSetDevice(ctx->c.device);
    (void)hipDeviceSynchronize();
    evict_cached_job(ctx);
    {
        std::lock_guard<std::mutex> g(ctx->src_mu);
        ctx->srcs.clear();
    }
    drop_arena_cache(ctx->c);
    drop_buffer_cache(ctx->c);
    return BNPP_OK;
}

int bnpp_ctx_stream(bnpp_ctx *ctx, void **stream) {
    if (!ctx || !stream) return set_err(BNPP_ERR_INVALID, "null argument");
    *stream = ctx->c.stream;
    return BNPP_OK;
}

int bnpp_malloc(bnpp_ctx *ctx, size_t bytes, void **dptr) {
    if (!ctx || !dptr) return set_err(BNPP_ERR_INVALID, "null argument");
    (void)hipSetDevice(ctx->c.device);
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) return set_err(e == hipErrorOutOfMemory ? BNPP_ERR_OOM : BNPP_ERR_HIP, hipGetErrorString(e));
    return BNPP_OK;
}

int bnpp_free(bnpp_ctx *ctx, void *dptr) {
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    (void)hipSetDevice(ctx->c.device);
    hipError_t e = hipFree(dptr);
    return e == hipSuccess ? BNPP_OK : set_err(BNPP_ERR_HIP, hipGetErrorString(e));
}

int bnpp_memcpy_h2d(bnpp_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    (void)hipSetDevice(ctx->c.device);
    hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? BNPP_OK : set_err(BNPP_ERR_HIP, hipGetErrorString(e));
}

int bnpp_memcpy_d2h(bnpp_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    (void)hipSetDevice(ctx->c.device);
    hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? BNPP_OK : set_err(BNPP_ERR_HIP, hipGetErrorString(e));
}

int bnpp_synchronize(bnpp_ctx *ctx, void *stream) {
    if (!ctx) return set_err(BNPP_ERR_INVALID, "null context");
    (void)hipSetDevice(ctx->c.device);
    hipError_t e = hipStreamSynchronize(pick_stream(ctx, stream));
    return e == hipSuccess ? BNPP_OK : set_err(BNPP_ERR_HIP, hipGetErrorString(e));
}

int bnpp_out_scope(int n_in, const int *in_ndims, const int *const *in_vars, int elim_var, int cap,
                   int *out_ndims, int *out_vars) {
    BNPP_GUARD_BEGIN
    if (n_in < 0 || (n_in > 0 && (!in_ndims || !in_vars)) || !out_ndims) return set_err(BNPP_ERR_INVALID, "bad arguments");
    std::vector<int> u;
    for (int i = 0; i < n_in; ++i) {
        std::vector<int> s(in_vars[i], in_vars[i] + in_ndims[i]);
        u = union_scope(u, s);
    }
    if (elim_var >= 0) u = remove_var(u, elim_var);
    *out_ndims = (int)u.size();
    if ((int)u.size() > cap) return set_err(BNPP_ERR_INVALID, "output scope larger than cap");
    std::copy(u.begin(), u.end(), out_vars);
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_bucket_eliminate(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, int n_in,
                          const void *const *in_tables, const int *in_ndims, const int *const *in_vars, int elim_var,
                          void *out_table, int out_ndims, const int *out_vars, double *out_sum) {
    BNPP_GUARD_BEGIN
    if (!ctx || !cards || n_in < 1 || !in_tables || !in_ndims || !in_vars || !out_table)
        return set_err(BNPP_ERR_INVALID, "null argument");
    if (n_in > kMaxIn) return set_err(BNPP_ERR_UNSUPPORTED, "at most 8 inputs per fused call");
    if (n_cards < 0 || elim_var >= n_cards || (out_ndims > 0 && !out_vars))
        return set_err(BNPP_ERR_INVALID, "variable id outside cards[0, n_cards)");
    for (int i = 0; i < n_in; ++i)
        if (!valid_scope(in_ndims[i], in_vars[i], cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad input scope");
    if (!valid_scope(out_ndims, out_vars, cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad output scope");
    std::vector<int> cv(cards, cards + n_cards);
    BucketSpec b;
    std::vector<const void *> ptrs;
    for (int i = 0; i < n_in; ++i) {
        std::vector<int> s(in_vars[i], in_vars[i] + in_ndims[i]);
        b.in.push_back(natural_view(i, s, cv));
        ptrs.push_back(in_tables[i]);
    }
    b.elim_var = elim_var;
    // the output must hold exactly the kept variables (domain.cpp:32-72), in any order
    std::vector<int> u = chain_scope(b.in);
    if (elim_var >= 0) u = remove_var(u, elim_var);
    std::vector<int> ov(out_vars, out_vars + out_ndims), us = u, os = ov;
    std::sort(us.begin(), us.end());
    std::sort(os.begin(), os.end());
    if (us != os) return set_err(BNPP_ERR_INVALID, "output scope must be the union of the inputs minus elim_var");
    b.out_vars = ov;
    b.out_table = n_in;
    if (int rc = seq_sum_supported(out_sum, u.size(), b.in.size())) return rc;
    int rc = run_single(ctx, stream, dtype, cv, b, ptrs, out_table);
    if (rc == BNPP_OK) rc = run_seq_sum(ctx, stream, dtype, cv, b.in, ptrs, u, elim_var, false, out_sum);
    return rc;
    BNPP_GUARD_END
}

int bnpp_bucket_max(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, int n_in,
                    const void *const *in_tables, const int *in_ndims, const int *const *in_vars, int elim_var,
                    void *out_table, int out_ndims, const int *out_vars, uint8_t *out_arg) {
    BNPP_GUARD_BEGIN
    if (!ctx || !in_tables || !out_table) return set_err(BNPP_ERR_INVALID, "null argument");
    BucketSpec b;
    std::vector<int> cv;
    if (int rc = max_single_spec(n_cards, cards, n_in, in_ndims, in_vars, elim_var, out_ndims, out_vars, b, cv)) return rc;
    SingleArgs a;
    if (int rc = plan_single(dtype, cv, b, a)) return rc;
    for (int i = 0; i < n_in; ++i) a.meta[i].ptr = const_cast<void *>(in_tables[i]);
    a.meta[n_in].ptr = out_table;
    a.arg_out = out_arg;
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_max_single(dtype == BNPP_F32, a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_plan_max_single(int dtype, int n_cards, const int *cards, int n_in, const int *in_ndims,
                         const int *const *in_vars, int elim_var, int out_ndims, const int *out_vars, int64_t *info,
                         int n_info) {
    BNPP_GUARD_BEGIN
    if (!info) return set_err(BNPP_ERR_INVALID, "null argument");
    BucketSpec b;
    std::vector<int> cv;
    if (int rc = max_single_spec(n_cards, cards, n_in, in_ndims, in_vars, elim_var, out_ndims, out_vars, b, cv)) return rc;
    SingleArgs a;
    if (int rc = plan_single(dtype, cv, b, a)) return rc;
    const SingleKey sk = max_single_key(dtype == BNPP_F32, a);
    std::vector<int> keys;
    kernel_keys(dtype == BNPP_F32, 0, sk.family, keys);
    const int64_t v[12] = {sk.family, sk.key, a.d.n_in, a.d.k, a.d.v1, a.d.v2, 0, (sk.key & kGenericO32) ? 1 : 0,
                           a.d.n_tiles, a.d.lanes, a.d.slab_y2,
                           std::find(keys.begin(), keys.end(), sk.key) != keys.end() ? 1 : 0};
    for (int i = 0; i < n_info && i < 12; ++i) info[i] = v[i];
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_bucket_sample(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, int n_in,
                       const void *const *in_tables, const int *in_ndims, const int *const *in_vars, int var,
                       int64_t n_samples, int64_t first_sample, uint64_t seed, uint8_t *x, int64_t *n_degenerate) {
    BNPP_GUARD_BEGIN
    if (!ctx || !cards || !x || (n_in > 0 && (!in_tables || !in_ndims || !in_vars)))
        return set_err(BNPP_ERR_INVALID, "null argument");
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32");
    if (n_in < 0) return set_err(BNPP_ERR_INVALID, "negative input count");
    if (n_in > kMaxIn) return set_err(BNPP_ERR_UNSUPPORTED, "at most 8 inputs per fused call");
    if (n_cards < 0 || var < 0 || var >= n_cards || cards[var] < 1)
        return set_err(BNPP_ERR_INVALID, "variable id outside cards[0, n_cards)");
    if (n_samples < 1 || first_sample < 0) return set_err(BNPP_ERR_INVALID, "n_samples must be at least 1, first_sample at least 0");
    for (int i = 0; i < n_in; ++i) {
        if (!valid_scope(in_ndims[i], in_vars[i], cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad input scope");
        if (!in_tables[i]) return set_err(BNPP_ERR_INVALID, "null input table");
        // every variable whose row of x the draw reads or writes holds one byte per value
        for (int j = 0; j < in_ndims[i]; ++j)
            if (cards[in_vars[i][j]] > kMaxOutCard)
                return set_err(BNPP_ERR_UNSUPPORTED, "sampling: a scope variable has more than 256 values (x holds one byte per variable)");
    }
    if (cards[var] > kMaxOutCard)
        return set_err(BNPP_ERR_UNSUPPORTED, "sampling: the sampled variable has more than 256 values (x holds one byte per variable)");
    std::vector<int> cv(cards, cards + n_cards);
    BucketSpec b;
    b.sample = true;
    b.n_samples = n_samples;
    BucketSpec::SampleRow row;
    row.var = var;
    for (int i = 0; i < n_in; ++i) row.in.push_back(natural_view(i, std::vector<int>(in_vars[i], in_vars[i] + in_ndims[i]), cv));
    b.sample_rows.push_back(row);
    BucketDesc d;
    std::vector<int64_t> pool;
    std::string msg;
    if (!build_desc(b, cv, max_vec_for(dtype), d, pool, &msg)) return set_err(BNPP_ERR_INVALID, msg);
    if (pool.size() > (size_t)kMaxPool) return set_err(BNPP_ERR_UNSUPPORTED, "too many scope variables for a single-op call");
    SampleSingleArgs a;
    std::memset(&a, 0, sizeof a);
    std::copy(pool.begin(), pool.end(), a.pool);
    for (int i = 0; i < n_in; ++i) a.meta[i].ptr = const_cast<void *>(in_tables[i]);
    a.x = x;
    a.n = n_samples;
    a.first = first_sample;
    a.seed = seed;
    a.n_degenerate = reinterpret_cast<unsigned long long *>(n_degenerate);
    hipStream_t st = pick_stream(ctx, stream);
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess && n_degenerate) e = hipMemsetAsync(n_degenerate, 0, sizeof(int64_t), st);
    if (e == hipSuccess) e = launch_sample_single(dtype == BNPP_F32, a, ctx->c.max_grid, st);
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_product(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *a, int a_ndims,
                 const int *a_vars, const void *b, int b_ndims, const int *b_vars, void *out, int out_ndims,
                 const int *out_vars, double *out_sum) {
    const void *tabs[2] = {a, b};
    const int nd[2] = {a_ndims, b_ndims};
    const int *vs[2] = {a_vars, b_vars};
    return bnpp_bucket_eliminate(ctx, stream, dtype, n_cards, cards, 2, tabs, nd, vs, -1, out, out_ndims, out_vars,
                                 out_sum);
}

int bnpp_divide(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *a, int a_ndims,
                const int *a_vars, const void *b, int b_ndims, const int *b_vars, void *out, int out_ndims,
                const int *out_vars, double *out_sum) {
    BNPP_GUARD_BEGIN
    if (!ctx || !cards || !a || !b || !out || (a_ndims > 0 && !a_vars) || (b_ndims > 0 && !b_vars) ||
        (out_ndims > 0 && !out_vars))
        return set_err(BNPP_ERR_INVALID, "null argument");
    if (!valid_scope(a_ndims, a_vars, cards, n_cards) || !valid_scope(b_ndims, b_vars, cards, n_cards))
        return set_err(BNPP_ERR_INVALID, "bad input scope");
    if (!valid_scope(out_ndims, out_vars, cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad output scope");
    std::vector<int> cv(cards, cards + n_cards);
    BucketSpec bs;
    bs.in.push_back(natural_view(0, std::vector<int>(a_vars, a_vars + a_ndims), cv));
    bs.in.push_back(natural_view(1, std::vector<int>(b_vars, b_vars + b_ndims), cv));
    std::vector<int> u = chain_scope(bs.in), ov(out_vars, out_vars + out_ndims), us = u, os = ov;
    std::sort(us.begin(), us.end());
    std::sort(os.begin(), os.end());
    if (us != os) return set_err(BNPP_ERR_INVALID, "output scope must be the union of the inputs");
    bs.out_vars = ov;
    bs.out_table = 2;
    bs.divide = true;
    if (int rc = seq_sum_supported(out_sum, u.size(), bs.in.size())) return rc;
    int rc = run_single(ctx, stream, dtype, cv, bs, {a, b}, out);
    if (rc == BNPP_OK) rc = run_seq_sum(ctx, stream, dtype, cv, bs.in, {a, b}, u, -1, true, out_sum);
    return rc;
    BNPP_GUARD_END
}

int bnpp_sum_out(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in, int ndims,
                 const int *vars, int var, void *out, int out_ndims, const int *out_vars, double *out_sum) {
    const void *tabs[1] = {in};
    return bnpp_bucket_eliminate(ctx, stream, dtype, n_cards, cards, 1, tabs, &ndims, &vars, var, out, out_ndims, out_vars,
                                 out_sum);
}

int bnpp_condition(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in, int ndims,
                   const int *vars, int n_ev, const int *ev_vars, const int *ev_vals, void *out, double *out_sum) {
    BNPP_GUARD_BEGIN
    if (!ctx || !cards || !in || !out || (ndims > 0 && !vars) || n_ev < 0 || (n_ev > 0 && (!ev_vars || !ev_vals)))
        return set_err(BNPP_ERR_INVALID, "null argument");
    if (!valid_scope(ndims, vars, cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad scope");
    std::vector<int> cv(cards, cards + n_cards);
    std::vector<int> ev(n_cards, -1);
    std::vector<char> in_scope(n_cards, 0);
    for (int i = 0; i < ndims; ++i) in_scope[vars[i]] = 1;
    for (int i = 0; i < n_ev; ++i) {
        int v = ev_vars[i];
        if (v < 0) return set_err(BNPP_ERR_INVALID, "bad evidence variable");
        // evidence on a variable outside the scope does not touch the factor
        // (Domain(d, ev) looks up scope variables only, domain.cpp:74-90)
        if (v >= n_cards || !in_scope[v]) continue;
        if (ev_vals[i] < 0 || ev_vals[i] >= cv[v]) return set_err(BNPP_ERR_INVALID, "evidence value out of range");
        ev[v] = ev_vals[i];
    }
    std::vector<int> s(vars, vars + ndims);
    BucketSpec b;
    b.in.push_back(conditioned_view(0, s, cv, ev));
    b.out_vars = b.in[0].vars;
    b.out_table = 1;
    if (int rc = seq_sum_supported(out_sum, b.out_vars.size(), b.in.size())) return rc;
    int rc = run_single(ctx, stream, dtype, cv, b, {in}, out);
    if (rc == BNPP_OK) rc = run_seq_sum(ctx, stream, dtype, cv, b.in, {in}, b.out_vars, -1, false, out_sum);
    return rc;
    BNPP_GUARD_END
}

int bnpp_model_load_uai(const char *path, bnpp_model **out) {
    BNPP_GUARD_BEGIN
    if (!path || !out) return set_err(BNPP_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<bnpp_model> m(new bnpp_model);
    std::string err;
    if (load_uai(path, m->d, &err)) return set_err(BNPP_ERR_IO, err);
    *out = m.release();
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_model_from_arrays(int is_bayes, int n_vars, const int *cards, int n_factors, const int *widths,
                           const int *scopes, const double *values, bnpp_model **out) {
    BNPP_GUARD_BEGIN
    if (!out || n_vars < 0 || n_factors < 0 || (n_vars > 0 && !cards) || (n_factors > 0 && (!widths || !scopes || !values)))
        return set_err(BNPP_ERR_INVALID, "bad arguments");
    *out = nullptr;
    std::unique_ptr<bnpp_model> m(new bnpp_model);
    m->d.is_bayes = is_bayes != 0;
    m->d.cards.assign(cards, cards + n_vars);
    for (int c : m->d.cards)
        if (c < 1) return set_err(BNPP_ERR_INVALID, "cardinality must be >= 1");
    const int *sc = scopes;
    const double *vals = values;
    for (int f = 0; f < n_factors; ++f) {
        if (widths[f] < 0) return set_err(BNPP_ERR_INVALID, "negative width");
        std::vector<int> s(sc, sc + widths[f]);
        sc += widths[f];
        int64_t sz = 1;
        for (int v : s) {
            if (v < 0 || v >= n_vars) return set_err(BNPP_ERR_INVALID, "scope id out of range");
            sz *= m->d.cards[v];
        }
        m->d.scopes.push_back(s);
        m->d.values.emplace_back(vals, vals + sz);
        vals += sz;
    }
    std::string err;
    if (!validate(m->d, &err)) return set_err(BNPP_ERR_INVALID, err);
    *out = m.release();
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_model_free(bnpp_model *m) {
    if (!m) return BNPP_OK;
    // every live context drops the model's uploaded sources and a cached
    // one-shot job planned for it (a context in the middle of a call keeps
    // its job until its next one-shot call replaces it)
    // The contexts holding such a job are collected under the context list's
    // lock; their jobs are destroyed after it is released (destroy_job waits
    // for the device: other threads' ctx_create / ctx_destroy / model_free do
    // not wait with it), each under its own context's cache lock, and the
    // caller's current device is restored afterwards.
    std::vector<std::pair<bnpp_ctx *, std::unique_lock<std::mutex>>> evict;
    {
        std::lock_guard<std::mutex> g(g_ctxs_mu);
        for (bnpp_ctx *ctx : g_ctxs) {
            {
                std::lock_guard<std::mutex> gs(ctx->src_mu);
                ctx->srcs.erase(std::remove_if(ctx->srcs.begin(), ctx->srcs.end(),
                                               [&](const bnpp_ctx::Src &e) { return e.uid == m->uid; }),
                                ctx->srcs.end());
            }
            std::unique_lock<std::mutex> lk(ctx->cache_mu, std::try_to_lock);
            if (lk.owns_lock() && ctx->job_cached && ctx->job_cached->model_uid == m->uid)
                evict.emplace_back(ctx, std::move(lk));
        }
    }
    if (!evict.empty()) {
        int dev = -1;
        const bool had = hipGetDevice(&dev) == hipSuccess;
        for (auto &e : evict) evict_cached_job(e.first);
        if (had) (void)hipSetDevice(dev);
    }
    delete m;
    return BNPP_OK;
}

int bnpp_model_info(const bnpp_model *m, int *is_bayes, int *n_vars, int *n_factors) {
    if (!m) return set_err(BNPP_ERR_INVALID, "null model");
    if (is_bayes) *is_bayes = m->d.is_bayes ? 1 : 0;
    if (n_vars) *n_vars = (int)m->d.cards.size();
    if (n_factors) *n_factors = (int)m->d.scopes.size();
    return BNPP_OK;
}

int bnpp_model_cards(const bnpp_model *m, int *cards) {
    if (!m || !cards) return set_err(BNPP_ERR_INVALID, "null argument");
    std::copy(m->d.cards.begin(), m->d.cards.end(), cards);
    return BNPP_OK;
}

int bnpp_model_values(const bnpp_model *m, double *values) {
    if (!m || !values) return set_err(BNPP_ERR_INVALID, "null argument");
    for (const auto &v : m->d.values) values = std::copy(v.begin(), v.end(), values);
    return BNPP_OK;
}

int bnpp_evidence_load(const char *path, int cap, int *n, int *vars, int *vals) {
    BNPP_GUARD_BEGIN
    if (!path || !n) return set_err(BNPP_ERR_INVALID, "null argument");
    std::vector<std::pair<int, int>> ev;
    if (load_evidence(path, ev)) return set_err(BNPP_ERR_IO, std::string("couldn't read file ") + path);
    *n = (int)ev.size();
    if ((int)ev.size() > cap) return set_err(BNPP_ERR_INVALID, "evidence larger than cap");
    for (size_t i = 0; i < ev.size(); ++i) {
        vars[i] = ev[i].first;
        vals[i] = ev[i].second;
    }
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_evidence_load_batch(const char *path, int cap_vars, int64_t cap_rows, int *n_ev, int *ev_vars,
                             int64_t *n_rows, int *ev_vals) {
    BNPP_GUARD_BEGIN
    if (!path || !n_ev || !n_rows) return set_err(BNPP_ERR_INVALID, "null argument");
    std::vector<int> vars, vals;
    int64_t rows = 0;
    std::string msg;
    const int rc = load_evidence_batch(path, vars, vals, rows, &msg);
    if (rc == -1) return set_err(BNPP_ERR_IO, std::string("couldn't read file ") + path);
    if (rc == -3) return set_err(BNPP_ERR_UNSUPPORTED, msg);
    if (rc) return set_err(BNPP_ERR_IO, msg);
    *n_ev = (int)vars.size();
    *n_rows = rows;
    if ((int)vars.size() > cap_vars || rows > cap_rows) return set_err(BNPP_ERR_INVALID, "evidence larger than cap");
    if ((!vars.empty() && !ev_vars) || (!vals.empty() && !ev_vals)) return set_err(BNPP_ERR_INVALID, "null argument");
    std::copy(vars.begin(), vars.end(), ev_vars);
    std::copy(vals.begin(), vals.end(), ev_vals);
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_evidence_load_batch_mv(const char *path, int cap_vars, int64_t cap_rows, int *n_ev, int *ev_vars,
                                int64_t *n_rows, int *ev_vals, unsigned char *partial) {
    BNPP_GUARD_BEGIN
    if (!path || !n_ev || !n_rows) return set_err(BNPP_ERR_INVALID, "null argument");
    std::vector<int> vars, vals;
    std::vector<unsigned char> part;
    int64_t rows = 0;
    std::string msg;
    const int rc = load_evidence_batch_missing(path, vars, vals, part, rows, &msg);
    if (rc == -1) return set_err(BNPP_ERR_IO, std::string("couldn't read file ") + path);
    if (rc) return set_err(BNPP_ERR_IO, msg);
    *n_ev = (int)vars.size();
    *n_rows = rows;
    if ((int)vars.size() > cap_vars || rows > cap_rows) return set_err(BNPP_ERR_INVALID, "evidence larger than cap");
    if ((!vars.empty() && (!ev_vars || !partial)) || (!vals.empty() && !ev_vals)) return set_err(BNPP_ERR_INVALID, "null argument");
    std::copy(vars.begin(), vars.end(), ev_vars);
    std::copy(vals.begin(), vals.end(), ev_vals);
    std::copy(part.begin(), part.end(), partial);
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_condition_batch_sv(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in,
                            int ndims, const int *vars, int n_ev, const int *ev_vars, const unsigned char *partial,
                            int n_soft, const int *soft_vars, const void *lam, int64_t n_rows, const int32_t *ev,
                            void *out) {
    BNPP_GUARD_BEGIN
    if (!ctx || !cards || !in || !out || (n_ev > 0 && (!ev_vars || !ev))) return set_err(BNPP_ERR_INVALID, "null argument");
    if (n_soft < 0 || (n_soft > 0 && (!soft_vars || !lam))) return set_err(BNPP_ERR_INVALID, "bad soft evidence arrays");
    for (int i = 0; i < n_soft; ++i) {
        if (soft_vars[i] < 0 || soft_vars[i] >= n_cards)
            return set_err(BNPP_ERR_INVALID, "soft variable " + std::to_string(soft_vars[i]) + " out of range");
        for (int k = 0; k < i; ++k)
            if (soft_vars[k] == soft_vars[i])
                return set_err(BNPP_ERR_INVALID, "soft variable " + std::to_string(soft_vars[i]) + " is listed twice");
        for (int e = 0; e < n_ev; ++e)
            if (ev_vars[e] == soft_vars[i])
                return set_err(BNPP_ERR_INVALID, "variable " + std::to_string(soft_vars[i]) + " is both an evidence and a soft variable");
    }
    if (dtype != BNPP_F32 && dtype != BNPP_F64) return set_err(BNPP_ERR_INVALID, "dtype must be BNPP_F64 or BNPP_F32");
    if (n_cards < 0 || !valid_scope(ndims, vars, cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad input scope");
    if (n_ev < 0 || !valid_scope(n_ev, ev_vars, cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad evidence variables");
    if (n_rows < 1 || n_rows > (int64_t)INT32_MAX) return set_err(BNPP_ERR_INVALID, "n_rows must be in [1, 2^31)");
    std::vector<int> cv(cards, cards + n_cards);
    cv.push_back((int)n_rows);                              // the row variable
    BucketSpec b;
    b.cond_batch = true;
    b.in.push_back(natural_view(0, std::vector<int>(vars, vars + ndims), cv));
    int n_in_scope = 0;
    bool masked = false, weighted = false;
    for (int j = 0; j < ndims; ++j) {
        int row = -1, lrow = -1, lnext = 0;
        for (int e = 0; e < n_ev; ++e)
            if (ev_vars[e] == vars[j]) row = e;
        for (int i = 0; i < n_soft; ++i) {                  // the variable's first row of lam: the cards of those before it
            if (soft_vars[i] == vars[j]) lrow = lnext;
            lnext += cards[soft_vars[i]];
        }
        b.soft_rows.push_back(lrow);
        weighted = weighted || lrow >= 0;
        const bool part = row >= 0 && partial && partial[row];     // kept, under the row's mask
        b.cond_rows.push_back(part ? -1 : row);
        b.mask_rows.push_back(part ? row : -1);
        masked = masked || part;
        if (row < 0 || part) b.out_vars.push_back(vars[j]);
        else ++n_in_scope;
    }
    if (!masked) b.mask_rows.clear();
    if (!weighted) b.soft_rows.clear();
    if (n_in_scope > kCondMaxEv) return set_err(BNPP_ERR_UNSUPPORTED, "at most 32 evidence variables in the scope of a single-op call");
    b.out_vars.push_back(n_cards);
    b.out_table = 1;
    BucketDesc d;
    std::vector<int64_t> pool;
    std::string msg;
    if (!build_desc(b, cv, max_vec_for(dtype), d, pool, &msg)) return set_err(BNPP_ERR_UNSUPPORTED, msg);
    const int form = weighted ? kCondWeighted : masked ? kCondMasked : kCondPlain;
    CondBatchArgs a;
    std::memset(&a, 0, sizeof a);
    if ((int64_t)pool.size() > cond_single_pool_words(form)) return set_err(BNPP_ERR_UNSUPPORTED, "scope too wide for a single-op call");
    std::copy(pool.begin(), pool.end(), a.pool);
    a.src = in;
    a.out = out;
    a.ev = ev;
    a.lam = weighted ? lam : nullptr;
    a.n_rows = n_rows;
    hipError_t e = hipSetDevice(ctx->c.device);
    if (e == hipSuccess) e = launch_cond_batch_single(dtype == BNPP_F32, form, a, ctx->c.max_grid, pick_stream(ctx, stream));
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_condition_batch_mv(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in,
                            int ndims, const int *vars, int n_ev, const int *ev_vars, const unsigned char *partial,
                            int64_t n_rows, const int32_t *ev, void *out) {
    return bnpp_condition_batch_sv(ctx, stream, dtype, n_cards, cards, in, ndims, vars, n_ev, ev_vars, partial, 0, nullptr,
                                   nullptr, n_rows, ev, out);
}

int bnpp_likelihood_load(const bnpp_model *m, const char *path, int cap_vars, int64_t cap_vals, int *n_soft,
                         int *soft_vars, int64_t *n_rows, double *lik) {
    BNPP_GUARD_BEGIN
    if (!m || !path || !n_soft || !n_rows) return set_err(BNPP_ERR_INVALID, "null argument");
    std::ifstream f(path);
    if (!f) return set_err(BNPP_ERR_IO, std::string("couldn't read file ") + path);
    const int nv = (int)m->d.cards.size();
    long long ns = 0, nr = 0;
    if (!(f >> ns) || ns < 0 || ns > nv) return set_err(BNPP_ERR_IO, std::string(path) + ": bad soft variable count");
    std::vector<int> vars((size_t)ns);
    int64_t ws = 0;
    for (auto &v : vars) {
        if (!(f >> v) || v < 0 || v >= nv) return set_err(BNPP_ERR_IO, std::string(path) + ": bad soft variable id");
        ws += m->d.cards[v];
    }
    if (!(f >> nr) || nr < 0) return set_err(BNPP_ERR_IO, std::string(path) + ": bad row count");
    *n_soft = (int)ns;
    *n_rows = nr;
    if (ns > cap_vars) return set_err(BNPP_ERR_INVALID, "likelihoods larger than cap");
    if (ns > 0 && !soft_vars) return set_err(BNPP_ERR_INVALID, "null argument");
    std::copy(vars.begin(), vars.end(), soft_vars);
    if (nr * ws > cap_vals) return set_err(BNPP_ERR_INVALID, "likelihoods larger than cap");
    if (nr * ws > 0 && !lik) return set_err(BNPP_ERR_INVALID, "null argument");
    for (int64_t i = 0; i < nr * ws; ++i) {
        std::string tok;
        if (!(f >> tok)) return set_err(BNPP_ERR_IO, std::string(path) + ": row " + std::to_string(i / ws) + " is short");
        char *end = nullptr;
        lik[i] = std::strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end) return set_err(BNPP_ERR_IO, std::string(path) + ": row " + std::to_string(i / ws) + ": bad number " + tok);
    }
    return BNPP_OK;
    BNPP_GUARD_END
}

// A hook of the test suite, not part of include/bnpp.h: the job cache key of a bnpp_partition_batch call of this
// shape with the default heuristic and at least 2^16 rows (tests/test_soft_host.py: the key ignores values and is
// the old one without soft variables)
extern "C" int bnpp_batch_job_key(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int n_soft,
                                  const int *soft_vars, int dtype, int64_t rows_per_launch, uint64_t *key);
int bnpp_batch_job_key(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int n_soft,
                       const int *soft_vars, int dtype, int64_t rows_per_launch, uint64_t *key) {
    BNPP_GUARD_BEGIN
    if (!m || !key || (n_ev > 0 && !ev_vars) || (n_soft > 0 && !soft_vars)) return set_err(BNPP_ERR_INVALID, "null argument");
    BatchCall c = batch_call(m, kKindBatch, n_ev, ev_vars, BNPP_MIN_FILL, nullptr, 0, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, nullptr);
    *key = batch_call_key(c, kBatchAutoRows);
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_condition_batch(bnpp_ctx *ctx, void *stream, int dtype, int n_cards, const int *cards, const void *in,
                         int ndims, const int *vars, int n_ev, const int *ev_vars, int64_t n_rows, const int32_t *ev,
                         void *out) {
    return bnpp_condition_batch_mv(ctx, stream, dtype, n_cards, cards, in, ndims, vars, n_ev, ev_vars, nullptr, n_rows, ev,
                                   out);
}

int bnpp_ordering(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int n_vars,
                  const int *vars, int heuristic, int *order_out, int *width_out) {
    BNPP_GUARD_BEGIN
    if (!m || !order_out) return set_err(BNPP_ERR_INVALID, "null argument");
    if (heuristic < BNPP_ORDER_GIVEN || heuristic > BNPP_MIN_DEGREE) return set_err(BNPP_ERR_INVALID, "unknown heuristic");
    const ModelData &d = m->d;
    std::vector<int> ev;
    std::string msg;
    if (!evidence_array(d, n_ev, ev_vars, ev_vals, ev, msg)) return set_err(BNPP_ERR_INVALID, msg);
    std::vector<int> vs;
    if (vars) {
        for (int i = 0; i < n_vars; ++i) {
            if (vars[i] < 0 || vars[i] >= (int)d.cards.size()) return set_err(BNPP_ERR_INVALID, "bad variable");
            vs.push_back(vars[i]);
        }
    } else {
        for (int v = 0; v < (int)d.cards.size(); ++v)
            if (ev[v] < 0) vs.push_back(v);
    }
    std::vector<int> ord;
    int w = elimination_order((int)d.cards.size(), d.cards, conditioned_scopes(d, ev), vs, (Heuristic)heuristic, ord);
    std::copy(ord.begin(), ord.end(), order_out);
    if (width_out) *width_out = w;
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_job_create(bnpp_ctx *ctx, const bnpp_model *m, int kind, int n_ev, const int *ev_vars, const int *ev_vals,
                    int heuristic, const int *order, int n_order, int n_targets, const int *targets, int dtype,
                    bnpp_job **out) {
    BNPP_GUARD_BEGIN
    if (!out) return set_err(BNPP_ERR_INVALID, "null output");
    *out = nullptr;
    if (kind != 0 && kind != 1 && kind != 3 && kind != 4)
        return set_err(BNPP_ERR_INVALID, "kind must be 0 (partition), 1 (marginals), 3 (bucket-tree marginals) or 4 (MPE)");
    std::unique_ptr<bnpp_job> job;
    int rc = create_job(ctx, m, kind, n_ev, ev_vars, ev_vals, heuristic, order, n_order, n_targets, targets, dtype, job);
    if (rc) {
        if (job) destroy_job(job.release());
        return rc;
    }
    *out = job.release();
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_variable_elimination(bnpp_ctx *ctx, const bnpp_model *m, int n_vars, const int *vars, int heuristic,
                              int dtype, int cap_vars, int *out_ndims, int *out_vars, int64_t cap_values,
                              int64_t *out_size, double *out_values, int64_t *exp2) {
    BNPP_GUARD_BEGIN
    if (!out_ndims || !out_size || !exp2 || (n_vars > 0 && !vars)) return set_err(BNPP_ERR_INVALID, "null argument");
    std::unique_ptr<bnpp_job> job;
    std::unique_lock<std::mutex> lk;
    if (ctx) lk = std::unique_lock<std::mutex>(ctx->cache_mu, std::try_to_lock);
    int rc = create_job(ctx, m, 2, 0, nullptr, nullptr, heuristic, vars, n_vars, 0, nullptr, dtype, job, 0, 1,
                        lk.owns_lock());
    if (rc == BNPP_OK) rc = from_ctx(ctx, launch_program(ctx->c, job->pg, ctx->c.stream));
    std::vector<std::vector<double>> vals;
    std::vector<int64_t> e2;
    if (rc == BNPP_OK) rc = from_ctx(ctx, fetch_program(ctx->c, job->pg, ctx->c.stream, vals, e2));
    if (rc == BNPP_OK) {
        const std::vector<int> &rv = job->pg.parts[0].sched.plan_result_vars[0];
        *out_ndims = (int)rv.size();
        *out_size = (int64_t)vals[0].size();
        *exp2 = e2[0];
        if ((int)rv.size() > cap_vars || (int64_t)vals[0].size() > cap_values) {
            rc = set_err(BNPP_ERR_INVALID, "result larger than the output capacity");
        } else {
            std::copy(rv.begin(), rv.end(), out_vars);
            std::copy(vals[0].begin(), vals[0].end(), out_values);
        }
    }
    if (job) destroy_job(job.release());
    return rc;
    BNPP_GUARD_END
}

int bnpp_plan_stats(const bnpp_model *m, int kind, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                    const int *order, int n_order, int dtype, double *stats, int n_stats) {
    BNPP_GUARD_BEGIN
    if (!m || !stats) return set_err(BNPP_ERR_INVALID, "null argument");
    if (kind < 0 || kind > 4) return set_err(BNPP_ERR_INVALID, "kind must be 0, 1, 2, 3 or 4");
    std::vector<int> ev, targets;
    std::string msg;
    if (!evidence_array(m->d, n_ev, ev_vars, ev_vals, ev, msg)) return set_err(BNPP_ERR_INVALID, msg);
    if (kind == 1 || kind == 3)
        for (int v = 0; v < (int)m->d.cards.size(); ++v) targets.push_back(v);
    std::vector<Schedule> batches;
    double st[10] = {0};
    int rc = plan_schedules(m->d, ev, kind, heuristic, order, n_order, targets, dtype, memory_budget(nullptr), batches, st);
    if (rc) return rc;
    for (int i = 0; i < n_stats && i < 8; ++i) stats[i] = st[i];
    return BNPP_OK;
    BNPP_GUARD_END
}

// the launch groups of a plan (bnpp_plan_groups: kinds 0-3; bnpp_plan_mpe_groups: kind 4)
static int plan_groups_rows(const bnpp_model *m, int kind, int n_ev, const int *ev_vars, const int *ev_vals,
                            int heuristic, const int *order, int n_order, int dtype, int part, int n_parts,
                            int64_t *rows, int cap_rows, int *n_rows) {
    BNPP_GUARD_BEGIN
    if (!m || !n_rows || (cap_rows > 0 && !rows)) return set_err(BNPP_ERR_INVALID, "null argument");
    if (n_parts < 1 || part < 0 || part >= n_parts || (n_parts > 1 && kind != 3))
        return set_err(BNPP_ERR_INVALID, "bad part / n_parts");
    std::vector<int> ev, targets;
    std::string msg;
    if (!evidence_array(m->d, n_ev, ev_vars, ev_vals, ev, msg)) return set_err(BNPP_ERR_INVALID, msg);
    if (kind == 1 || kind == 3)
        for (int v = 0; v < (int)m->d.cards.size(); ++v) targets.push_back(v);
    std::vector<Schedule> batches;
    double st[10] = {0};
    int rc = plan_schedules(m->d, ev, kind, heuristic, order, n_order, targets, dtype, memory_budget(nullptr), batches, st,
                            part, n_parts);
    if (rc) return rc;
    int64_t n = 0;
    for (size_t b = 0; b < batches.size(); ++b) n = copy_group_rows(batches[b], (int64_t)b, rows, cap_rows, n);
    if (n > INT32_MAX) return set_err(BNPP_ERR_UNSUPPORTED, "more launch groups than the count can hold");
    *n_rows = (int)n;
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_plan_groups(const bnpp_model *m, int kind, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                     const int *order, int n_order, int dtype, int part, int n_parts, int64_t *rows, int cap_rows,
                     int *n_rows) {
    // the sum plans; an MPE plan's groups have an entry point of their own (bnpp_plan_mpe_groups)
    if (kind < 0 || kind > 3) return set_err(BNPP_ERR_INVALID, "kind must be 0, 1, 2 or 3");
    return plan_groups_rows(m, kind, n_ev, ev_vars, ev_vals, heuristic, order, n_order, dtype, part, n_parts, rows,
                            cap_rows, n_rows);
}

int bnpp_plan_mpe_groups(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                         const int *order, int n_order, int dtype, int64_t *rows, int cap_rows, int *n_rows) {
    return plan_groups_rows(m, 4, n_ev, ev_vars, ev_vals, heuristic, order, n_order, dtype, 0, 1, rows, cap_rows, n_rows);
}

int bnpp_plan_sample(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                     const int *order, int n_order, int dtype, int64_t n_samples, double *stats, int n_stats,
                     int64_t *rows, int cap_rows, int *n_rows) {
    BNPP_GUARD_BEGIN
    if (!m || !n_rows || (cap_rows > 0 && !rows) || (n_stats > 0 && !stats)) return set_err(BNPP_ERR_INVALID, "null argument");
    if (n_samples < 1) return set_err(BNPP_ERR_INVALID, "n_samples must be at least 1");
    std::vector<int> ev, targets;
    std::string msg;
    if (!evidence_array(m->d, n_ev, ev_vars, ev_vals, ev, msg)) return set_err(BNPP_ERR_INVALID, msg);
    std::vector<Schedule> batches;
    double st[12] = {0};
    int rc = plan_schedules(m->d, ev, kKindSample, heuristic, order, n_order, targets, dtype, memory_budget(nullptr), batches,
                            st, 0, 1, 1, 0, n_samples, st + 10);
    if (rc) return rc;
    st[8] = st[10];                                  // rows of the sampling step
    st[9] = st[11];                                  // bytes of x
    for (int i = 0; i < n_stats && i < 10; ++i) stats[i] = st[i];
    int64_t n = 0;
    for (size_t b = 0; b < batches.size(); ++b) n = copy_group_rows(batches[b], (int64_t)b, rows, cap_rows, n);
    if (n > INT32_MAX) return set_err(BNPP_ERR_UNSUPPORTED, "more launch groups than the count can hold");
    *n_rows = (int)n;
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_plan_single(int dtype, int n_cards, const int *cards, int n_in, const int *in_ndims, const int *const *in_vars,
                     int elim_var, int out_ndims, const int *out_vars, int divide, int n_ev, const int *ev_vars,
                     const int *ev_vals, int64_t *info, int n_info) {
    BNPP_GUARD_BEGIN
    if (!cards || n_in < 1 || !in_ndims || !in_vars || !info || (n_ev > 0 && (!ev_vars || !ev_vals)))
        return set_err(BNPP_ERR_INVALID, "null argument");
    if (n_in > kMaxIn) return set_err(BNPP_ERR_UNSUPPORTED, "at most 8 inputs per fused call");
    if (n_cards < 0 || elim_var >= n_cards || (out_ndims > 0 && !out_vars) || n_ev < 0)
        return set_err(BNPP_ERR_INVALID, "variable id outside cards[0, n_cards)");
    for (int i = 0; i < n_in; ++i)
        if (!valid_scope(in_ndims[i], in_vars[i], cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad input scope");
    if (!valid_scope(out_ndims, out_vars, cards, n_cards)) return set_err(BNPP_ERR_INVALID, "bad output scope");
    if (divide && (n_in != 2 || elim_var >= 0)) return set_err(BNPP_ERR_INVALID, "divide takes two inputs and sums nothing");
    std::vector<int> cv(cards, cards + n_cards);
    // the conditioning view (bnpp_condition): evidence on a variable outside a scope does not touch it
    std::vector<int> ev(n_cards, -1);
    for (int i = 0; i < n_ev; ++i) {
        const int v = ev_vars[i];
        if (v < 0) return set_err(BNPP_ERR_INVALID, "bad evidence variable");
        if (v >= n_cards) continue;
        if (ev_vals[i] < 0 || ev_vals[i] >= cv[v]) return set_err(BNPP_ERR_INVALID, "evidence value out of range");
        ev[v] = ev_vals[i];
    }
    BucketSpec b;
    for (int i = 0; i < n_in; ++i) {
        std::vector<int> s(in_vars[i], in_vars[i] + in_ndims[i]);
        b.in.push_back(n_ev > 0 ? conditioned_view(i, s, cv, ev) : natural_view(i, s, cv));
    }
    b.elim_var = elim_var;
    std::vector<int> u = chain_scope(b.in);
    if (elim_var >= 0) u = remove_var(u, elim_var);
    std::vector<int> ov(out_vars, out_vars + out_ndims), us = u, os = ov;
    std::sort(us.begin(), us.end());
    std::sort(os.begin(), os.end());
    if (us != os) return set_err(BNPP_ERR_INVALID, "output scope must be the union of the inputs minus elim_var");
    b.out_vars = ov;
    b.out_table = n_in;
    b.divide = divide != 0;
    SingleArgs a;
    if (int rc = plan_single(dtype, cv, b, a)) return rc;
    const SingleKey sk = single_key(dtype == BNPP_F32, a);
    std::vector<int> keys;
    kernel_keys(dtype == BNPP_F32, 0, sk.family, keys);
    const bool o32 = sk.family == kFamGeneric && (sk.key & kGenericO32);
    const int64_t v[12] = {sk.family, sk.key, a.d.n_in, a.d.k, a.d.v1, a.d.v2, a.d.big >= 0 ? a.d.bcls : 0, o32 ? 1 : 0,
                           a.d.n_tiles, a.d.lanes, a.d.slab_y2,
                           std::find(keys.begin(), keys.end(), sk.key) != keys.end() ? 1 : 0};
    for (int i = 0; i < n_info && i < 12; ++i) info[i] = v[i];
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_kernel_keys(int dtype, int launch, int family, int *keys, int cap, int *n) {
    BNPP_GUARD_BEGIN
    if (!n || (cap > 0 && !keys)) return set_err(BNPP_ERR_INVALID, "null argument");
    if ((dtype != BNPP_F32 && dtype != BNPP_F64) || (launch != 0 && launch != 1) || family < kFamGeneric || family > kFamMax)
        return set_err(BNPP_ERR_INVALID, "bad dtype, launch or family");
    std::vector<int> k;
    kernel_keys(dtype == BNPP_F32, launch, family, k);
    *n = (int)k.size();
    for (int i = 0; i < *n && i < cap; ++i) keys[i] = k[i];
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_chain_key_supported(int dtype, int key, int *supported) {
    if (!supported || (dtype != BNPP_F32 && dtype != BNPP_F64)) return set_err(BNPP_ERR_INVALID, "bad dtype or null output");
    *supported = chain_supported(dtype == BNPP_F32 ? 4 : 8, key) ? 1 : 0;
    return BNPP_OK;
}

int bnpp_plan_tree_part(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                        const int *order, int n_order, int part, int n_parts, int dtype, int *owned, double *stats,
                        int n_stats) {
    BNPP_GUARD_BEGIN
    if (!m || !owned) return set_err(BNPP_ERR_INVALID, "null argument");
    if (n_parts < 1 || part < 0 || part >= n_parts) return set_err(BNPP_ERR_INVALID, "bad part / n_parts");
    std::vector<int> ev, targets;
    std::string msg;
    if (!evidence_array(m->d, n_ev, ev_vars, ev_vals, ev, msg)) return set_err(BNPP_ERR_INVALID, msg);
    for (int v = 0; v < (int)m->d.cards.size(); ++v) targets.push_back(v);
    std::vector<Schedule> batches;
    double st[10] = {0};
    int rc = plan_schedules(m->d, ev, 3, heuristic, order, n_order, targets, dtype, memory_budget(nullptr), batches, st,
                            part, n_parts);
    if (rc) return rc;
    size_t i = 0;
    for (auto &s : batches)
        for (char c : s.plan_result_owned) owned[i++] = c ? 1 : 0;
    for (int k = 0; stats && k < n_stats && k < 8; ++k) stats[k] = st[k];
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_job_stats(const bnpp_job *job, double *stats, int n_stats) {
    if (!job || !stats) return set_err(BNPP_ERR_INVALID, "null argument");
    for (int i = 0; i < n_stats && i < 8; ++i) stats[i] = job->stats[i];
    return BNPP_OK;
}

int bnpp_job_launch(bnpp_job *job, void *stream) {
    BNPP_GUARD_BEGIN
    if (!job) return set_err(BNPP_ERR_INVALID, "null job");
    (void)hipSetDevice(job->ctx->c.device);
    return from_ctx(job->ctx, launch_program(job->ctx->c, job->pg, pick_stream(job->ctx, stream)));
    BNPP_GUARD_END
}

int bnpp_job_results(bnpp_job *job, void *stream, double *out) {
    BNPP_GUARD_BEGIN
    if (!job || !out) return set_err(BNPP_ERR_INVALID, "null argument");
    (void)hipSetDevice(job->ctx->c.device);
    return job_results(job, pick_stream(job->ctx, stream), out, nullptr);
    BNPP_GUARD_END
}

int bnpp_job_free(bnpp_job *job) {
    destroy_job(job);
    return BNPP_OK;
}

int bnpp_partition(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                   int heuristic, const int *order, int n_order, int dtype, double *log10_z, double *z,
                   double *uptime_ms) {
    BNPP_GUARD_BEGIN
    double t0 = now_ms();
    if (!ctx || !m) return set_err(BNPP_ERR_INVALID, "null context or model");
    bnpp_job *job = nullptr;
    std::unique_lock<std::mutex> lk(ctx->cache_mu, std::try_to_lock);
    const bool cache_ok = lk.owns_lock();
    const int64_t budget = memory_budget(ctx, true);
    const uint64_t key = cache_ok ? call_key(m, 0, n_ev, ev_vars, ev_vals, heuristic, order, n_order, 0, nullptr, dtype,
                                             0, 1) : 0;
    int rc = oneshot_job(ctx, cache_ok, key, budget, [&](std::unique_ptr<bnpp_job> &j) {
        return create_job(ctx, m, 0, n_ev, ev_vars, ev_vals, heuristic, order, n_order, 0, nullptr, dtype, j, 0, 1,
                          cache_ok);
    }, job);
    const double t1 = now_ms();
    if (rc == BNPP_OK) rc = from_ctx(ctx, launch_program(ctx->c, job->pg, ctx->c.stream));
    const double t2 = now_ms();
    double lz = 0, zz = 0;
    if (rc == BNPP_OK) rc = job_results(job, ctx->c.stream, &lz, &zz);
    const double t3 = now_ms();
    oneshot_done(ctx, cache_ok, key, budget, job, rc);
    record_call_timing(t0, t1, t2, t3);
    if (rc) return rc;
    if (log10_z) *log10_z = lz;
    if (z) *z = zz;
    if (uptime_ms) *uptime_ms = now_ms() - t0;
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_mpe(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
             const int *order, int n_order, int dtype, double *log10_value, int *assignment, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    double t0 = now_ms();
    if (!ctx || !m) return set_err(BNPP_ERR_INVALID, "null context or model");
    bnpp_job *job = nullptr;
    std::unique_lock<std::mutex> lk(ctx->cache_mu, std::try_to_lock);
    const bool cache_ok = lk.owns_lock();
    const int64_t budget = memory_budget(ctx, true);
    // the job kind is part of the key: an MPE call and a PR call on the same model never share a job
    const uint64_t key = cache_ok ? call_key(m, 4, n_ev, ev_vars, ev_vals, heuristic, order, n_order, 0, nullptr, dtype,
                                             0, 1) : 0;
    int rc = oneshot_job(ctx, cache_ok, key, budget, [&](std::unique_ptr<bnpp_job> &j) {
        return create_job(ctx, m, 4, n_ev, ev_vars, ev_vals, heuristic, order, n_order, 0, nullptr, dtype, j, 0, 1,
                          cache_ok);
    }, job);
    const double t1 = now_ms();
    if (rc == BNPP_OK) rc = from_ctx(ctx, launch_program(ctx->c, job->pg, ctx->c.stream));
    const double t2 = now_ms();
    std::vector<double> res(1 + m->d.cards.size(), 0.0);
    if (rc == BNPP_OK) rc = job_results(job, ctx->c.stream, res.data(), nullptr);
    const double t3 = now_ms();
    oneshot_done(ctx, cache_ok, key, budget, job, rc);
    record_call_timing(t0, t1, t2, t3);
    if (rc) return rc;
    if (log10_value) *log10_value = res[0];
    if (assignment)
        for (size_t v = 0; v < m->d.cards.size(); ++v) assignment[v] = (int)res[1 + v];
    if (uptime_ms) *uptime_ms = now_ms() - t0;
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_sample(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                const int *order, int n_order, int dtype, int64_t n_samples, int64_t first_sample, uint64_t seed,
                uint8_t *out, double *log10_z, int64_t *n_degenerate, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    double t0 = now_ms();
    if (!ctx || !m) return set_err(BNPP_ERR_INVALID, "null context or model");
    if (n_samples < 1 || first_sample < 0) return set_err(BNPP_ERR_INVALID, "n_samples must be at least 1, first_sample at least 0");
    bnpp_job *job = nullptr;
    std::unique_lock<std::mutex> lk(ctx->cache_mu, std::try_to_lock);
    const bool cache_ok = lk.owns_lock();
    const int64_t budget = memory_budget(ctx, true);
    // the job kind and n_samples are part of the key, seed and first_sample are
    // not: another seed relaunches the cached job
    uint64_t key = cache_ok ? call_key(m, kKindSample, n_ev, ev_vars, ev_vals, heuristic, order, n_order, 0, nullptr, dtype,
                                       0, 1) : 0;
    if (key) {
        key = (key ^ (uint64_t)n_samples) * 1099511628211ull;
        key = key ? key : 1;
    }
    int rc = oneshot_job(ctx, cache_ok, key, budget, [&](std::unique_ptr<bnpp_job> &j) {
        return create_job(ctx, m, kKindSample, n_ev, ev_vars, ev_vals, heuristic, order, n_order, 0, nullptr, dtype, j, 0, 1,
                          cache_ok, 1, 0, 0, n_samples);
    }, job);
    const double t1 = now_ms();
    // the sampling step: the last launch group of the (one) schedule
    const BucketDesc *sd = nullptr;
    Executable *ex = nullptr;
    if (rc == BNPP_OK) {
        if (job->pg.parts.size() == 1 && !job->pg.parts[0].sched.groups.empty() &&
            job->pg.parts[0].sched.groups.back().variant == kSampleKey) {
            ex = &job->pg.parts[0];
            sd = &ex->sched.descs[ex->sched.groups.back().begin];
            ex->sample_seed = seed;
            ex->sample_first = first_sample;
        } else {
            rc = set_err(BNPP_ERR_INVALID, "sampling job without a sampling step");
        }
    }
    if (rc == BNPP_OK) rc = from_ctx(ctx, launch_program(ctx->c, job->pg, ctx->c.stream));
    const double t2 = now_ms();
    double lz = 0;
    bool impossible = false;                               // Z == 0 (or NaN): there is no posterior to draw from
    if (rc == BNPP_OK) {
        std::vector<std::vector<double>> vals;
        std::vector<int64_t> exp2;
        rc = from_ctx(ctx, fetch_program(ctx->c, job->pg, ctx->c.stream, vals, exp2));   // waits for the stream
        if (rc == BNPP_OK) {
            double p = 0;
            for (double v : vals[0]) p += v;
            lz = p > 0 ? std::log10(p) + (double)exp2[0] * std::log10(2.0) : -INFINITY;
            impossible = !(p > 0);
        }
    }
    if (rc == BNPP_OK) {
        const uint8_t *x = static_cast<const uint8_t *>(ex->h_meta[sd->out_table].ptr);
        const int64_t bytes = (int64_t)m->d.cards.size() * n_samples;
        hipError_t e = hipSuccess;
        if (out && bytes > 0) e = hipMemcpy(out, x, (size_t)bytes, hipMemcpyDeviceToHost);
        int64_t cnt = 0;
        if (e == hipSuccess)
            e = hipMemcpy(&cnt, x + sample_counter_offset((int64_t)m->d.cards.size(), n_samples), sizeof cnt, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = set_err(BNPP_ERR_HIP, std::string("hipMemcpy(samples): ") + hipGetErrorString(e));
        if (rc == BNPP_OK && impossible) {
            // impossible evidence: every draw counts as degenerate and every sampled value is 0, also where the
            // zero reached the result without passing through the bucket of a draw (evidence rows keep their values)
            std::vector<char> is_ev(m->d.cards.size(), 0);
            for (int j = 0; j < n_ev; ++j)
                if (ev_vars[j] >= 0 && (size_t)ev_vars[j] < is_ev.size()) is_ev[(size_t)ev_vars[j]] = 1;
            for (size_t v = 0; out && v < is_ev.size(); ++v)
                if (!is_ev[v]) std::memset(out + v * (size_t)n_samples, 0, (size_t)n_samples);
            cnt = n_samples * (int64_t)sd->k;
        }
        if (rc == BNPP_OK && n_degenerate) *n_degenerate = cnt;
    }
    const double t3 = now_ms();
    oneshot_done(ctx, cache_ok, key, budget, job, rc);
    record_call_timing(t0, t1, t2, t3);
    if (rc) return rc;
    if (log10_z) *log10_z = lz;
    if (uptime_ms) *uptime_ms = now_ms() - t0;
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_partition_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik, int heuristic, const int *order,
                            int n_order, int dtype, int64_t rows_per_launch, double *log10_z, double *z,
                            double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, lik);
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    return run_batch(ctx, c, false, log10_z, z, nullptr, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_partition_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int heuristic, const int *order,
                            int n_order, int dtype, int64_t rows_per_launch, double *log10_z, double *z,
                            double *uptime_ms) {
    return bnpp_partition_batch_sv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, partial, 0, nullptr, nullptr, heuristic, order, n_order, dtype, rows_per_launch, log10_z, z, uptime_ms);
}

int bnpp_partition_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals, int heuristic, const int *order, int n_order, int dtype,
                         int64_t rows_per_launch, double *log10_z, double *z, double *uptime_ms) {
    return bnpp_partition_batch_mv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, nullptr, heuristic, order, n_order, dtype,
                                   rows_per_launch, log10_z, z, uptime_ms);
}

int bnpp_posterior_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik, int heuristic, int target, int dtype,
                            int64_t rows_per_launch, double *out, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindBatch, n_ev, ev_vars, heuristic, nullptr, 0, dtype, rows_per_launch, partial, n_soft, soft_vars, lik);
    c.target = target;
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    return run_batch(ctx, c, true, nullptr, nullptr, out, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_posterior_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                            const int *ev_vals, const unsigned char *partial, int heuristic, int target, int dtype,
                            int64_t rows_per_launch, double *out, double *uptime_ms) {
    return bnpp_posterior_batch_sv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, partial, 0, nullptr, nullptr, heuristic, target, dtype, rows_per_launch, out, uptime_ms);
}

int bnpp_posterior_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals, int heuristic, int target, int dtype, int64_t rows_per_launch, double *out,
                         double *uptime_ms) {
    return bnpp_posterior_batch_mv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, nullptr, heuristic, target, dtype,
                                   rows_per_launch, out, uptime_ms);
}

int bnpp_mpe_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                      const int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik, int heuristic, const int *order, int n_order,
                      int dtype, int64_t rows_per_launch, double *log10_value, int *assignment, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindMpeBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, lik);
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    return run_mpe_batch(ctx, c, log10_value, assignment, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_mpe_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                      const int *ev_vals, const unsigned char *partial, int heuristic, const int *order, int n_order,
                      int dtype, int64_t rows_per_launch, double *log10_value, int *assignment, double *uptime_ms) {
    return bnpp_mpe_batch_sv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, partial, 0, nullptr, nullptr, heuristic, order, n_order, dtype, rows_per_launch, log10_value, assignment, uptime_ms);
}

int bnpp_mpe_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows, const int *ev_vals,
                   int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch, double *log10_value,
                   int *assignment, double *uptime_ms) {
    return bnpp_mpe_batch_mv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, nullptr, heuristic, order, n_order, dtype,
                             rows_per_launch, log10_value, assignment, uptime_ms);
}

int bnpp_plan_mpe_batch_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik,
                           int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                           double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *mask_factor, int *lam_factor) {
    BNPP_GUARD_BEGIN
    Schedule s;
    VEPlan plan;
    double st[BNPP_PLAN_MPE_BATCH_STATS] = {0};
    BatchCall c = batch_call(m, kKindMpeBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, lik);
    if (int rc = plan_batch_entry(c, false, stats, n_stats, rows, cap_rows, n_rows, s, plan, st)) return rc;
    st[10] = (double)plan.arg_bytes;
    st[11] = plan.n_max_buckets;
    st[12] = plan.n_arg_b;
    st[13] = plan.n_arg_nob;
    st[14] = (double)plan.arg_b_entries;
    st[15] = (double)plan.arg_nob_entries;
    for (int i = 0; i < n_stats && i < BNPP_PLAN_MPE_BATCH_STATS; ++i) stats[i] = st[i];
    report_evidence_factors(plan, n_ev, mask_factor, n_soft, lam_factor);
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_plan_mpe_batch_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial,
                           int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                           double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *mask_factor) {
    return bnpp_plan_mpe_batch_sv(m, n_ev, ev_vars, partial, 0, nullptr, nullptr, heuristic, order, n_order, dtype, rows_per_launch, stats, n_stats, rows, cap_rows, n_rows, mask_factor, nullptr);
}

int bnpp_plan_mpe_batch(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order, int n_order,
                        int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows, int cap_rows,
                        int *n_rows) {
    return bnpp_plan_mpe_batch_mv(m, n_ev, ev_vars, nullptr, heuristic, order, n_order, dtype, rows_per_launch, stats,
                                  n_stats, rows, cap_rows, n_rows, nullptr);
}

int bnpp_sample_batch_sv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik, int heuristic, const int *order,
                         int n_order, int dtype, int64_t rows_per_launch, int64_t n_per_row, int64_t first_sample,
                         int64_t row_stride, uint64_t seed, uint8_t *out, double *log10_z, int64_t *n_degenerate,
                         double *uptime_ms) {
    BNPP_GUARD_BEGIN
    BatchCall c = batch_call(m, kKindSampleBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, lik);
    c.K = n_per_row;
    c.n_rows = n_rows;
    c.ev_vals = ev_vals;
    return run_sample_batch(ctx, c, first_sample, row_stride, seed, out, log10_z, n_degenerate, uptime_ms);
    BNPP_GUARD_END
}

int bnpp_sample_batch_mv(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows,
                         const int *ev_vals, const unsigned char *partial, int heuristic, const int *order,
                         int n_order, int dtype, int64_t rows_per_launch, int64_t n_per_row, int64_t first_sample,
                         int64_t row_stride, uint64_t seed, uint8_t *out, double *log10_z, int64_t *n_degenerate,
                         double *uptime_ms) {
    return bnpp_sample_batch_sv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, partial, 0, nullptr, nullptr, heuristic, order, n_order, dtype, rows_per_launch, n_per_row, first_sample, row_stride, seed, out, log10_z, n_degenerate, uptime_ms);
}

int bnpp_sample_batch(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, int64_t n_rows, const int *ev_vals,
                      int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch, int64_t n_per_row,
                      int64_t first_sample, int64_t row_stride, uint64_t seed, uint8_t *out, double *log10_z,
                      int64_t *n_degenerate, double *uptime_ms) {
    return bnpp_sample_batch_mv(ctx, m, n_ev, ev_vars, n_rows, ev_vals, nullptr, heuristic, order, n_order, dtype,
                                rows_per_launch, n_per_row, first_sample, row_stride, seed, out, log10_z,
                                n_degenerate, uptime_ms);
}

int bnpp_plan_sample_batch_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik,
                              int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                              int64_t n_per_row, double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows,
                              int *mask_factor, int *lam_factor) {
    BNPP_GUARD_BEGIN
    Schedule s;
    VEPlan plan;
    double st[BNPP_PLAN_SAMPLE_BATCH_STATS] = {0};
    BatchCall c = batch_call(m, kKindSampleBatch, n_ev, ev_vars, heuristic, order, n_order, dtype, rows_per_launch,
                             partial, n_soft, soft_vars, lik);
    c.K = n_per_row;
    if (int rc = plan_batch_entry(c, false, stats, n_stats, rows, cap_rows, n_rows, s, plan, st)) return rc;
    st[10] = (double)n_per_row;
    st[11] = (double)plan.sample_bytes;
    st[12] = plan.n_draw_b + plan.n_draw_nob;
    st[13] = plan.n_draw_b;
    st[14] = plan.n_draw_nob;
    for (int i = 0; i < n_stats && i < BNPP_PLAN_SAMPLE_BATCH_STATS; ++i) stats[i] = st[i];
    report_evidence_factors(plan, n_ev, mask_factor, n_soft, lam_factor);
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_plan_sample_batch_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial,
                              int heuristic, const int *order, int n_order, int dtype, int64_t rows_per_launch,
                              int64_t n_per_row, double *stats, int n_stats, int64_t *rows, int cap_rows, int *n_rows,
                              int *mask_factor) {
    return bnpp_plan_sample_batch_sv(m, n_ev, ev_vars, partial, 0, nullptr, nullptr, heuristic, order, n_order, dtype, rows_per_launch, n_per_row, stats, n_stats, rows, cap_rows, n_rows, mask_factor, nullptr);
}

int bnpp_plan_sample_batch(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order, int n_order,
                           int dtype, int64_t rows_per_launch, int64_t n_per_row, double *stats, int n_stats,
                           int64_t *rows, int cap_rows, int *n_rows) {
    return bnpp_plan_sample_batch_mv(m, n_ev, ev_vars, nullptr, heuristic, order, n_order, dtype, rows_per_launch,
                                     n_per_row, stats, n_stats, rows, cap_rows, n_rows, nullptr);
}

int bnpp_plan_batch_sv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int n_soft, const int *soft_vars,
        const double *lik, int heuristic,
                       const int *order, int n_order, int target, int dtype, int64_t rows_per_launch, double *stats,
                       int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *result_scope, int *n_result_scope,
                       int *mask_factor, int *lam_factor) {
    BNPP_GUARD_BEGIN
    Schedule s;
    VEPlan plan;
    double st[10] = {0};
    BatchCall c = batch_call(m, kKindBatch, n_ev, ev_vars, heuristic, target >= 0 ? nullptr : order,
                             target >= 0 ? 0 : n_order, dtype, rows_per_launch, partial, n_soft, soft_vars, lik);
    c.target = target >= 0 ? target : -1;
    if (int rc = plan_batch_entry(c, target >= 0, stats, n_stats, rows, cap_rows, n_rows, s, plan, st)) return rc;
    for (int i = 0; i < n_stats && i < 10; ++i) stats[i] = st[i];
    const std::vector<int> &rv = s.plan_result_vars[0];
    if (n_result_scope) *n_result_scope = (int)rv.size();
    if (result_scope)
        for (size_t i = 0; i < rv.size() && i < 2; ++i) result_scope[i] = rv[i];
    report_evidence_factors(plan, n_ev, mask_factor, n_soft, lam_factor);
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_plan_batch_mv(const bnpp_model *m, int n_ev, const int *ev_vars, const unsigned char *partial, int heuristic,
                       const int *order, int n_order, int target, int dtype, int64_t rows_per_launch, double *stats,
                       int n_stats, int64_t *rows, int cap_rows, int *n_rows, int *result_scope, int *n_result_scope,
                       int *mask_factor) {
    return bnpp_plan_batch_sv(m, n_ev, ev_vars, partial, 0, nullptr, nullptr, heuristic, order, n_order, target, dtype, rows_per_launch, stats, n_stats, rows, cap_rows, n_rows, result_scope, n_result_scope, mask_factor, nullptr);
}

int bnpp_plan_batch(const bnpp_model *m, int n_ev, const int *ev_vars, int heuristic, const int *order, int n_order,
                    int target, int dtype, int64_t rows_per_launch, double *stats, int n_stats, int64_t *rows,
                    int cap_rows, int *n_rows, int *result_scope, int *n_result_scope) {
    return bnpp_plan_batch_mv(m, n_ev, ev_vars, nullptr, heuristic, order, n_order, target, dtype, rows_per_launch,
                              stats, n_stats, rows, cap_rows, n_rows, result_scope, n_result_scope, nullptr);
}

int bnpp_marginals(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                   int heuristic, int n_targets, const int *targets, int dtype, double *out, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    if (!out) return set_err(BNPP_ERR_INVALID, "null output");
    double t0 = now_ms();
    if (!ctx || !m) return set_err(BNPP_ERR_INVALID, "null context or model");
    bnpp_job *job = nullptr;
    std::unique_lock<std::mutex> lk(ctx->cache_mu, std::try_to_lock);
    const bool cache_ok = lk.owns_lock();
    const int64_t budget = memory_budget(ctx, true);
    const uint64_t key = cache_ok ? call_key(m, 1, n_ev, ev_vars, ev_vals, heuristic, nullptr, 0, n_targets, targets,
                                             dtype, 0, 1) : 0;
    int rc = oneshot_job(ctx, cache_ok, key, budget, [&](std::unique_ptr<bnpp_job> &j) {
        return create_job(ctx, m, 1, n_ev, ev_vars, ev_vals, heuristic, nullptr, 0, n_targets, targets, dtype, j, 0, 1,
                          cache_ok);
    }, job);
    const double t1 = now_ms();
    if (rc == BNPP_OK) rc = from_ctx(ctx, launch_program(ctx->c, job->pg, ctx->c.stream));
    const double t2 = now_ms();
    if (rc == BNPP_OK) rc = job_results(job, ctx->c.stream, out, nullptr);
    const double t3 = now_ms();
    oneshot_done(ctx, cache_ok, key, budget, job, rc);
    record_call_timing(t0, t1, t2, t3);
    if (std::getenv("BNPP_TIMING"))
        std::fprintf(stderr, "[bnpp] marginals: create %.1f ms, launch %.1f ms, run+fetch %.1f ms, free %.1f ms\n",
                     t1 - t0, t2 - t1, t3 - t2, now_ms() - t3);
    if (rc) return rc;
    if (uptime_ms) *uptime_ms = now_ms() - t0;
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_marginals_tree(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                        int heuristic, const int *order, int n_order, int n_targets, const int *targets, int dtype,
                        double *out, double *uptime_ms) {
    return bnpp_marginals_tree_part(ctx, m, n_ev, ev_vars, ev_vals, heuristic, order, n_order, n_targets, targets, 0,
                                    1, dtype, out, nullptr, uptime_ms);
}

int bnpp_marginals_tree_part(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                             int heuristic, const int *order, int n_order, int n_targets, const int *targets,
                             int part, int n_parts, int dtype, double *out, int *owned, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    if (!out) return set_err(BNPP_ERR_INVALID, "null output");
    double t0 = now_ms();
    if (!ctx || !m) return set_err(BNPP_ERR_INVALID, "null context or model");
    const bool timing = std::getenv("BNPP_TIMING") != nullptr;
    bnpp_job *job = nullptr;
    std::unique_lock<std::mutex> lk(ctx->cache_mu, std::try_to_lock);
    const bool cache_ok = lk.owns_lock();
    const int64_t budget = memory_budget(ctx, true);
    const uint64_t key = cache_ok ? call_key(m, 3, n_ev, ev_vars, ev_vals, heuristic, order, n_order, n_targets,
                                             targets, dtype, part, n_parts) : 0;
    int rc = oneshot_job(ctx, cache_ok, key, budget, [&](std::unique_ptr<bnpp_job> &j) {
        return create_job(ctx, m, 3, n_ev, ev_vars, ev_vals, heuristic, order, n_order, n_targets, targets, dtype, j,
                          part, n_parts, cache_ok);
    }, job);
    const double t1 = now_ms();
    if (rc == BNPP_OK) rc = from_ctx(ctx, launch_program(ctx->c, job->pg, ctx->c.stream));
    const double t2 = now_ms();
    if (rc == BNPP_OK) rc = job_results(job, ctx->c.stream, out, nullptr, owned);
    const double t3 = now_ms();
    oneshot_done(ctx, cache_ok, key, budget, job, rc);
    record_call_timing(t0, t1, t2, t3);
    if (timing)
        std::fprintf(stderr, "[bnpp] tree marginals: create %.1f ms, launch %.1f ms, run+fetch %.1f ms, free %.1f ms\n",
                     t1 - t0, t2 - t1, t3 - t2, now_ms() - t3);
    if (rc) return rc;
    if (uptime_ms) *uptime_ms = now_ms() - t0;
    return BNPP_OK;
    BNPP_GUARD_END
}

int bnpp_marginals_tree_sliced(bnpp_ctx *ctx, const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals,
                               int heuristic, const int *order, int n_order, int n_targets, const int *targets,
                               int rank, int n_ranks, bnpp_collective_fn coll, void *user, double budget_gb,
                               int dtype, double *out, int64_t *out_exp2, double *uptime_ms) {
    BNPP_GUARD_BEGIN
    if (!out || !out_exp2 || !coll) return set_err(BNPP_ERR_INVALID, "null output or collective");
    if (n_ranks < 2) return set_err(BNPP_ERR_INVALID, "sliced runs need n_ranks >= 2 (bnpp_marginals_tree otherwise)");
    double t0 = now_ms();
    if (!ctx || !m) return set_err(BNPP_ERR_INVALID, "null context or model");
    // an identical call (same model, evidence, order, targets, dtype, rank,
    // world and budget) relaunches the job the previous one planned, as the
    // one-GPU tree marginals do; the collective is bound per call
    bnpp_job *job = nullptr;
    std::unique_lock<std::mutex> lk(ctx->cache_mu, std::try_to_lock);
    const bool cache_ok = lk.owns_lock();
    const int64_t fixed = budget_gb > 0 ? (int64_t)(budget_gb * 1e9) : 0;
    const int64_t budget = fixed ? fixed : memory_budget(ctx, true);
    const uint64_t key = cache_ok ? call_key(m, 4, n_ev, ev_vars, ev_vals, heuristic, order, n_order, n_targets, targets,
                                             dtype, rank, n_ranks) : 0;
    int rc = oneshot_job(ctx, cache_ok, key, budget, [&](std::unique_ptr<bnpp_job> &j) {
        return create_job(ctx, m, 3, n_ev, ev_vars, ev_vals, heuristic, order, n_order, n_targets, targets, dtype, j,
                          0, 1, cache_ok, n_ranks, rank, fixed);
    }, job);
    const double t1 = now_ms();
    if (rc == BNPP_OK) {
        job->pg.hooks.fn = coll;
        job->pg.hooks.user = user;
        rc = from_ctx(ctx, launch_program(ctx->c, job->pg, ctx->c.stream));
    }
    const double t2 = now_ms();
    if (rc == BNPP_OK) rc = job_results_sliced(job, ctx->c.stream, out, out_exp2);
    const double t3 = now_ms();
    oneshot_done(ctx, cache_ok, key, budget, job, rc);
    record_call_timing(t0, t1, t2, t3);
    if (std::getenv("BNPP_TIMING"))
        std::fprintf(stderr, "[bnpp] sliced tree marginals (rank %d of %d): create %.1f ms, launch %.1f ms, run+fetch %.1f ms\n",
                     rank, n_ranks, t1 - t0, t2 - t1, t3 - t2);
    if (rc) return rc;
    if (uptime_ms) *uptime_ms = now_ms() - t0;
    return BNPP_OK;
    BNPP_GUARD_END
}

// a world of n_ranks identical ranks (user: int[4] = {n_ranks, flags,
// link MB/s, latency us}): every block this rank would receive is a copy of
// what it sends -- the timing of one rank's share of a sliced run on one GPU,
// the data movement local; flags & 1: no bytes move; flags & 2: the stream
// waits the transfer's modelled xGMI time (latency + bytes sent over
// min(n_ranks - 1, 7) links at the given rate each)
int bnpp_collective_loopback(void *user, int op, const void *send, void *recv, int64_t bytes, void *stream) {
    if (!user || !send || !recv || bytes < 0) return 1;
    const int *u = static_cast<const int *>(user);
    const int R = u[0];
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (u[1] & 2) {                                          // a modelled transfer: the stream waits its duration
        const double links = R - 1 < 7 ? R - 1 : 7, sent = (double)bytes * (R - 1);
        const double ns = u[3] * 1e3 + sent / (links * (double)u[2] * 1e6) * 1e9;
        if (launch_delay(ns, s) != hipSuccess) return 1;
    }
    if (u[1] & 1) return 0;                                  // no data movement: the compute alone
    if (op == BNPP_COLL_ALLGATHER) {
        for (int r = 0; r < R; ++r)
            if (hipMemcpyAsync(static_cast<char *>(recv) + (int64_t)r * bytes, send, (size_t)bytes,
                               hipMemcpyDeviceToDevice, s) != hipSuccess)
                return 1;
        return 0;
    }
    if (op == BNPP_COLL_ALLTOALL)
        return hipMemcpyAsync(recv, send, (size_t)bytes * R, hipMemcpyDeviceToDevice, s) == hipSuccess ? 0 : 1;
    return 1;
}

int bnpp_plan_tree_sliced(const bnpp_model *m, int n_ev, const int *ev_vars, const int *ev_vals, int heuristic,
                          const int *order, int n_order, int rank, int n_ranks, int dtype, int *slice_bit,
                          double *stats, int n_stats) {
    BNPP_GUARD_BEGIN
    if (!m) return set_err(BNPP_ERR_INVALID, "null argument");
    if (n_ranks < 2 || rank < 0 || rank >= n_ranks) return set_err(BNPP_ERR_INVALID, "bad rank / n_ranks");
    std::vector<int> ev, targets;
    std::string msg;
    if (!evidence_array(m->d, n_ev, ev_vars, ev_vals, ev, msg)) return set_err(BNPP_ERR_INVALID, msg);
    for (int v = 0; v < (int)m->d.cards.size(); ++v) targets.push_back(v);
    std::vector<Schedule> batches;
    double st[10] = {0};
    int rc = plan_schedules(m->d, ev, 3, heuristic, order, n_order, targets, dtype, memory_budget(nullptr), batches, st,
                            0, 1, n_ranks, rank);
    if (rc) return rc;
    size_t i = 0;
    for (auto &s : batches)
        for (int b : s.plan_result_slice_bit)
            if (slice_bit) slice_bit[i++] = b;
    for (int k = 0; stats && k < n_stats && k < 10; ++k) stats[k] = st[k];
    return BNPP_OK;
    BNPP_GUARD_END
}

// Loopy BP as one launch per phase and iteration (bp.hip bp_flood_*, the
// layout of BpFlood): the choice for models whose iteration is too much work
// for one workgroup and for tables of 2^31 entries or more.  The host checks
// the per-iteration maxima every kBpErrChunk iterations; launches after the
// converging iteration return at once on the device.
// one-workgroup loop up to this much work per iteration (f2v terms x scope
// size + v2f products), the flood beyond (tools/bp_modes.py: a 12x12 Ising
// grid, work 1.2e4, 11 us per iteration in one workgroup against 24 us
// flooded; 32x32, 8.3e4: 61 against 22 us)
constexpr double kBpMultiWork = 32768.0;

static int sum_product_flood(bnpp_ctx *ctx, const ModelData &d, int max_iter, double eps, double *out,
                             int *iterations, double *uptime_ms, double t0) {
    const int nv = (int)d.cards.size(), nf = (int)d.scopes.size();
    std::vector<int32_t> f_edge_off(nf + 1, 0), edge_var, edge_fac, msg_off(1, 0), item_edge, v_edge_off(nv + 1, 0),
        v_edges, marg_off(nv + 1, 0);
    std::vector<uint64_t> edge_stride;
    std::vector<int64_t> tab_off(nf + 1, 0);
    for (int f = 0; f < nf; ++f) {
        const std::vector<int> &sc = d.scopes[f];
        uint64_t size = 1;
        for (int v : sc) size *= (uint64_t)d.cards[v];
        uint64_t st = size;
        for (size_t j = 0; j < sc.size(); ++j) {
            st /= (uint64_t)d.cards[sc[j]];
            const int e = (int)edge_var.size();
            edge_var.push_back(sc[j]);
            edge_fac.push_back(f);
            edge_stride.push_back(st);
            for (int x = 0; x < d.cards[sc[j]]; ++x) item_edge.push_back(e);
            if ((int64_t)msg_off.back() + d.cards[sc[j]] >= INT32_MAX)
                return set_err(BNPP_ERR_UNSUPPORTED, "sum-product: more than 2^31 message entries");
            msg_off.push_back(msg_off.back() + d.cards[sc[j]]);
            ++v_edge_off[sc[j] + 1];
        }
        f_edge_off[f + 1] = (int32_t)edge_var.size();
        tab_off[f + 1] = tab_off[f] + (int64_t)size;
    }
    const int ne = (int)edge_var.size(), nmsg = msg_off.back();
    for (int v = 0; v < nv; ++v) {
        v_edge_off[v + 1] += v_edge_off[v];
        marg_off[v + 1] = marg_off[v] + d.cards[v];
    }
    v_edges.resize(ne);
    {
        std::vector<int32_t> fill(v_edge_off.begin(), v_edge_off.end() - 1);
        for (int e = 0; e < ne; ++e) v_edges[fill[edge_var[e]]++] = msg_off[e];   // ascending edge = factor id
    }
    // segments in entry order, then their lane classes
    std::vector<int64_t> seg_off(nmsg + 1, 0);
    for (int t = 0; t < nmsg; ++t) {
        const int e = item_edge[t];
        const uint64_t terms = (uint64_t)(tab_off[edge_fac[e] + 1] - tab_off[edge_fac[e]]) / d.cards[edge_var[e]];
        seg_off[t + 1] = seg_off[t] + (int64_t)std::max<uint64_t>(1, (terms + kBpSegTerms - 1) / kBpSegTerms);
    }
    const int64_t nseg = seg_off[nmsg];
    if (nseg >= INT32_MAX) return set_err(BNPP_ERR_UNSUPPORTED, "sum-product: more than 2^31 segments");
    std::vector<int32_t> seg_item(nseg), cls[4];
    std::vector<uint64_t> seg_q0(nseg);
    for (int t = 0; t < nmsg; ++t) {
        const int e = item_edge[t];
        const uint64_t terms = (uint64_t)(tab_off[edge_fac[e] + 1] - tab_off[edge_fac[e]]) / d.cards[edge_var[e]];
        for (int64_t s = seg_off[t]; s < seg_off[t + 1]; ++s) {
            const uint64_t q0 = (uint64_t)(s - seg_off[t]) * kBpSegTerms;
            seg_item[s] = t;
            seg_q0[s] = q0;
            cls[bp_lane_class((int64_t)std::min<uint64_t>(kBpSegTerms, terms - std::min(q0, terms)))].push_back((int32_t)s);
        }
    }
    std::vector<int32_t> cls_seg;
    cls_seg.reserve(nseg);
    BpFlood a{};
    const int lanes[4] = {1, 4, 16, 64};
    for (int c = 0; c < 4; ++c) {
        a.cls_pos[c] = (int64_t)cls_seg.size();
        cls_seg.insert(cls_seg.end(), cls[c].begin(), cls[c].end());
        a.cls_pos[c + 1] = (int64_t)cls_seg.size();
        const int64_t per_block = kBpFloodBlock / lanes[c];
        const int64_t blocks = ((int64_t)cls[c].size() + per_block - 1) / per_block;
        if ((int64_t)a.cls_blk[c] + blocks >= INT32_MAX) return set_err(BNPP_ERR_UNSUPPORTED, "sum-product: grid too large");
        a.cls_blk[c + 1] = a.cls_blk[c] + (int32_t)blocks;
    }
    // device block: index arrays (256-B aligned pieces), tables, messages
    size_t off = 0;
    auto place = [&](size_t bytes) {
        const size_t o = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t o_cards = place(4 * (size_t)nv), o_tab_off = place(8 * (size_t)(nf + 1)),
                 o_feo = place(4 * (size_t)(nf + 1)), o_ev = place(4 * (size_t)ne), o_ef = place(4 * (size_t)ne),
                 o_es = place(8 * (size_t)ne), o_mo = place(4 * (size_t)(ne + 1)), o_ie = place(4 * (size_t)nmsg),
                 o_so = place(8 * (size_t)(nmsg + 1)), o_si = place(4 * (size_t)nseg), o_sq = place(8 * (size_t)nseg),
                 o_cs = place(4 * (size_t)nseg), o_veo = place(4 * (size_t)(nv + 1)), o_ve = place(4 * (size_t)ne),
                 o_mgo = place(4 * (size_t)(nv + 1));
    const size_t idx_bytes = off;
    const size_t o_tabs = place(8 * (size_t)tab_off[nf]);
    const size_t o_v2f = place(8 * (size_t)nmsg), o_f2v = place(8 * (size_t)nmsg), o_raw = place(8 * (size_t)nmsg),
                 o_part = place(8 * (size_t)nseg), o_marg = place(8 * (size_t)marg_off[nv]),
                 o_err = place(8 * (size_t)kBpErrRing);
    std::vector<unsigned char> host(idx_bytes);
    auto put = [&](size_t o, const void *src, size_t bytes) {
        if (bytes) std::memcpy(host.data() + o, src, bytes);
    };
    std::vector<int32_t> cards32(d.cards.begin(), d.cards.end());
    put(o_cards, cards32.data(), 4 * (size_t)nv);
    put(o_tab_off, tab_off.data(), 8 * tab_off.size());
    put(o_feo, f_edge_off.data(), 4 * f_edge_off.size());
    put(o_ev, edge_var.data(), 4 * (size_t)ne);
    put(o_ef, edge_fac.data(), 4 * (size_t)ne);
    put(o_es, edge_stride.data(), 8 * (size_t)ne);
    put(o_mo, msg_off.data(), 4 * msg_off.size());
    put(o_ie, item_edge.data(), 4 * (size_t)nmsg);
    put(o_so, seg_off.data(), 8 * seg_off.size());
    put(o_si, seg_item.data(), 4 * (size_t)nseg);
    put(o_sq, seg_q0.data(), 8 * (size_t)nseg);
    put(o_cs, cls_seg.data(), 4 * (size_t)nseg);
    put(o_veo, v_edge_off.data(), 4 * v_edge_off.size());
    put(o_ve, v_edges.data(), 4 * (size_t)ne);
    put(o_mgo, marg_off.data(), 4 * marg_off.size());

    hipStream_t s = ctx->c.stream;
    unsigned char *dev = nullptr;
    if (hipSetDevice(ctx->c.device) != hipSuccess) return set_err(BNPP_ERR_HIP, "sum-product: hipSetDevice");
    if (hipMalloc(&dev, off) != hipSuccess) return set_err(BNPP_ERR_OOM, "sum-product: device allocation");
    struct Free {
        unsigned char *p;
        ~Free() { (void)hipFree(p); }
    } guard{dev};
    a.n_vars = nv;
    a.n_edges = ne;
    a.n_msg = nmsg;
    a.idx64 = std::getenv("BNPP_BP_IDX64") ? 1 : 0;
    a.one_seg = nseg == nmsg ? 1 : 0;
    a.eps = eps;
    a.cards = reinterpret_cast<const int32_t *>(dev + o_cards);
    a.tables = reinterpret_cast<const double *>(dev + o_tabs);
    a.tab_off = reinterpret_cast<const int64_t *>(dev + o_tab_off);
    a.f_edge_off = reinterpret_cast<const int32_t *>(dev + o_feo);
    a.edge_var = reinterpret_cast<const int32_t *>(dev + o_ev);
    a.edge_fac = reinterpret_cast<const int32_t *>(dev + o_ef);
    a.edge_stride = reinterpret_cast<const uint64_t *>(dev + o_es);
    a.msg_off = reinterpret_cast<const int32_t *>(dev + o_mo);
    a.item_edge = reinterpret_cast<const int32_t *>(dev + o_ie);
    a.seg_off = reinterpret_cast<const int64_t *>(dev + o_so);
    a.seg_item = reinterpret_cast<const int32_t *>(dev + o_si);
    a.seg_q0 = reinterpret_cast<const uint64_t *>(dev + o_sq);
    a.cls_seg = reinterpret_cast<const int32_t *>(dev + o_cs);
    a.v_edge_off = reinterpret_cast<const int32_t *>(dev + o_veo);
    a.v_moff = reinterpret_cast<const int32_t *>(dev + o_ve);
    a.marg_off = reinterpret_cast<const int32_t *>(dev + o_mgo);
    a.v2f = reinterpret_cast<double *>(dev + o_v2f);
    a.f2v = reinterpret_cast<double *>(dev + o_f2v);
    a.raw = reinterpret_cast<double *>(dev + o_raw);
    a.part = reinterpret_cast<double *>(dev + o_part);
    a.marg = reinterpret_cast<double *>(dev + o_marg);
    a.err = reinterpret_cast<unsigned long long *>(dev + o_err);
    hipError_t e = hipMemcpyAsync(dev, host.data(), idx_bytes, hipMemcpyHostToDevice, s);
    // tables: small ones gathered into a bounded staging buffer (one copy per
    // 256 MB: a grid has ~10^5 factors, and a copy per factor costs ~3 us of
    // host time), tables of 64 MB and more copied straight from the model
    {
        constexpr size_t kStage = (size_t)256 << 20, kDirect = (size_t)64 << 20;
        std::vector<unsigned char> stage;
        size_t at = o_tabs;                                   // device offset of stage[0]
        auto flush = [&]() {
            if (!stage.empty() && e == hipSuccess) {
                e = hipMemcpyAsync(dev + at, stage.data(), stage.size(), hipMemcpyHostToDevice, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);      // stage is reused
            }
            at += stage.size();
            stage.clear();
        };
        for (int f = 0; f < nf && e == hipSuccess; ++f) {
            const size_t bytes = 8 * d.values[f].size();
            if (bytes >= kDirect) {
                flush();
                e = hipMemcpyAsync(dev + at, d.values[f].data(), bytes, hipMemcpyHostToDevice, s);
                at += bytes;
                continue;
            }
            if (stage.size() + bytes > kStage) flush();
            const unsigned char *p = reinterpret_cast<const unsigned char *>(d.values[f].data());
            stage.insert(stage.end(), p, p + bytes);
        }
        flush();
    }
    if (e == hipSuccess) e = hipMemsetAsync(a.err, 0, 8 * (size_t)kBpErrRing, s);
    if (e == hipSuccess) e = launch_bp_flood_init(a, s);
    int it_done = max_iter;
    std::vector<unsigned long long> chunk(kBpErrChunk);
    for (int c = 0; e == hipSuccess && (int64_t)c * kBpErrChunk < max_iter; ++c) {
        const int it0 = c * kBpErrChunk, it1 = std::min(max_iter, it0 + kBpErrChunk);
        unsigned long long *half = a.err + (c % 2) * kBpErrChunk;
        e = hipMemsetAsync(half, 0, 8 * (size_t)kBpErrChunk, s);
        for (int it = it0; it < it1 && e == hipSuccess; ++it) e = launch_bp_flood_iteration(a, it, s);
        if (e == hipSuccess) e = hipMemcpyAsync(chunk.data(), half, 8 * (size_t)(it1 - it0), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        bool done = false;
        for (int it = it0; e == hipSuccess && it < it1; ++it) {
            double m;
            std::memcpy(&m, &chunk[it - it0], 8);
            if (m < eps) {                        // graph.cpp:328
                it_done = it;
                done = true;
                break;
            }
        }
        if (done) break;
    }
    if (e == hipSuccess) e = launch_bp_flood_marginals(a, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out, a.marg, 8 * (size_t)marg_off[nv], hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("sum-product: ") + hipGetErrorString(e));
    if (iterations) *iterations = it_done;
    if (uptime_ms) *uptime_ms = now_ms() - t0;
    return BNPP_OK;
}

// BN::marginals with options["sum-product"] (model.cpp:313-317): loopy BP on
// the factor graph of the model's own factors (evidence is not used on this
// path, as in the reference), FactorGraph::update(max_iter, eps) then one
// marginal per variable (graph.cpp:256-403).  One workgroup runs the whole
// loop (bp.hip) unless the iteration's work calls for the multi-workgroup
// flood above.
int bnpp_sum_product(bnpp_ctx *ctx, const bnpp_model *m, int max_iter, double eps, double *out, int *iterations,
                     double *uptime_ms) {
    BNPP_GUARD_BEGIN
    if (!ctx || !m || !out) return set_err(BNPP_ERR_INVALID, "null argument");
    if (max_iter < 0) return set_err(BNPP_ERR_INVALID, "max_iter must be >= 0");
    const double t0 = now_ms();
    const ModelData &d = m->d;
    const int nv = (int)d.cards.size(), nf = (int)d.scopes.size();
    // one workgroup for the whole loop, or one launch per phase and iteration
    // (BNPP_BP_MODE=single|multi overrides the choice by work per iteration)
    bool big_table = false;
    double work = 0.0;
    {
        std::vector<double> deg(nv, 0.0);
        for (int f = 0; f < nf; ++f) {
            double size = 1.0;
            for (int v : d.scopes[f]) {
                size *= d.cards[v];
                deg[v] += 1.0;
            }
            const double m = (double)d.scopes[f].size();
            work += size * m * m;
            big_table |= size >= 2147483648.0;
        }
        for (int v = 0; v < nv; ++v) work += deg[v] * deg[v] * d.cards[v];
    }
    const char *mode = std::getenv("BNPP_BP_MODE");
    bool multi = big_table || work > kBpMultiWork;
    if (mode && !std::strcmp(mode, "multi")) multi = true;
    if (mode && !std::strcmp(mode, "single")) {
        if (big_table) return set_err(BNPP_ERR_UNSUPPORTED, "sum-product: one-workgroup loop needs tables < 2^31 entries");
        multi = false;
    }
    if (multi) return sum_product_flood(ctx, d, max_iter, eps, out, iterations, uptime_ms, t0);
    // host image of every input array, laid out as on the device
    std::vector<int32_t> f_edge_off(nf + 1, 0), edge_var, edge_fac, msg_off(1, 0), item_edge, v_edge_off(nv + 1, 0),
        v_edges, marg_off(nv + 1, 0);
    std::vector<uint32_t> edge_stride;
    std::vector<int64_t> tab_off(nf + 1, 0);
    for (int f = 0; f < nf; ++f) {
        const std::vector<int> &sc = d.scopes[f];
        int64_t size = 1;
        for (int v : sc) size *= d.cards[v];
        int64_t st = size;
        for (size_t j = 0; j < sc.size(); ++j) {
            st /= d.cards[sc[j]];
            const int e = (int)edge_var.size();
            edge_var.push_back(sc[j]);
            edge_fac.push_back(f);
            edge_stride.push_back((uint32_t)st);
            for (int x = 0; x < d.cards[sc[j]]; ++x) item_edge.push_back(e);
            msg_off.push_back(msg_off.back() + d.cards[sc[j]]);
            ++v_edge_off[sc[j] + 1];
        }
        f_edge_off[f + 1] = (int32_t)edge_var.size();
        tab_off[f + 1] = tab_off[f] + size;
    }
    const int ne = (int)edge_var.size(), nmsg = msg_off.back();
    std::vector<int32_t> cls[4], cls_items;
    for (int t = 0; t < nmsg; ++t) {
        const int e = item_edge[t];
        cls[bp_lane_class((tab_off[edge_fac[e] + 1] - tab_off[edge_fac[e]]) / d.cards[edge_var[e]])].push_back(t);
    }
    int32_t cls_off[5] = {0};
    for (int c = 0; c < 4; ++c) {
        cls_items.insert(cls_items.end(), cls[c].begin(), cls[c].end());
        cls_off[c + 1] = (int32_t)cls_items.size();
    }
    for (int v = 0; v < nv; ++v) {
        v_edge_off[v + 1] += v_edge_off[v];
        marg_off[v + 1] = marg_off[v] + d.cards[v];
    }
    v_edges.resize(ne);
    {
        std::vector<int32_t> fill(v_edge_off.begin(), v_edge_off.end() - 1);
        for (int e = 0; e < ne; ++e) v_edges[fill[edge_var[e]]++] = e;     // ascending edge = factor id
    }
    // one device block: inputs, then messages and outputs (256-B aligned pieces)
    std::vector<unsigned char> host;
    size_t off = 0;
    auto place = [&](size_t bytes) {
        const size_t o = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t o_cards = place(4 * (size_t)nv), o_tabs = place(8 * (size_t)tab_off[nf]),
                 o_tab_off = place(8 * (size_t)(nf + 1)), o_feo = place(4 * (size_t)(nf + 1)),
                 o_ev = place(4 * (size_t)ne), o_ef = place(4 * (size_t)ne), o_es = place(4 * (size_t)ne),
                 o_mo = place(4 * (size_t)(ne + 1)), o_ie = place(4 * (size_t)nmsg), o_veo = place(4 * (size_t)(nv + 1)),
                 o_ve = place(4 * (size_t)ne), o_mgo = place(4 * (size_t)(nv + 1)),
                 o_ci = place(4 * cls_items.size());
    const size_t in_bytes = off;
    const size_t o_v2f = place(8 * (size_t)nmsg), o_f2v = place(8 * (size_t)nmsg), o_raw = place(8 * (size_t)nmsg),
                 o_marg = place(8 * (size_t)marg_off[nv]), o_it = place(4);
    host.resize(in_bytes);
    auto put = [&](size_t o, const void *src, size_t bytes) {
        if (bytes) std::memcpy(host.data() + o, src, bytes);
    };
    std::vector<int32_t> cards32(d.cards.begin(), d.cards.end());
    put(o_cards, cards32.data(), 4 * (size_t)nv);
    for (int f = 0; f < nf; ++f) put(o_tabs + 8 * (size_t)tab_off[f], d.values[f].data(), 8 * d.values[f].size());
    put(o_tab_off, tab_off.data(), 8 * tab_off.size());
    put(o_feo, f_edge_off.data(), 4 * f_edge_off.size());
    put(o_ev, edge_var.data(), 4 * (size_t)ne);
    put(o_ef, edge_fac.data(), 4 * (size_t)ne);
    put(o_es, edge_stride.data(), 4 * (size_t)ne);
    put(o_mo, msg_off.data(), 4 * msg_off.size());
    put(o_ie, item_edge.data(), 4 * (size_t)nmsg);
    put(o_veo, v_edge_off.data(), 4 * v_edge_off.size());
    put(o_ve, v_edges.data(), 4 * (size_t)ne);
    put(o_mgo, marg_off.data(), 4 * marg_off.size());
    put(o_ci, cls_items.data(), 4 * cls_items.size());

    hipStream_t s = ctx->c.stream;
    unsigned char *dev = nullptr;
    if (hipSetDevice(ctx->c.device) != hipSuccess) return set_err(BNPP_ERR_HIP, "sum-product: hipSetDevice");
    if (hipMalloc(&dev, off) != hipSuccess) return set_err(BNPP_ERR_OOM, "sum-product: device allocation");
    struct Free {
        unsigned char *p;
        ~Free() { (void)hipFree(p); }
    } guard{dev};
    BpArgs a{};
    a.n_vars = nv;
    a.n_edges = ne;
    a.n_msg = nmsg;
    a.max_iter = max_iter;
    a.eps = eps;
    a.cards = reinterpret_cast<const int32_t *>(dev + o_cards);
    a.tables = reinterpret_cast<const double *>(dev + o_tabs);
    a.tab_off = reinterpret_cast<const int64_t *>(dev + o_tab_off);
    a.f_edge_off = reinterpret_cast<const int32_t *>(dev + o_feo);
    a.edge_var = reinterpret_cast<const int32_t *>(dev + o_ev);
    a.edge_fac = reinterpret_cast<const int32_t *>(dev + o_ef);
    a.edge_stride = reinterpret_cast<const uint32_t *>(dev + o_es);
    a.msg_off = reinterpret_cast<const int32_t *>(dev + o_mo);
    a.item_edge = reinterpret_cast<const int32_t *>(dev + o_ie);
    for (int c = 0; c < 5; ++c) a.cls_off[c] = cls_off[c];
    a.cls_items = reinterpret_cast<const int32_t *>(dev + o_ci);
    a.msgs_in_lds = nmsg <= kBpLdsMsgMax && !std::getenv("BNPP_BP_NO_LDS");
    a.v_edge_off = reinterpret_cast<const int32_t *>(dev + o_veo);
    a.v_edges = reinterpret_cast<const int32_t *>(dev + o_ve);
    a.marg_off = reinterpret_cast<const int32_t *>(dev + o_mgo);
    a.v2f = reinterpret_cast<double *>(dev + o_v2f);
    a.f2v = reinterpret_cast<double *>(dev + o_f2v);
    a.raw = reinterpret_cast<double *>(dev + o_raw);
    a.marg = reinterpret_cast<double *>(dev + o_marg);
    a.iterations = reinterpret_cast<int32_t *>(dev + o_it);
    int32_t it = 0;
    hipError_t e = hipMemcpyAsync(dev, host.data(), in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_sum_product(a, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out, a.marg, 8 * (size_t)marg_off[nv], hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&it, a.iterations, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_err(BNPP_ERR_HIP, std::string("sum-product: ") + hipGetErrorString(e));
    if (iterations) *iterations = it;
    if (uptime_ms) *uptime_ms = now_ms() - t0;
    return BNPP_OK;
    BNPP_GUARD_END
}

}  // extern "C"
