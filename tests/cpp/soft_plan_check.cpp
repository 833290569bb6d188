// soft_plan_check — the host side of soft evidence through the C ABI alone (no
// device is looked at): the five bnpp_plan_*_sv entries and the argument checks
// of the six _sv run entries with a null context, on the models given, for every
// single non-evidence variable of the first few soft and for all of those, with
// the first evidence variable partial and without, both dtypes, R = 1, 64 and
// automatic.  A stand-alone program with its own main, so that the host code can
// be checked under ASan and UBSan by linking it against
// `make -C bn-pp_amd sanitize`'s library.  Prints "OK <plans> <checks>".
//   soft_plan_check <model.uai> <n_ev> <v_1 ... v_n> [<model.uai> <n_ev> ...]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bnpp.h"

static int fail(const char *what, int rc) {
    std::fprintf(stderr, "%s: rc %d (%s)\n", what, rc, bnpp_last_error());
    return 1;
}

int main(int argc, char **argv) {
    long plans = 0, checks = 0;
    for (int a = 1; a + 1 < argc;) {
        bnpp_model *m = nullptr;
        if (bnpp_model_load_uai(argv[a], &m) != BNPP_OK) return fail("load", -1);
        const int n_ev = std::atoi(argv[a + 1]);
        if (n_ev < 1 || a + 2 + n_ev > argc) return fail("arguments", -1);
        std::vector<int> ev(n_ev);
        for (int j = 0; j < n_ev; ++j) ev[j] = std::atoi(argv[a + 2 + j]);
        a += 2 + n_ev;
        int nv = 0, nf = 0;
        bnpp_model_info(m, nullptr, &nv, &nf);
        std::vector<int> cards(nv);
        bnpp_model_cards(m, cards.data());
        std::vector<int> cand;                              // the first three variables that are no evidence
        for (int v = 0; v < nv && cand.size() < 3; ++v) {
            bool listed = false;
            for (int e : ev) listed = listed || e == v;
            if (!listed) cand.push_back(v);
        }
        const int nc = (int)cand.size();
        for (int which = 0; which <= nc; ++which) {         // candidate `which` soft; nc: all of them
            std::vector<int> soft = which == nc ? cand : std::vector<int>{cand[which]};
            const int n_soft = (int)soft.size();
            int ws = 0;
            for (int v : soft) ws += cards[v];
            for (int with_partial = 0; with_partial < 2; ++with_partial) {
                std::vector<unsigned char> part(n_ev, 0);
                part[0] = (unsigned char)with_partial;
                const unsigned char *pf = with_partial ? part.data() : nullptr;
                for (int dtype : {BNPP_F64, BNPP_F32})
                    for (int64_t R : {(int64_t)1, (int64_t)64, (int64_t)0}) {
                        double st[32];
                        std::vector<int64_t> rows(4096 * BNPP_PLAN_GROUP_FIELDS);
                        std::vector<int> mf(n_ev, -7), lf(n_soft, -7), off(nf + 1), bv(65536), kinds(nv);
                        int n = 0, rs[2], nrs = 0, nb = 0, flag = 0, rc;
                        if ((rc = bnpp_plan_batch_sv(m, n_ev, ev.data(), pf, n_soft, soft.data(), nullptr, BNPP_MIN_FILL,
                                                     nullptr, 0, -1, dtype, R, st, 10, rows.data(), 4096, &n, rs, &nrs,
                                                     mf.data(), lf.data())))
                            return fail("plan_batch_sv", rc);
                        for (int i = 0; i < n_soft; ++i)
                            if (lf[i] < 0 || lf[i] >= nf) return fail("lam_factor", lf[i]);
                        bool seen_key = false;
                        for (int g = 0; g < n; ++g)
                            seen_key = seen_key || rows[g * BNPP_PLAN_GROUP_FIELDS + 2] == (1 << 24) + 36864;
                        if (!seen_key) return fail("no weighted gather step in the groups", 0);
                        if ((rc = bnpp_plan_mpe_batch_sv(m, n_ev, ev.data(), pf, n_soft, soft.data(), nullptr, BNPP_MIN_FILL,
                                                         nullptr, 0, dtype, R, st, 16, rows.data(), 4096, &n, mf.data(),
                                                         lf.data())))
                            return fail("plan_mpe_batch_sv", rc);
                        if ((rc = bnpp_plan_sample_batch_sv(m, n_ev, ev.data(), pf, n_soft, soft.data(), nullptr,
                                                            BNPP_MIN_FILL, nullptr, 0, dtype, R, 3, st, 15, rows.data(), 4096,
                                                            &n, mf.data(), lf.data())))
                            return fail("plan_sample_batch_sv", rc);
                        if ((rc = bnpp_plan_counts_sv(m, n_ev, ev.data(), pf, n_soft, soft.data(), nullptr, BNPP_MIN_FILL,
                                                      nullptr, 0, dtype, R, st, 12, rows.data(), 4096, &n, off.data(),
                                                      bv.data(), (int)bv.size(), &nb, &flag, mf.data(), lf.data())))
                            return fail("plan_counts_sv", rc);
                        if ((rc = bnpp_plan_marginals_batch_sv(m, n_ev, ev.data(), pf, n_soft, soft.data(), nullptr,
                                                               BNPP_MIN_FILL, nullptr, 0, 0, nullptr, dtype, R, st, 18,
                                                               rows.data(), 4096, &n, kinds.data(), mf.data(), lf.data())))
                            return fail("plan_marginals_batch_sv", rc);
                        plans += 5;
                    }
                // the argument checks: two rows of valid evidence and likelihoods
                std::vector<int> vals(2 * n_ev, 0);
                std::vector<double> lik(2 * ws, 0.5), out(65536);
                std::vector<int> x(2 * nv);
                std::vector<unsigned char> s(2 * nv);
                int target = 0;                             // the posterior's: a variable neither evidence nor soft
                for (bool listed = true; listed; target += listed) {
                    listed = false;
                    for (int v : ev) listed = listed || v == target;
                    for (int v : soft) listed = listed || v == target;
                }
                // every run entry fails (no context), each with `must` in its message
                auto run_all = [&](int ns, const int *sv, const double *lk, const char *must) {
                    bool good = true;
                    auto seen = [&](int rc) {
                        ++checks;
                        good = good && rc != BNPP_OK && std::strstr(bnpp_last_error(), must) != nullptr;
                    };
                    seen(bnpp_partition_batch_sv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, ns, sv, lk, BNPP_MIN_FILL,
                                                 nullptr, 0, BNPP_F64, 0, out.data(), nullptr, nullptr));
                    seen(bnpp_mpe_batch_sv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, ns, sv, lk, BNPP_MIN_FILL, nullptr,
                                           0, BNPP_F64, 0, out.data(), x.data(), nullptr));
                    seen(bnpp_sample_batch_sv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, ns, sv, lk, BNPP_MIN_FILL,
                                              nullptr, 0, BNPP_F64, 0, 1, 0, 1, 7, s.data(), nullptr, nullptr, nullptr));
                    seen(bnpp_expected_counts_sv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, ns, sv, lk, nullptr,
                                                 BNPP_MIN_FILL, nullptr, 0, BNPP_F64, 0, out.data(), nullptr, nullptr,
                                                 nullptr));
                    seen(bnpp_marginals_batch_sv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, ns, sv, lk, BNPP_MIN_FILL,
                                                 nullptr, 0, 0, nullptr, BNPP_F64, 0, out.data(), nullptr, nullptr));
                    seen(bnpp_posterior_batch_sv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, ns, sv, lk, BNPP_MIN_FILL,
                                                 target, BNPP_F64, 0, out.data(), nullptr));
                    return good;
                };
                // valid rows get as far as the missing context (or, batched MPE and sampling, the missing device)
                if (!run_all(n_soft, soft.data(), lik.data(), "e")) return fail("valid rows must reach the context check", 0);
                if (std::strstr(bnpp_last_error(), "row ")) return fail("valid rows were refused", 0);
                for (double bad : {(double)NAN, (double)INFINITY, -0.25}) {
                    lik[ws + ws - 1] = bad;                 // the last likelihood of row 1
                    if (!run_all(n_soft, soft.data(), lik.data(), "row 1")) return fail("a bad likelihood must name the row", 0);
                    lik[ws + ws - 1] = 0.5;
                }
                std::vector<int> both = soft;               // an evidence variable listed as soft, a duplicate, a bad id
                both.push_back(ev[0]);
                std::vector<double> wide(2 * (ws + cards[ev[0]] + 64), 0.5);
                if (!run_all(n_soft + 1, both.data(), wide.data(), "both")) return fail("evidence and soft", 0);
                both.back() = soft[0];
                if (!run_all(n_soft + 1, both.data(), wide.data(), "twice")) return fail("a soft variable twice", 0);
                both.back() = nv;
                if (!run_all(n_soft + 1, both.data(), wide.data(), "out of range")) return fail("a soft id out of range", 0);
            }
        }
        bnpp_model_free(m);
    }
    std::printf("OK %ld %ld\n", plans, checks);
    return 0;
}
