// missing_plan_check — the host side of missing values through the C ABI alone
// (no device is looked at): the five bnpp_plan_*_mv entries and the argument
// checks of the six _mv run entries with a null context, on the models given,
// for every single evidence variable partial and for all of them, both dtypes,
// R = 1, 64 and automatic.  A stand-alone program with its own main, so that the
// host code can be checked under ASan and UBSan by linking it against
// `make -C bn-pp_amd sanitize`'s library.  Prints "OK <plans> <checks>".
//   missing_plan_check <model.uai> <n_ev> <v_1 ... v_n> [<model.uai> <n_ev> ...]
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
        for (int which = 0; which <= n_ev; ++which) {      // variable `which` partial; n_ev: all of them
            std::vector<unsigned char> part(n_ev, which == n_ev ? 1 : 0);
            if (which < n_ev) part[which] = 1;
            for (int dtype : {BNPP_F64, BNPP_F32})
                for (int64_t R : {(int64_t)1, (int64_t)64, (int64_t)0}) {
                    double st[32];
                    std::vector<int64_t> rows(4096 * BNPP_PLAN_GROUP_FIELDS);
                    std::vector<int> mf(n_ev, -7), off(nf + 1), bv(65536), kinds(nv);
                    int n = 0, rs[2], nrs = 0, nb = 0, flag = 0, rc;
                    if ((rc = bnpp_plan_batch_mv(m, n_ev, ev.data(), part.data(), BNPP_MIN_FILL, nullptr, 0, -1, dtype, R, st,
                                                 10, rows.data(), 4096, &n, rs, &nrs, mf.data())))
                        return fail("plan_batch_mv", rc);
                    for (int j = 0; j < n_ev; ++j)
                        if (mf[j] < -1 || mf[j] >= nf || (!part[j] && mf[j] != -1)) return fail("mask_factor", mf[j]);
                    if ((rc = bnpp_plan_mpe_batch_mv(m, n_ev, ev.data(), part.data(), BNPP_MIN_FILL, nullptr, 0, dtype, R, st,
                                                     16, rows.data(), 4096, &n, mf.data())))
                        return fail("plan_mpe_batch_mv", rc);
                    if ((rc = bnpp_plan_sample_batch_mv(m, n_ev, ev.data(), part.data(), BNPP_MIN_FILL, nullptr, 0, dtype, R,
                                                        3, st, 15, rows.data(), 4096, &n, mf.data())))
                        return fail("plan_sample_batch_mv", rc);
                    if ((rc = bnpp_plan_counts_mv(m, n_ev, ev.data(), part.data(), BNPP_MIN_FILL, nullptr, 0, dtype, R, st, 12,
                                                  rows.data(), 4096, &n, off.data(), bv.data(), (int)bv.size(), &nb, &flag,
                                                  mf.data())))
                        return fail("plan_counts_mv", rc);
                    if ((rc = bnpp_plan_marginals_batch_mv(m, n_ev, ev.data(), part.data(), BNPP_MIN_FILL, nullptr, 0, 0,
                                                           nullptr, dtype, R, st, 18, rows.data(), 4096, &n, kinds.data(),
                                                           mf.data())))
                        return fail("plan_marginals_batch_mv", rc);
                    plans += 5;
                }
            // the argument checks: two rows, the second one's partial entries missing
            std::vector<int> vals(2 * n_ev, 0);
            for (int j = 0; j < n_ev; ++j)
                if (part[j]) vals[n_ev + j] = BNPP_MISSING;
            std::vector<double> out(65536);
            std::vector<int> x(2 * nv);
            std::vector<unsigned char> s(2 * nv);
            int target = 0;                                         // the posterior's: the first variable not listed
            for (bool listed = true; listed; target += listed) {
                listed = false;
                for (int v : ev) listed = listed || v == target;
            }
            // every run entry fails (no context), each with `must` in its message
            auto run_all = [&](const unsigned char *pf, const char *must) {
                bool good = true;
                auto seen = [&](int rc) {
                    ++checks;
                    good = good && rc != BNPP_OK && std::strstr(bnpp_last_error(), must) != nullptr;
                };
                seen(bnpp_partition_batch_mv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, BNPP_MIN_FILL, nullptr, 0,
                                             BNPP_F64, 0, out.data(), nullptr, nullptr));
                seen(bnpp_mpe_batch_mv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, BNPP_MIN_FILL, nullptr, 0, BNPP_F64, 0,
                                       out.data(), x.data(), nullptr));
                seen(bnpp_sample_batch_mv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, BNPP_MIN_FILL, nullptr, 0, BNPP_F64,
                                          0, 1, 0, 1, 7, s.data(), nullptr, nullptr, nullptr));
                seen(bnpp_expected_counts_mv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, nullptr, BNPP_MIN_FILL, nullptr,
                                             0, BNPP_F64, 0, out.data(), nullptr, nullptr, nullptr));
                seen(bnpp_marginals_batch_mv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, BNPP_MIN_FILL, nullptr, 0, 0,
                                             nullptr, BNPP_F64, 0, out.data(), nullptr, nullptr));
                seen(bnpp_posterior_batch_mv(nullptr, m, n_ev, ev.data(), 2, vals.data(), pf, BNPP_MIN_FILL, target, BNPP_F64,
                                             0, out.data(), nullptr));
                return good;
            };
            // valid rows get as far as the missing context (or, batched MPE and sampling, the missing device)
            if (!run_all(part.data(), "e")) return fail("valid rows must reach the context check", 0);
            if (std::strstr(bnpp_last_error(), "row ")) return fail("valid rows were refused", 0);
            if (!run_all(nullptr, "row 1")) return fail("-1 without the declaration must name the row", 0);
            for (int j = 0; j < n_ev; ++j)
                if (part[j]) {
                    vals[j] = cards[ev[j]];                                 // the card in a partial column
                    if (!run_all(part.data(), "row 0")) return fail("the card in a partial column", 0);
                    vals[j] = -2;
                    if (!run_all(part.data(), "row 0")) return fail("-2 in a partial column", 0);
                    vals[j] = 0;
                }
        }
        bnpp_model_free(m);
    }
    std::printf("OK %ld %ld\n", plans, checks);
    return 0;
}
