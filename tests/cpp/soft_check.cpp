// soft_check — the soft-evidence overloads of bn::Model's batched calls through
// the C++ class mirror (include/bnpp/bn.hpp), on an evidence file whose samples
// observe differing variable sets (bnpp_evidence_load_batch_mv) and a likelihood
// file (bnpp_likelihood_load) with one row per sample.  Prints, %.17g, so that
// tests/test_gpu_soft.py can compare the bits with the Python binding's:
//   per sample "Z log10_z | marginals ...", then per sample "X assignment ...",
//   "S sample ..." (one draw per row, seed 5) and "P posterior of variable 1 ...",
//   then per factor "C counts ..."
//   soft_check <model.uai> <rows.evid> <rows.lik>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "bnpp.h"
#include "bnpp/bn.hpp"

using namespace bn;

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: soft_check model.uai rows.evid rows.lik\n");
        return 1;
    }
    if (!bnpp_abi_matches()) {
        std::fprintf(stderr, "libbnpp ABI version differs from include/bnpp.h\n");
        return 1;
    }
    std::string path = argv[1];
    BN *m = nullptr;
    if (read_uai_model(path, &m)) return 2;
    int n_ev = 0;
    int64_t n_rows = 0;
    bnpp_evidence_load_batch_mv(argv[2], 0, 0, &n_ev, nullptr, &n_rows, nullptr, nullptr);   // the sizes
    std::vector<int> ev_vars(n_ev > 0 ? n_ev : 1), flat((size_t)(n_ev > 0 ? n_ev : 1) * (size_t)(n_rows > 0 ? n_rows : 1));
    std::vector<unsigned char> partial((size_t)(n_ev > 0 ? n_ev : 1), 0);
    if (bnpp_evidence_load_batch_mv(argv[2], n_ev, n_rows, &n_ev, ev_vars.data(), &n_rows, flat.data(), partial.data()) !=
        BNPP_OK)
        return 3;
    partial.resize((size_t)n_ev);
    const std::vector<unsigned> vars(ev_vars.begin(), ev_vars.begin() + n_ev);
    std::vector<std::vector<int>> rows((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) rows[r].assign(flat.begin() + r * n_ev, flat.begin() + (r + 1) * n_ev);
    SoftEvidence soft;
    {
        bnpp_model *h = nullptr;
        if (bnpp_model_load_uai(argv[1], &h) != BNPP_OK) return 6;
        int n_soft = 0, nv = 0;
        int64_t n_lik = 0;
        bnpp_model_info(h, nullptr, &nv, nullptr);
        std::vector<int> cards((size_t)nv), ids((size_t)nv);
        bnpp_model_cards(h, cards.data());
        bnpp_likelihood_load(h, argv[3], nv, 0, &n_soft, ids.data(), &n_lik, nullptr);        // the sizes and ids
        int64_t ws = 0;
        for (int i = 0; i < n_soft; ++i) ws += cards[ids[i]];
        std::vector<double> lik((size_t)(n_lik * ws > 0 ? n_lik * ws : 1));
        const int rc = bnpp_likelihood_load(h, argv[3], nv, n_lik * ws, &n_soft, ids.data(), &n_lik, lik.data());
        bnpp_model_free(h);
        if (rc != BNPP_OK || n_lik != n_rows) return 7;
        soft.vars.assign(ids.begin(), ids.begin() + n_soft);
        for (int64_t r = 0; r < n_rows; ++r) soft.lik.emplace_back(lik.begin() + r * ws, lik.begin() + (r + 1) * ws);
    }
    std::unordered_map<std::string, bool> opt{{"min-fill", true}};
    // rows of likelihoods shorter than the soft variables' values, and a soft id out of range, are refused
    // before anything is read
    for (int bad = 0; bad < 2; ++bad) {
        SoftEvidence wrong = soft;
        if (bad == 0) wrong.lik.back().pop_back();
        else wrong.vars.back() = 1000000;
        try {
            m->partition_batch(vars, rows, partial, wrong, opt);
            std::fprintf(stderr, "a malformed SoftEvidence was accepted\n");
            return 8;
        } catch (const std::runtime_error &e) {
            if (!std::strstr(e.what(), bad == 0 ? "likelihoods" : "out of range")) return 9;
        }
    }
    try {
        std::vector<double> lz;
        const std::vector<std::vector<double>> out = m->marginals_batch(vars, rows, partial, soft, {}, opt, &lz);
        const std::vector<double> lz2 = m->partition_batch(vars, rows, partial, soft, opt);
        for (size_t r = 0; r < out.size(); ++r) {
            if (lz[r] != lz2[r] && !(lz[r] != lz[r])) return 5;
            std::printf("Z %.17g |", lz[r]);
            for (double v : out[r]) std::printf(" %.17g", v);
            std::printf("\n");
        }
        for (const auto &x : m->mpe_batch(vars, rows, partial, soft, opt)) {
            std::printf("X");
            for (unsigned v : x) std::printf(" %u", v);
            std::printf("\n");
        }
        for (const auto &x : m->sample_batch(vars, rows, partial, soft, opt, 1, 5)) {
            std::printf("S");
            for (unsigned char v : x) std::printf(" %u", (unsigned)v);
            std::printf("\n");
        }
        for (const auto &t : m->posterior_batch(vars, rows, partial, soft, 1, opt)) {
            std::printf("P");
            for (double v : t) std::printf(" %.17g", v);
            std::printf("\n");
        }
        for (const auto &t : m->expected_counts(vars, rows, partial, soft, {}, opt)) {
            std::printf("C");
            for (double v : t) std::printf(" %.17g", v);
            std::printf("\n");
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        delete m;
        return 4;
    }
    delete m;
    return 0;
}
