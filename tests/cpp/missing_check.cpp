// missing_check — the missing-values overloads of bn::Model's batched calls
// through the C++ class mirror (include/bnpp/bn.hpp), on an evidence file whose
// samples observe differing variable sets (bnpp_evidence_load_batch_mv).
// Prints, %.17g, so that tests/test_gpu_missing.py can compare the bits with
// the Python binding's:
//   per sample "Z log10_z | marginals ...", then per sample "X assignment ..."
//   and "S sample ..." (one draw per row, seed 5), then per factor "C counts ..."
//   missing_check <model.uai> <rows.evid>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

#include "bnpp.h"
#include "bnpp/bn.hpp"

using namespace bn;

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: missing_check model.uai rows.evid\n");
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
    std::unordered_map<std::string, bool> opt{{"min-fill", true}};
    try {
        std::vector<double> lz;
        const std::vector<std::vector<double>> out = m->marginals_batch(vars, rows, partial, {}, opt, &lz);
        const std::vector<double> lz2 = m->partition_batch(vars, rows, partial, opt);
        for (size_t r = 0; r < out.size(); ++r) {
            if (lz[r] != lz2[r] && !(lz[r] != lz[r])) return 5;
            std::printf("Z %.17g |", lz[r]);
            for (double v : out[r]) std::printf(" %.17g", v);
            std::printf("\n");
        }
        for (const auto &x : m->mpe_batch(vars, rows, partial, opt)) {
            std::printf("X");
            for (unsigned v : x) std::printf(" %u", v);
            std::printf("\n");
        }
        for (const auto &x : m->sample_batch(vars, rows, partial, opt, 1, 5)) {
            std::printf("S");
            for (unsigned char v : x) std::printf(" %u", (unsigned)v);
            std::printf("\n");
        }
        for (const auto &t : m->expected_counts(vars, rows, partial, {}, opt)) {
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
