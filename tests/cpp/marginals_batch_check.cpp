// marginals_batch_check — bn::Model::marginals_batch through the C++ class
// mirror (include/bnpp/bn.hpp): every posterior marginal of every sample of a
// batched evidence file.  Prints one line per sample, "log10_z | p p p ...",
// %.17g, so tests/test_gpu_marginals_batch.py can compare the bits with the
// Python binding's.
//   marginals_batch_check <model.uai> <rows.evid> [target ...]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <vector>

#include "bnpp.h"
#include "bnpp/bn.hpp"

using namespace bn;

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: marginals_batch_check model.uai rows.evid [target ...]\n");
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
    bnpp_evidence_load_batch(argv[2], 0, 0, &n_ev, nullptr, &n_rows, nullptr);   // the sizes
    std::vector<int> ev_vars(n_ev > 0 ? n_ev : 1), flat((size_t)(n_ev > 0 ? n_ev : 1) * (size_t)(n_rows > 0 ? n_rows : 1));
    if (bnpp_evidence_load_batch(argv[2], n_ev, n_rows, &n_ev, ev_vars.data(), &n_rows, flat.data()) != BNPP_OK) return 3;
    const std::vector<unsigned> vars(ev_vars.begin(), ev_vars.begin() + n_ev);
    std::vector<std::vector<unsigned>> rows((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) rows[r].assign(flat.begin() + r * n_ev, flat.begin() + (r + 1) * n_ev);
    std::vector<unsigned> targets;
    for (int i = 3; i < argc; ++i) targets.push_back((unsigned)std::strtoul(argv[i], nullptr, 10));
    std::unordered_map<std::string, bool> opt{{"min-fill", true}};
    try {
        std::vector<double> lz;
        const std::vector<std::vector<double>> out = m->marginals_batch(vars, rows, targets, opt, &lz);
        for (size_t r = 0; r < out.size(); ++r) {
            std::printf("%.17g |", lz[r]);
            for (double v : out[r]) std::printf(" %.17g", v);
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
