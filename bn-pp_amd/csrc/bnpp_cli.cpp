// bnpp — command-line front end with the reference's task flags (bn.cpp:136-258,
// mn.cpp:135-155): -pr / -mar, -mf / -wmf / -md, -sp, -v, plus -f32, -mar-tree
// and -uai <base> (UAI-competition result files <base>.PR / <base>.MAR, the
// format of the reference's models/markovnets/*.PR / *.MAR fixtures: log10 Z;
// per variable its card and probabilities, evidence variables one-hot).
// -mpe (no reference counterpart): the most probable explanation, log10 of its
// value and the assignment; with -uai, <base>.MPE ("MPE", then "N x_0 .. x_{N-1}").
// -sample N [-seed S] (no reference counterpart): N exact joint samples of the
// posterior, log10 Z and the first sample; with -uai, <base>.SAMPLES ("SAMPLES",
// then "N n_vars", then one line of n_vars values per sample).
// -pr-batch / -post-batch T (no reference counterpart): the evidence file holds
// any number of samples over one variable set (bnpp_evidence_load_batch); log10 Z
// per sample, or P(T | sample); with -uai, <base>.PR ("PR", the sample count,
// one log10 Z per line) or <base>.MAR ("MAR", the sample count, then per sample
// "1 card(T) p_0 .. p_{card-1}").
// -mpe-batch (no reference counterpart): the most probable completion of every
// sample of the evidence file (bnpp_mpe_batch), one line per sample; with -uai,
// <base>.MPE ("MPE", the sample count, then per sample "N x_0 .. x_{N-1}").
// -sample-batch K [-seed S] (no reference counterpart): K exact joint samples of
// the posterior of every sample of the evidence file (bnpp_sample_batch), row r
// drawing at the global indices r * K .. r * K + K - 1; with -uai,
// <base>.SAMPLES ("SAMPLES", then "n_rows K n_vars", then one line of n_vars
// values per sample, rows outermost).
// -counts (no reference counterpart): the expected sufficient statistics of the
// evidence file's samples (bnpp_expected_counts); prints the total log10-
// likelihood of the possible samples and n_impossible; with -uai, <base>.COUNTS
// ("COUNTS", the factor count, then per factor "size v_0 .. v_{size-1}", %.17g).
// -missing beside a batch mode: the samples of the evidence file may observe
// differing variable sets (bnpp_evidence_load_batch_mv); every variable some
// sample lacks is declared partial and the _mv entries run.  Outputs as without it.
// -soft rows.lik beside a batch mode: soft evidence (bnpp_likelihood_load, the
// _sv entries) -- the file names the soft variables and gives every sample of
// the evidence file one row of likelihoods.  It combines with -missing.
// -mar-batch (no reference counterpart): every posterior marginal of every
// sample of the evidence file (bnpp_marginals_batch), one line per sample; with
// -uai, <base>.MAR ("MAR", the sample count, then per sample the UAI MAR line
// "n_vars card_0 p.. card_1 p.. ...", %.17g, evidence variables one-hot).
// BAYES files print like `bn` (raw Z), MARKOV files like `mn` (log10 Z).
// -ve is accepted and, as in the reference, changes nothing here: bn reads it
// only for REPL queries (bn.cpp:346); partition / marginals always run VE
// (model.cpp:275, 319).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bnpp/bn.hpp"
#include "../../include/bnpp.h"

int main(int argc, char **argv) {
    std::unordered_map<std::string, bool> options;
    std::vector<std::string> positional;
    std::string uai_out, soft_path;
    unsigned long long n_samples = 0, n_per_row = 0, seed = 0;
    unsigned post_target = 0;
    for (int i = 1; i < argc; ++i) {
        std::string p(argv[i]);
        if (p == "-uai" && i + 1 < argc) uai_out = argv[++i];
        else if (p == "-pr") options["partition"] = true;
        else if (p == "-mar") options["marginals"] = true;
        else if (p == "-mpe") options["mpe"] = true;
        else if (p == "-pr-batch") options["partition-batch"] = true;
        else if (p == "-mpe-batch") options["mpe-batch"] = true;
        else if (p == "-counts") options["counts"] = true;
        else if (p == "-mar-batch") options["marginals-batch"] = true;
        else if (p == "-missing") options["missing"] = true;
        else if (p == "-soft" && i + 1 < argc) soft_path = argv[++i];
        else if (p == "-post-batch" && i + 1 < argc) { options["posterior-batch"] = true; post_target = (unsigned)std::strtoul(argv[++i], nullptr, 10); }
        else if (p == "-sample" && i + 1 < argc) { options["sample"] = true; n_samples = std::strtoull(argv[++i], nullptr, 10); }
        else if (p == "-sample-batch" && i + 1 < argc) { options["sample-batch"] = true; n_per_row = std::strtoull(argv[++i], nullptr, 10); }
        else if (p == "-seed" && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
        else if (p == "-mar-tree") { options["marginals"] = true; options["bucket-tree"] = true; }
        else if (p == "-ve") options["variable-elimination"] = true;
        else if (p == "-sp") options["sum-product"] = true;      // bn.cpp:177-178: loopy BP marginals
        else if (p == "-mf") options["min-fill"] = true;
        else if (p == "-wmf") options["weighted-min-fill"] = true;
        else if (p == "-md") options["min-degree"] = true;
        else if (p == "-f32") options["fp32"] = true;
        else if (p == "-v") options["verbose"] = true;
        else if (p == "-h") options["help"] = true;
        else if (p[0] == '-') { std::cerr << "Error: invalid option `" << p << "'." << std::endl; return -1; }
        else positional.push_back(p);
    }
    if (!soft_path.empty() && !(options["partition-batch"] || options["posterior-batch"] || options["counts"] ||
                                options["mpe-batch"] || options["sample-batch"] || options["marginals-batch"])) {
        std::cerr << "Error: -soft needs a batch mode (-pr-batch, -post-batch, -mpe-batch, -sample-batch, -counts, -mar-batch)." << std::endl;
        return -1;
    }
    if (positional.empty() || options["help"]) {
        std::cout << "usage: " << argv[0] << " /path/to/model.uai [/path/to/evidence.uai.evid] -pr|-mar|-mar-tree|-mpe|-sample N [-seed S]|-pr-batch|-post-batch T|-mpe-batch|-sample-batch K [-seed S]|-counts|-mar-batch [-missing] [-soft rows.lik] [-sp] [-mf|-wmf|-md] [-f32] [-uai base]" << std::endl;
        return positional.empty() ? 1 : 0;
    }
    bnpp_model *probe = nullptr;
    if (bnpp_model_load_uai(positional[0].c_str(), &probe) != BNPP_OK) {
        std::cerr << "Error: " << bnpp_last_error() << std::endl;
        return -1;
    }
    int is_bayes = 0;
    bnpp_model_info(probe, &is_bayes, nullptr, nullptr);
    bnpp_model_free(probe);
    std::unordered_map<unsigned, unsigned> evidence;
    if (positional.size() > 1 && bn::read_uai_evidence(positional[1], evidence)) return -2;
    bn::Model *model = nullptr;
    if (is_bayes) {
        bn::BN *m = nullptr;
        if (bn::read_uai_model(positional[0], &m)) return -1;
        model = m;
    } else {
        bn::MN *m = nullptr;
        if (bn::read_uai_model(positional[0], &m)) return -1;
        model = m;
    }
    try {
        double uptime = 0;
        if (options["partition"]) {
            double lz = 0;
            if (is_bayes) {
                double p = model->partition(evidence, options, uptime);
                std::cout << ">> Partition = " << p << std::endl;
                lz = std::log10(p);
            } else {
                lz = model->log10_partition(evidence, options, uptime);
                std::cout << "Partition = " << lz << std::endl << std::endl;
            }
            std::cout << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
            if (!uai_out.empty()) {
                FILE *f = std::fopen((uai_out + ".PR").c_str(), "w");
                if (!f) throw std::runtime_error("cannot write " + uai_out + ".PR");
                std::fprintf(f, "PR\n1\n%g\n", lz);
                std::fclose(f);
            }
        }
        if (options["marginals"]) {
            std::vector<const bn::Factor *> marg = model->marginals(evidence, options, uptime);
            std::cout << ">> Marginals:" << std::endl;
            for (auto pf : marg) std::cout << *pf << std::endl;
            std::cout << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
            if (!uai_out.empty()) {
                FILE *f = std::fopen((uai_out + ".MAR").c_str(), "w");
                if (!f) throw std::runtime_error("cannot write " + uai_out + ".MAR");
                std::fprintf(f, "MAR\n1\n%zu\n", marg.size());
                const std::vector<bn::Variable *> &vars = model->variables();
                for (size_t i = 0; i < marg.size(); ++i) {
                    const unsigned k = vars[i]->size();
                    std::fprintf(f, "%u", k);
                    auto ev = evidence.find(vars[i]->id());
                    for (unsigned x = 0; x < k; ++x) {
                        // an evidence variable's marginal is a width-0 factor (model.cpp:333): one-hot here
                        const double p = ev != evidence.end() && marg[i]->width() == 0 ? (x == ev->second ? 1.0 : 0.0)
                                                                                      : (*marg[i])[x];
                        std::fprintf(f, " %g", p);
                    }
                    std::fprintf(f, "\n");
                }
                std::fclose(f);
            }
            for (auto pf : marg) delete pf;
        }
        if (options["mpe"]) {
            double lv = 0;
            const std::vector<unsigned> x = model->mpe(evidence, options, &lv, &uptime);
            std::cout << ">> MPE log10 value = " << lv << std::endl << ">> MPE assignment:";
            for (unsigned v : x) std::cout << " " << v;
            std::cout << std::endl << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
            if (!uai_out.empty()) {
                FILE *f = std::fopen((uai_out + ".MPE").c_str(), "w");
                if (!f) throw std::runtime_error("cannot write " + uai_out + ".MPE");
                std::fprintf(f, "MPE\n%zu", x.size());
                for (unsigned v : x) std::fprintf(f, " %u", v);
                std::fprintf(f, "\n");
                std::fclose(f);
            }
        }
        if (options["sample"]) {
            double lz = 0;
            const std::vector<std::vector<unsigned char>> xs = model->sample(evidence, options, n_samples, seed, &lz, &uptime);
            std::cout << ">> log10 Z = " << lz << std::endl << ">> First of " << xs.size() << " samples:";
            if (!xs.empty())
                for (unsigned char v : xs[0]) std::cout << " " << (unsigned)v;
            std::cout << std::endl << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
            if (!uai_out.empty()) {
                FILE *f = std::fopen((uai_out + ".SAMPLES").c_str(), "w");
                if (!f) throw std::runtime_error("cannot write " + uai_out + ".SAMPLES");
                std::fprintf(f, "SAMPLES\n%zu %zu\n", xs.size(), model->variables().size());
                for (const auto &x : xs) {
                    for (size_t v = 0; v < x.size(); ++v) std::fprintf(f, v ? " %u" : "%u", (unsigned)x[v]);
                    std::fprintf(f, "\n");
                }
                std::fclose(f);
            }
        }
        if (options["partition-batch"] || options["posterior-batch"] || options["counts"] || options["mpe-batch"] ||
            options["sample-batch"] || options["marginals-batch"]) {
            if (positional.size() < 2)
                throw std::runtime_error("-pr-batch / -post-batch / -mpe-batch / -sample-batch / -counts / -mar-batch need an evidence file");
            int n_ev = 0;
            int64_t n_rows = 0;
            // -missing: the samples may observe differing variable sets; every variable some sample lacks is partial
            const bool missing = options["missing"];
            if (missing) bnpp_evidence_load_batch_mv(positional[1].c_str(), 0, 0, &n_ev, nullptr, &n_rows, nullptr, nullptr);
            else bnpp_evidence_load_batch(positional[1].c_str(), 0, 0, &n_ev, nullptr, &n_rows, nullptr);   // the sizes
            std::vector<int> ev_vars(n_ev > 0 ? n_ev : 1), flat((size_t)(n_ev > 0 ? n_ev : 1) * (size_t)(n_rows > 0 ? n_rows : 1));
            std::vector<unsigned char> partial;             // empty: the calls without missing values
            if (missing) partial.assign((size_t)(n_ev > 0 ? n_ev : 1), 0);
            if ((missing ? bnpp_evidence_load_batch_mv(positional[1].c_str(), n_ev, n_rows, &n_ev, ev_vars.data(), &n_rows,
                                                       flat.data(), partial.data())
                         : bnpp_evidence_load_batch(positional[1].c_str(), n_ev, n_rows, &n_ev, ev_vars.data(), &n_rows,
                                                    flat.data())) != BNPP_OK)
                throw std::runtime_error(bnpp_last_error());
            if (missing) partial.resize((size_t)n_ev);
            const std::vector<unsigned> vars(ev_vars.begin(), ev_vars.begin() + n_ev);
            std::vector<std::vector<int>> rows((size_t)n_rows);
            for (int64_t r = 0; r < n_rows; ++r) rows[r].assign(flat.begin() + r * n_ev, flat.begin() + (r + 1) * n_ev);
            // -soft: the soft variables and one row of likelihoods per sample
            bn::SoftEvidence soft;
            if (!soft_path.empty()) {
                bnpp_model *h = nullptr;
                if (bnpp_model_load_uai(positional[0].c_str(), &h) != BNPP_OK) throw std::runtime_error(bnpp_last_error());
                int n_soft = 0, nv = 0;
                int64_t n_lik = 0;
                bnpp_model_info(h, nullptr, &nv, nullptr);
                std::vector<int> cards((size_t)(nv > 0 ? nv : 1)), ids((size_t)(nv > 0 ? nv : 1));
                bnpp_model_cards(h, cards.data());
                // the sizes and ids: BNPP_ERR_INVALID ("larger than cap") is the answer expected here
                if (bnpp_likelihood_load(h, soft_path.c_str(), nv, 0, &n_soft, ids.data(), &n_lik, nullptr) == BNPP_ERR_IO) {
                    bnpp_model_free(h);
                    throw std::runtime_error(bnpp_last_error());
                }
                int64_t ws = 0;
                for (int i = 0; i < n_soft && i < nv; ++i) ws += cards[ids[i]];
                std::vector<double> lik((size_t)(n_lik * ws > 0 ? n_lik * ws : 1));
                const int rc = bnpp_likelihood_load(h, soft_path.c_str(), nv, n_lik * ws, &n_soft, ids.data(), &n_lik, lik.data());
                bnpp_model_free(h);
                if (rc != BNPP_OK) throw std::runtime_error(bnpp_last_error());
                if (n_lik != n_rows)
                    throw std::runtime_error("-soft: " + std::to_string(n_lik) + " rows of likelihoods for " +
                                             std::to_string(n_rows) + " evidence rows");
                soft.vars.assign(ids.begin(), ids.begin() + n_soft);
                soft.lik.resize((size_t)n_rows);
                for (int64_t r = 0; r < n_rows; ++r) soft.lik[r].assign(lik.begin() + r * ws, lik.begin() + (r + 1) * ws);
            }
            if (options["partition-batch"]) {
                const std::vector<double> lz = model->partition_batch(vars, rows, partial, soft, options, nullptr, &uptime);
                std::cout << ">> log10 Z of " << lz.size() << " evidence rows:";
                for (size_t r = 0; r < lz.size() && r < 8; ++r) std::cout << " " << lz[r];
                std::cout << (lz.size() > 8 ? " ..." : "") << std::endl << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
                if (!uai_out.empty()) {
                    FILE *f = std::fopen((uai_out + ".PR").c_str(), "w");
                    if (!f) throw std::runtime_error("cannot write " + uai_out + ".PR");
                    std::fprintf(f, "PR\n%zu\n", lz.size());
                    for (double v : lz) std::fprintf(f, "%.17g\n", v);
                    std::fclose(f);
                }
            }
            if (options["mpe-batch"]) {
                std::vector<double> lv;
                const std::vector<std::vector<unsigned>> xs = model->mpe_batch(vars, rows, partial, soft, options, &lv, &uptime);
                for (size_t r = 0; r < xs.size(); ++r) {
                    std::cout << ">> MPE row " << r << " log10 value = " << lv[r] << " assignment:";
                    for (unsigned v : xs[r]) std::cout << " " << v;
                    std::cout << std::endl;
                }
                std::cout << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
                if (!uai_out.empty()) {
                    FILE *f = std::fopen((uai_out + ".MPE").c_str(), "w");
                    if (!f) throw std::runtime_error("cannot write " + uai_out + ".MPE");
                    std::fprintf(f, "MPE\n%zu\n", xs.size());
                    for (const auto &x : xs) {
                        std::fprintf(f, "%zu", x.size());
                        for (unsigned v : x) std::fprintf(f, " %u", v);
                        std::fprintf(f, "\n");
                    }
                    std::fclose(f);
                }
            }
            if (options["sample-batch"]) {
                std::vector<double> lz;
                const std::vector<std::vector<unsigned char>> xs =
                    model->sample_batch(vars, rows, partial, soft, options, n_per_row, seed, &lz, &uptime);
                std::cout << ">> " << n_per_row << " samples for each of " << rows.size() << " evidence rows; log10 Z:";
                for (size_t r = 0; r < lz.size() && r < 8; ++r) std::cout << " " << lz[r];
                std::cout << (lz.size() > 8 ? " ..." : "") << std::endl << ">> First sample:";
                if (!xs.empty())
                    for (unsigned char v : xs[0]) std::cout << " " << (unsigned)v;
                std::cout << std::endl << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
                if (!uai_out.empty()) {
                    FILE *f = std::fopen((uai_out + ".SAMPLES").c_str(), "w");
                    if (!f) throw std::runtime_error("cannot write " + uai_out + ".SAMPLES");
                    std::fprintf(f, "SAMPLES\n%zu %llu %zu\n", rows.size(), n_per_row, model->variables().size());
                    for (const auto &x : xs) {
                        for (size_t v = 0; v < x.size(); ++v) std::fprintf(f, v ? " %u" : "%u", (unsigned)x[v]);
                        std::fprintf(f, "\n");
                    }
                    std::fclose(f);
                }
            }
            if (options["counts"]) {
                std::vector<double> lz;
                long long n_impossible = 0;
                const std::vector<std::vector<double>> counts =
                    model->expected_counts(vars, rows, partial, soft, {}, options, &lz, &n_impossible, &uptime);
                double ll = 0;
                for (double v : lz)
                    if (std::isfinite(v)) ll += v;
                std::printf(">> log10-likelihood of %zu evidence rows = %.17g\n>> n_impossible %lld\n", lz.size(), ll, n_impossible);
                std::cout << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
                if (!uai_out.empty()) {
                    FILE *f = std::fopen((uai_out + ".COUNTS").c_str(), "w");
                    if (!f) throw std::runtime_error("cannot write " + uai_out + ".COUNTS");
                    std::fprintf(f, "COUNTS\n%zu\n", counts.size());
                    for (const auto &t : counts) {
                        std::fprintf(f, "%zu", t.size());
                        for (double v : t) std::fprintf(f, " %.17g", v);
                        std::fprintf(f, "\n");
                    }
                    std::fclose(f);
                }
            }
            if (options["marginals-batch"]) {
                std::vector<double> lz;
                const std::vector<std::vector<double>> marg = model->marginals_batch(vars, rows, partial, soft, {}, options, &lz, &uptime);
                const std::vector<bn::Variable *> &mv = model->variables();
                for (size_t r = 0; r < marg.size(); ++r) {
                    std::cout << ">> MAR row " << r << " log10 Z = " << lz[r] << " marginals:";
                    for (double v : marg[r]) std::cout << " " << v;
                    std::cout << std::endl;
                }
                std::cout << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
                if (!uai_out.empty()) {
                    FILE *f = std::fopen((uai_out + ".MAR").c_str(), "w");
                    if (!f) throw std::runtime_error("cannot write " + uai_out + ".MAR");
                    std::fprintf(f, "MAR\n%zu\n", marg.size());
                    for (const auto &row : marg) {
                        std::fprintf(f, "%zu", mv.size());
                        size_t at = 0;
                        for (const bn::Variable *v : mv) {
                            std::fprintf(f, " %u", (unsigned)v->size());
                            for (unsigned x = 0; x < v->size(); ++x) std::fprintf(f, " %.17g", row[at++]);
                        }
                        std::fprintf(f, "\n");
                    }
                    std::fclose(f);
                }
            }
            if (options["posterior-batch"]) {
                const std::vector<std::vector<double>> post = model->posterior_batch(vars, rows, partial, soft, post_target, options, &uptime);
                std::cout << ">> P(" << post_target << " | row) of " << post.size() << " evidence rows; row 0:";
                if (!post.empty())
                    for (double v : post[0]) std::cout << " " << v;
                std::cout << std::endl << ">> Executed in " << uptime << "ms." << std::endl << std::endl;
                if (!uai_out.empty()) {
                    FILE *f = std::fopen((uai_out + ".MAR").c_str(), "w");
                    if (!f) throw std::runtime_error("cannot write " + uai_out + ".MAR");
                    std::fprintf(f, "MAR\n%zu\n", post.size());
                    for (const auto &row : post) {
                        std::fprintf(f, "1 %zu", row.size());
                        for (double v : row) std::fprintf(f, " %.17g", v);
                        std::fprintf(f, "\n");
                    }
                    std::fclose(f);
                }
            }
        }
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << std::endl;
        delete model;
        return -3;
    }
    delete model;
    return 0;
}
