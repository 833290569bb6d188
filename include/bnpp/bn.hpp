// bn.hpp — C++ mirror of bn-pp's class API (code/variable.hh, domain.hh,
// factor.hh, model.hh, io.hh) on top of the MI355X engine.
//
// Same names, argument meaning and error behaviour as the reference, with two
// deliberate differences:
//   - sizes and positions are 64-bit (the reference's `unsigned` wraps at 2^32,
//     domain.hh:21-22);
//   - every factor-algebra operation (product, sum_out, conditioning, the VE
//     buckets) runs on the GPU through include/bnpp.h; there is no CPU
//     fallback: without a device they throw std::runtime_error.
// Index-range errors throw const char* exactly like factor.cpp:87/94 and
// domain.cpp:96.
#pragma once

#include <cstdint>
#include <memory>
#include <ostream>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace bn {

class Variable {                                   // variable.hh:8-21
public:
    Variable(unsigned id, unsigned size) : _id(id), _size(size) {}
    unsigned id() const { return _id; }
    unsigned size() const { return _size; }
    friend std::ostream &operator<<(std::ostream &o, const Variable &v);

private:
    unsigned _id;
    unsigned _size;
};

class Domain {                                     // domain.hh:11-45
public:
    Domain();
    Domain(std::vector<const Variable *> scope);
    Domain(const Domain &d);
    Domain(const Domain &d1, const Domain &d2);    // union: d1 order, then new d2 vars
    Domain(const Domain &d, const Variable *v);    // remove v
    Domain(const Domain &d, const std::unordered_map<unsigned, unsigned> &evidence);

    std::vector<const Variable *> scope() const { return _scope; }
    unsigned width() const { return (unsigned)_scope.size(); }
    uint64_t size() const { return _size; }
    const Variable *operator[](unsigned i) const;
    bool in_scope(const Variable *v) const;
    bool in_scope(unsigned id) const;
    void next_valuation(std::vector<unsigned> &valuation) const;
    uint64_t position_valuation(const std::vector<unsigned> &valuation) const;
    uint64_t position_consistent_valuation(const std::vector<unsigned> &valuation, const Domain &domain) const;
    friend std::ostream &operator<<(std::ostream &o, const Domain &d);

private:
    void init();
    std::vector<const Variable *> _scope;
    std::vector<uint64_t> _offset;
    uint64_t _size = 1;
};

class Factor {                                     // factor.hh:11-48
public:
    Factor(const Domain *domain, std::vector<double> values, double partition);   // adopts domain
    Factor(const Domain *domain, double value = 0.0);
    Factor(double value = 1.0);
    Factor(const Factor &f);
    Factor(Factor &&f) noexcept;
    ~Factor();
    Factor &operator=(Factor &&f) noexcept;
    Factor &operator=(const Factor &f);
    Factor operator*(const Factor &f);
    void operator*=(const Factor &f);

    const Domain &domain() const { return *_domain; }
    uint64_t size() const { return _domain->size(); }
    unsigned width() const { return _domain->width(); }
    double partition() const;                    // factor.hh:26 (computed on first read)
    const double &operator[](uint64_t i) const;
    double &operator[](uint64_t i);
    const std::vector<double> &values() const { return _values; }
    double max() const;
    double min() const;

    Factor sum_out(const Variable *variable) const;                                  // factor.cpp:182-212
    Factor product(const Factor &f) const;                                           // factor.cpp:117-147
    Factor divide(const Factor &f) const;                                            // factor.cpp:149-180
    Factor conditioning(const std::unordered_map<unsigned, unsigned> &evidence) const;  // factor.cpp:214-242
    Factor normalize() const;                                                        // factor.cpp:244-255
    friend std::ostream &operator<<(std::ostream &os, const Factor &f);

private:
    // The reference computes _partition with every op (factor.cpp:129-139,
    // 161-172, 196-208, 226-236); here an op leaves it pending and the first
    // read (partition(), normalize(), min(), printing, a mutable operator[])
    // computes it on the host in the reference's order, so an op whose
    // partition nobody reads costs its kernel and transfers only.
    struct PendingSum;
    void resolve_partition() const;
    const Domain *_domain;
    std::vector<double> _values;
    mutable double _partition;
    mutable std::shared_ptr<const PendingSum> _pending;
};

// EXTENSION: soft evidence of the batched calls (Model::*_batch, expected_counts): the soft variables and, per
// evidence row, their likelihoods -- the variables' blocks in the listed order
struct SoftEvidence {
    std::vector<unsigned> vars;
    std::vector<std::vector<double>> lik;
};

// The GPU engine's precision for Model/BN inference (default fp64, bit-exact
// with the reference's arithmetic); options["fp32"] selects fp32 storage.
class Model {                                      // model.hh:11-38
public:
    Model(std::string name, std::vector<Variable *> &variables, std::vector<Factor *> &factors);
    virtual ~Model();
    const std::string name() const { return _name; }
    const std::vector<Variable *> &variables() const { return _variables; }
    const std::vector<Factor *> &factors() const { return _factors; }

    // VE on the GPU (the reference's Model:: versions form the full joint; the
    // result is the same quantity)
    virtual double partition(const std::unordered_map<unsigned, unsigned> &evidence,
                             std::unordered_map<std::string, bool> &options, double &uptime) const;
    // options["bucket-tree"]: all marginals from one two-pass bucket tree
    // (bnpp_marginals_tree, equal to rounding); default: one VE per target,
    // bit-exact with the reference arithmetic
    virtual std::vector<const Factor *> marginals(const std::unordered_map<unsigned, unsigned> &evidence,
                                                  std::unordered_map<std::string, bool> &options,
                                                  double &uptime) const;
    // log10 of the partition function (finite beyond the double range)
    double log10_partition(const std::unordered_map<unsigned, unsigned> &evidence,
                           std::unordered_map<std::string, bool> &options, double &uptime) const;
    // EXTENSION beyond the reference's class API (bn-pp has no MPE): the most
    // probable explanation given the evidence (bnpp_mpe): one value per
    // variable, in variables() order, evidence variables keeping theirs.
    // Max-product elimination with a traceback on the device; ties resolve to
    // the lowest value of a variable as it is maximised.  Every non-evidence
    // variable needs a size <= 256.  log10_value (optional): log10 of the
    // maximum, the assignment's unnormalised probability.
    std::vector<unsigned> mpe(const std::unordered_map<unsigned, unsigned> &evidence,
                              std::unordered_map<std::string, bool> &options, double *log10_value = nullptr,
                              double *uptime = nullptr) const;
    // EXTENSION beyond the reference's class API (BN::sampling and the
    // estimators of model.cpp:541-720 sample the prior from random_device):
    // n exact joint samples of P(x | evidence) (bnpp_sample), reproducible
    // from `seed`; result[s] holds one value per variable, in variables()
    // order, evidence variables keeping theirs.  Every non-evidence variable
    // needs a size <= 256.  log10_z (optional): log10 of the partition function.
    std::vector<std::vector<unsigned char>> sample(const std::unordered_map<unsigned, unsigned> &evidence,
                                                   std::unordered_map<std::string, bool> &options, size_t n,
                                                   unsigned long long seed = 0, double *log10_z = nullptr,
                                                   double *uptime = nullptr) const;
    // EXTENSION beyond the reference's class API: batched evidence
    // (bnpp_partition_batch / bnpp_posterior_batch).  rows[r][j] is the value
    // of variable ev_vars[j] in evidence row r; every row observes the same
    // variables.  partition_batch returns log10 Z per row (z, optional: Z per
    // row); posterior_batch returns P(target | row r) per row.  In fp64 each
    // row carries the bits of partition() / marginals() for that evidence.
    std::vector<double> partition_batch(const std::vector<unsigned> &ev_vars,
                                        const std::vector<std::vector<unsigned>> &rows,
                                        std::unordered_map<std::string, bool> &options, std::vector<double> *z = nullptr,
                                        double *uptime = nullptr) const;
    std::vector<std::vector<double>> posterior_batch(const std::vector<unsigned> &ev_vars,
                                                     const std::vector<std::vector<unsigned>> &rows, unsigned target,
                                                     std::unordered_map<std::string, bool> &options,
                                                     double *uptime = nullptr) const;
    // EXTENSION: batched MPE (bnpp_mpe_batch).  Row r of the result is mpe()'s
    // assignment for evidence row r, entry for entry (ties included), from one
    // plan; log10_value (optional) per row, -inf for an impossible row.
    std::vector<std::vector<unsigned>> mpe_batch(const std::vector<unsigned> &ev_vars,
                                                 const std::vector<std::vector<unsigned>> &rows,
                                                 std::unordered_map<std::string, bool> &options,
                                                 std::vector<double> *log10_value = nullptr,
                                                 double *uptime = nullptr) const;
    // EXTENSION: batched posterior sampling (bnpp_sample_batch).  k exact joint
    // samples of P(x | row r) for every evidence row from one plan, rows
    // outermost: sample s of row r is entry r * k + s, and it is sample()'s
    // draw for that evidence at the global index r * k + s (disjoint streams);
    // log10_z (optional) per row, -inf for an impossible row.
    std::vector<std::vector<unsigned char>> sample_batch(const std::vector<unsigned> &ev_vars,
                                                         const std::vector<std::vector<unsigned>> &rows,
                                                         std::unordered_map<std::string, bool> &options, size_t k,
                                                         unsigned long long seed = 0,
                                                         std::vector<double> *log10_z = nullptr,
                                                         double *uptime = nullptr) const;
    // EXTENSION: expected sufficient statistics (bnpp_expected_counts).  Per
    // factor, in model order, N_f(x_S) = sum_r w_r P(x_S | row r) in the
    // factor's own layout over its whole scope; weights empty: all 1.
    // log10_z (optional) per row; n_impossible (optional) the rows with Z = 0,
    // which count nowhere.  Every row observes the same variables: group rows
    // with different missing patterns by pattern and add the counts.
    std::vector<std::vector<double>> expected_counts(const std::vector<unsigned> &ev_vars,
                                                     const std::vector<std::vector<unsigned>> &rows,
                                                     const std::vector<double> &weights,
                                                     std::unordered_map<std::string, bool> &options,
                                                     std::vector<double> *log10_z = nullptr,
                                                     long long *n_impossible = nullptr, double *uptime = nullptr) const;
    // EXTENSION: batched marginals (bnpp_marginals_batch).  Row r of the result
    // holds P(X_t | row r) of every target t, one block of card(t) values after
    // another in the targets' order (targets empty: all variables); a target
    // that is an evidence variable reads one-hot, an impossible row NaN in its
    // other blocks.  log10_z (optional) per row, -inf for an impossible row.
    std::vector<std::vector<double>> marginals_batch(const std::vector<unsigned> &ev_vars,
                                                     const std::vector<std::vector<unsigned>> &rows,
                                                     const std::vector<unsigned> &targets,
                                                     std::unordered_map<std::string, bool> &options,
                                                     std::vector<double> *log10_z = nullptr,
                                                     double *uptime = nullptr) const;
    // EXTENSION: missing values (the bnpp_*_mv entries).  The overloads below take rows of int, in which
    // BNPP_MISSING (-1) marks a value a row does not observe, and partial[j] != 0 for every ev_vars[j] that may
    // be missing in a row (empty: none -- the call above).  A row's result is the call's for evidence equal to
    // its observed entries; mpe_batch and sample_batch keep the observed entries.
    std::vector<double> partition_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial,
        std::unordered_map<std::string, bool> &options, std::vector<double> *z = nullptr,
        double *uptime = nullptr) const;
    std::vector<std::vector<unsigned>> mpe_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial,
        std::unordered_map<std::string, bool> &options, std::vector<double> *log10_value = nullptr,
        double *uptime = nullptr) const;
    std::vector<std::vector<double>> posterior_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial, unsigned target,
        std::unordered_map<std::string, bool> &options, double *uptime = nullptr) const;
    std::vector<std::vector<double>> expected_counts(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial,
        const std::vector<double> &weights, std::unordered_map<std::string, bool> &options,
        std::vector<double> *log10_z = nullptr, long long *n_impossible = nullptr, double *uptime = nullptr) const;
    std::vector<std::vector<double>> marginals_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial,
        const std::vector<unsigned> &targets, std::unordered_map<std::string, bool> &options,
        std::vector<double> *log10_z = nullptr, double *uptime = nullptr) const;
    std::vector<std::vector<unsigned char>> sample_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial,
        std::unordered_map<std::string, bool> &options, size_t k, unsigned long long seed = 0,
        std::vector<double> *log10_z = nullptr, double *uptime = nullptr) const;
    // EXTENSION: soft evidence (the bnpp_*_sv entries).  Beside the evidence a row carries likelihoods of the
    // SOFT variables soft.vars: soft.lik[b] holds row b's Ws = sum of their cards numbers, the variables'
    // blocks in the listed order (the layout marginals_batch returns), finite and >= 0.  A row's result is the
    // call's on the model with one more unary factor per soft variable; a soft variable is no evidence
    // variable: it is eliminated, maximised, drawn and counted.  Empty soft.vars: the overload above.
    std::vector<double> partition_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial, const SoftEvidence &soft,
        std::unordered_map<std::string, bool> &options, std::vector<double> *z = nullptr,
        double *uptime = nullptr) const;
    std::vector<std::vector<unsigned>> mpe_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial, const SoftEvidence &soft,
        std::unordered_map<std::string, bool> &options, std::vector<double> *log10_value = nullptr,
        double *uptime = nullptr) const;
    std::vector<std::vector<double>> posterior_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial, const SoftEvidence &soft,
        unsigned target, std::unordered_map<std::string, bool> &options, double *uptime = nullptr) const;
    std::vector<std::vector<double>> expected_counts(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial, const SoftEvidence &soft,
        const std::vector<double> &weights, std::unordered_map<std::string, bool> &options,
        std::vector<double> *log10_z = nullptr, long long *n_impossible = nullptr, double *uptime = nullptr) const;
    std::vector<std::vector<double>> marginals_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial, const SoftEvidence &soft,
        const std::vector<unsigned> &targets, std::unordered_map<std::string, bool> &options,
        std::vector<double> *log10_z = nullptr, double *uptime = nullptr) const;
    std::vector<std::vector<unsigned char>> sample_batch(const std::vector<unsigned> &ev_vars,
        const std::vector<std::vector<int>> &rows, const std::vector<unsigned char> &partial, const SoftEvidence &soft,
        std::unordered_map<std::string, bool> &options, size_t k, unsigned long long seed = 0,
        std::vector<double> *log10_z = nullptr, double *uptime = nullptr) const;
    virtual void write(std::ostream &) const {}

protected:
    std::string _name;
    std::vector<Variable *> _variables;
    std::vector<Factor *> _factors;
};

class BN : public Model {                          // model.hh:40-104
public:
    BN(std::string name, std::vector<Variable *> &variables, std::vector<Factor *> &factors);
    // model.cpp:348-446: bucket elimination, one fused GPU kernel per bucket
    Factor variable_elimination(std::vector<const Variable *> &variables, std::vector<const Factor *> &factors,
                                std::unordered_map<std::string, bool> &options) const;
    // model.cpp:205-248: P(target | evidence) as a table over target + evidence
    Factor query_ve(const std::unordered_set<const Variable *> &target,
                    const std::unordered_set<const Variable *> &evidence,
                    std::unordered_map<std::string, bool> &options, double &uptime) const;
    const std::unordered_set<const Variable *> parents(const Variable *v) const { return _parents.find(v)->second; }
    const std::unordered_set<const Variable *> children(const Variable *v) const { return _children.find(v)->second; }

private:
    std::unordered_map<const Variable *, std::unordered_set<const Variable *>> _parents;
    std::unordered_map<const Variable *, std::unordered_set<const Variable *>> _children;
};

class MN : public Model {                          // model.hh:106-118
public:
    MN(std::string name, std::vector<Variable *> &variables, std::vector<Factor *> &factors);
    // model.cpp:979-999: "MARKOV:", every variable with its neighbours, every factor
    void write(std::ostream &os) const override;
    friend std::ostream &operator<<(std::ostream &os, const MN &mn);

private:
    // the reference's container (model.hh:116), filled in the same order, so
    // the neighbours print in its iteration order
    std::unordered_map<const Variable *, std::unordered_set<const Variable *>> _neighbors;
};

// io.hh:10-19 (return 0 / -1 cannot open / -2 wrong network type)
int read_uai_model(std::string &filename, BN **model);
int read_uai_model(std::string &filename, MN **model);
int read_uai_evidence(std::string &filename, std::unordered_map<unsigned, unsigned> &evidence);

// Engine device used by the C++ API (default: env BNPP_DEVICE or 0).
void set_device(int device);

}  // namespace bn
