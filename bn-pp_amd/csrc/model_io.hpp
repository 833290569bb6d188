// Host data model + UAI reader (io.cpp:14-180 token rules).
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace bnpp {

struct ModelData {
    std::string name;
    bool is_bayes = false;
    std::vector<int> cards;                      // per variable
    std::vector<std::vector<int>> scopes;        // per factor, reference scope order
    std::vector<std::vector<double>> values;     // per factor, row-major (last var fastest)
};

// read_file_header / read_variables / read_factors (io.cpp:43-100).  Returns 0,
// -1 when the file cannot be opened (io.cpp:124), -2 on a malformed file.
int load_uai(const std::string &path, ModelData &m, std::string *err);
// read_uai_evidence (io.cpp:157-180): pairs are read only when the first integer
// is 1; a repeated id keeps the last value.  Returns 0 or -1 (cannot open).
int load_evidence(const std::string &path, std::vector<std::pair<int, int>> &ev);
// an .evid file of any number of samples (the count, then per sample
// `k v_1 x_1 ... v_k x_k`), every sample over the same variable set: vars
// ascending, vals[row][vars.size()] row-major.  Returns 0, -1 (cannot open), -2
// (malformed), -3 (a sample observes another variable set than the first; err names it)
int load_evidence_batch(const std::string &path, std::vector<int> &vars, std::vector<int> &vals, int64_t &n_rows,
                        std::string *err);
// ... whose samples may observe differing variable sets (missing values): vars is the union, ascending,
// vals holds -1 where a sample is silent, partial[j] = 1 for a variable some sample lacks.  Returns 0, -1, -2
int load_evidence_batch_missing(const std::string &path, std::vector<int> &vars, std::vector<int> &vals,
                                std::vector<unsigned char> &partial, int64_t &n_rows, std::string *err);
// validate shapes (scope ids in range, table sizes = prod(card))
bool validate(const ModelData &m, std::string *err);

}  // namespace bnpp
