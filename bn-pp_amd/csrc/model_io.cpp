#include "model_io.hpp"

#include <algorithm>
#include <cstdlib>
#include <fstream>

namespace bnpp {
namespace {

// read_next_token (io.cpp:14-23): a token starting with '#' drops the rest of its line
bool next_token(std::ifstream &in, std::string &tok) {
    while (in >> tok) {
        if (tok[0] != '#') return true;
        std::string rest;
        std::getline(in, rest);
    }
    return false;
}
bool next_long(std::ifstream &in, long &v) {
    std::string t;
    if (!next_token(in, t)) return false;
    char *end = nullptr;
    v = std::strtol(t.c_str(), &end, 10);
    return end != t.c_str();
}
bool next_double(std::ifstream &in, double &v) {
    std::string t;
    if (!next_token(in, t)) return false;
    char *end = nullptr;
    v = std::strtod(t.c_str(), &end);
    return end != t.c_str();
}

}  // namespace

int load_uai(const std::string &path, ModelData &m, std::string *err) {
    std::ifstream in(path);
    if (!in.is_open()) {
        if (err) *err = "couldn't read file " + path;
        return -1;
    }
    m = ModelData{};
    m.name = path;
    std::string hdr;
    if (!next_token(in, hdr) || (hdr != "BAYES" && hdr != "MARKOV")) {
        if (err) *err = "expected 'BAYES' or 'MARKOV' file header, found: " + hdr;
        return -2;
    }
    m.is_bayes = hdr == "BAYES";
    long nv, nf;
    if (!next_long(in, nv) || nv < 0) goto bad;
    m.cards.resize(nv);
    for (long i = 0; i < nv; ++i) {
        long c;
        if (!next_long(in, c) || c < 1) goto bad;
        m.cards[i] = (int)c;
    }
    if (!next_long(in, nf) || nf < 0) goto bad;
    m.scopes.resize(nf);
    m.values.resize(nf);
    for (long f = 0; f < nf; ++f) {
        long w;
        if (!next_long(in, w) || w < 0) goto bad;
        m.scopes[f].resize(w);
        for (long j = 0; j < w; ++j) {
            long id;
            if (!next_long(in, id) || id < 0 || id >= nv) goto bad;
            m.scopes[f][j] = (int)id;
        }
    }
    for (long f = 0; f < nf; ++f) {
        long sz;
        if (!next_long(in, sz) || sz < 0) goto bad;
        m.values[f].resize(sz);
        for (long j = 0; j < sz; ++j)
            if (!next_double(in, m.values[f][j])) goto bad;
    }
    if (!validate(m, err)) return -2;
    return 0;
bad:
    if (err) *err = "malformed UAI file " + path;
    return -2;
}

int load_evidence(const std::string &path, std::vector<std::pair<int, int>> &ev) {
    std::ifstream in(path);
    if (!in.is_open()) return -1;
    ev.clear();
    long n, size;
    if (next_long(in, n) && n == 1 && next_long(in, size)) {
        for (long i = 0; i < size; ++i) {
            long id, val;
            if (!next_long(in, id) || !next_long(in, val)) break;
            bool found = false;
            for (auto &p : ev)
                if (p.first == id) { p.second = (int)val; found = true; }
            if (!found) ev.push_back({(int)id, (int)val});
        }
    }
    return 0;
}

int load_evidence_batch(const std::string &path, std::vector<int> &vars, std::vector<int> &vals, int64_t &n_rows,
                        std::string *err) {
    std::ifstream in(path);
    if (!in.is_open()) return -1;
    vars.clear();
    vals.clear();
    n_rows = 0;
    long n;
    if (!next_long(in, n) || n < 0) {
        if (err) *err = "malformed evidence file " + path;
        return -2;
    }
    for (long s = 0; s < n; ++s) {
        long size;
        if (!next_long(in, size) || size < 0) {
            if (err) *err = "malformed evidence file " + path + ": sample " + std::to_string(s) + " is missing";
            return -2;
        }
        std::vector<std::pair<int, int>> ev;
        for (long i = 0; i < size; ++i) {
            long id, val;
            if (!next_long(in, id) || !next_long(in, val)) {
                if (err) *err = "malformed evidence file " + path + ": sample " + std::to_string(s) + " is cut short";
                return -2;
            }
            bool found = false;
            for (auto &p : ev)
                if (p.first == id) { p.second = (int)val; found = true; }   // a repeated id: the last value (io.cpp:171)
            if (!found) ev.push_back({(int)id, (int)val});
        }
        std::sort(ev.begin(), ev.end());
        if (s == 0)
            for (auto &p : ev) vars.push_back(p.first);
        bool same = ev.size() == vars.size();
        for (size_t i = 0; same && i < ev.size(); ++i) same = ev[i].first == vars[i];
        if (!same) {
            if (err) *err = "evidence file " + path + ": sample " + std::to_string(s) +
                            " observes another variable set than sample 0";
            return -3;
        }
        for (auto &p : ev) vals.push_back(p.second);
        ++n_rows;
    }
    return 0;
}

int load_evidence_batch_missing(const std::string &path, std::vector<int> &vars, std::vector<int> &vals,
                                std::vector<unsigned char> &partial, int64_t &n_rows, std::string *err) {
    std::ifstream in(path);
    if (!in.is_open()) return -1;
    vars.clear();
    vals.clear();
    partial.clear();
    n_rows = 0;
    long n;
    if (!next_long(in, n) || n < 0) {
        if (err) *err = "malformed evidence file " + path;
        return -2;
    }
    std::vector<std::vector<std::pair<int, int>>> samples((size_t)n);
    for (long s = 0; s < n; ++s) {
        long size;
        if (!next_long(in, size) || size < 0) {
            if (err) *err = "malformed evidence file " + path + ": sample " + std::to_string(s) + " is missing";
            return -2;
        }
        std::vector<std::pair<int, int>> &ev = samples[(size_t)s];
        for (long i = 0; i < size; ++i) {
            long id, val;
            if (!next_long(in, id) || !next_long(in, val)) {
                if (err) *err = "malformed evidence file " + path + ": sample " + std::to_string(s) + " is cut short";
                return -2;
            }
            bool found = false;
            for (auto &p : ev)
                if (p.first == id) { p.second = (int)val; found = true; }   // a repeated id: the last value
            if (!found) ev.push_back({(int)id, (int)val});
        }
        for (auto &p : ev) vars.push_back(p.first);
    }
    std::sort(vars.begin(), vars.end());                    // the union, ascending
    vars.erase(std::unique(vars.begin(), vars.end()), vars.end());
    const size_t ne = vars.size();
    vals.assign((size_t)n * ne, -1);                        // -1 where a sample is silent
    for (long s = 0; s < n; ++s)
        for (auto &p : samples[(size_t)s])
            vals[(size_t)s * ne + (size_t)(std::lower_bound(vars.begin(), vars.end(), p.first) - vars.begin())] = p.second;
    partial.assign(ne, 0);
    for (long s = 0; s < n; ++s)
        for (size_t j = 0; j < ne; ++j)
            if (vals[(size_t)s * ne + j] < 0) partial[j] = 1;
    n_rows = n;
    return 0;
}

bool validate(const ModelData &m, std::string *err) {
    for (size_t f = 0; f < m.scopes.size(); ++f) {
        long double sz = 1;
        for (int v : m.scopes[f]) {
            if (v < 0 || v >= (int)m.cards.size()) {
                if (err) *err = "factor " + std::to_string(f) + ": variable id out of range";
                return false;
            }
            sz *= m.cards[v];
        }
        if ((long double)m.values[f].size() != sz) {
            if (err) *err = "factor " + std::to_string(f) + ": table size does not match its scope";
            return false;
        }
    }
    return true;
}

}  // namespace bnpp
