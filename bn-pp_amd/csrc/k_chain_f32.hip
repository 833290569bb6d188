// Chain (sweep) kernel instantiations, float (separate translation unit).
#include "chainsplit.cuh"

namespace bnpp {

// grid_cap: bnpp_ctx_set_max_grid's cap for the split launches (0: none); the
// one-thread launches take it through max_grid
hipError_t dispatch_chain_level_f32(int key, const LevelArgs &a, int small_elems, int max_grid, int grid_cap,
                                    hipStream_t stream) {
    switch (key) { BNPP_CHAIN_F32(BNPP_CASE_CHAIN, float) BNPP_CHAIN_SPLIT(BNPP_CASE_CHAIN_SPLIT) default: break; }
    return hipErrorInvalidValue;
}
bool chain_supported_f32(int key) {
    switch (key) { BNPP_CHAIN_F32(BNPP_CASE_CHAIN_OK, float) BNPP_CHAIN_SPLIT(BNPP_CASE_CHAIN_SPLIT_OK) default: break; }
    return false;
}
void keys_chain_f32(std::vector<int> &keys) {
    static const int k[] = {BNPP_CHAIN_F32(BNPP_LIST_CHAIN, float) BNPP_CHAIN_SPLIT(BNPP_LIST_CHAIN_SPLIT)};
    keys.insert(keys.end(), k, k + sizeof k / sizeof *k);
}
}  // namespace bnpp
