// Slab-form kernel instantiations (float), a separate translation unit (parallel build).
#include <vector>

#include "slab.cuh"

namespace bnpp {

hipError_t dispatch_slab_single_f32(int key, const SingleArgs &a, hipStream_t stream) {
    switch (key) { BNPP_SLAB_F32(BNPP_CASE_SLAB_SINGLE, float) BNPP_SLAB8_F32(BNPP_CASE_SLAB8_SINGLE, float) default: break; }
    return hipErrorInvalidValue;
}
hipError_t dispatch_slab_level_f32(int key, const LevelArgs &a, hipStream_t stream) {
    switch (key) { BNPP_SLAB_F32(BNPP_CASE_SLAB_LEVEL, float) BNPP_SLAB_R2_F32(BNPP_CASE_SLAB_LEVEL_R2, float)
                   BNPP_SLAB8_F32(BNPP_CASE_SLAB8_LEVEL, float) default: break; }
    return hipErrorInvalidValue;
}
void keys_slab_f32(int level, std::vector<int> &keys) {
    static const int single[] = {BNPP_SLAB_F32(BNPP_LIST_SLAB, float) BNPP_SLAB8_F32(BNPP_LIST_SLAB8_SINGLE, float)};
    static const int lvl[] = {BNPP_SLAB_F32(BNPP_LIST_SLAB, float) BNPP_SLAB_R2_F32(BNPP_LIST_SLAB_R2, float)
                              BNPP_SLAB8_F32(BNPP_LIST_SLAB8_LEVEL, float)};
    if (level) keys.insert(keys.end(), lvl, lvl + sizeof lvl / sizeof *lvl);
    else keys.insert(keys.end(), single, single + sizeof single / sizeof *single);
}
}  // namespace bnpp
