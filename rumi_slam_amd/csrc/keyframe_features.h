// What a key-frame's constant part must satisfy before a kernel reads it: mvKeysUn, mDescriptors, mvScaleFactors and mFeatVec (CSR).  One
// validator for every entry that takes such a key-frame: rumi_create_new_map_points (mapping.hip) per call, and
// rumi_covis_set_keyframe_features (covis_features.inc) once, when the key-frame enters the store.
#pragma once
#include <cstdint>
#include <vector>

#include "rumi_match.h"

namespace rumi {

// False with *why set.  The kernels search node ids by bisection and give every cand[k][i1] one writer, hence the last two checks.
inline bool keyframe_features_valid(const RumiFrameFeatures &f, const RumiFeatureVector &v, const char **why) {
    *why = "key-frame features: bad sizes or missing arrays";
    if (f.n < 0 || f.nlevels < 1 || f.nlevels > 64 || !f.scale_factors || v.n_nodes < 0) return false;
    if (f.n > 0 && (!f.keys_un || !f.desc)) return false;
    if (v.n_nodes > 0 && (!v.node_ids || !v.offsets || !v.indices)) return false;
    *why = "key-frame features: key-point octave outside mvScaleFactors";
    for (int i = 0; i < f.n; i++) if (f.keys_un[i].octave < 0 || f.keys_un[i].octave >= f.nlevels) return false;
    *why = "key-frame features: FeatureVector offsets or indices out of range";
    if (v.n_nodes > 0) {
        if (v.offsets[0] != 0) return false;
        for (int a = 0; a < v.n_nodes; a++) if (v.offsets[a + 1] < v.offsets[a]) return false;
        for (int p = 0; p < v.offsets[v.n_nodes]; p++) if (v.indices[p] >= (uint32_t)f.n) return false;
        *why = "key-frame features: FeatureVector node ids not strictly ascending, or a feature listed twice";
        for (int a = 1; a < v.n_nodes; a++) if (v.node_ids[a] <= v.node_ids[a - 1]) return false;
        std::vector<uint8_t> seen((size_t)f.n, 0);
        for (int p = 0; p < v.offsets[v.n_nodes]; p++) { if (seen[v.indices[p]]) return false; seen[v.indices[p]] = 1; }
    }
    return true;
}

}  // namespace rumi
