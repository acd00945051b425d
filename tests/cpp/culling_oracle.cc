// Scalar restatement of LocalMapping::KeyFrameCulling (R/lib_src/LocalMapping.cc:953-1079) and CloudKeyFrameCulling (:820-951) on the flat
// arrays of rumi_keyframe_culling (include/rumi_mapping.h): non-inertial, monocular.  TEST ORACLE: it keeps a mutable copy of the map --
// every key-frame's mvpMapPoints, every point's observation entries, nObs and bad flag -- and really runs KeyFrame::SetBadFlag
// (KeyFrame.cc:778-861, the part that touches points), MapPoint::EraseObservation (MapPoint.cc:192-225) and MapPoint::SetBadFlag
// (:240-263) on it, so it shares nothing with the device's culled-set arithmetic.  Built with -ffp-contract=off.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rumi_mapping.h"

namespace {

struct MapState {
    const RumiCullKF *kf;
    const RumiCullPoint *pts;
    const int32_t *obs_kf, *obs_feature;
    std::vector<std::vector<int32_t>> mvpMapPoints;      // per key-frame, -1 = NULL
    std::vector<uint8_t> kfBad, kfToBeErased;
    std::vector<uint8_t> inMap;                          // per observation entry: still in its point's mObservations
    std::vector<int32_t> nObs;
    std::vector<uint8_t> ptBad;

    void MapPoint_SetBadFlag(int p) {                    // MapPoint.cc:240-263
        ptBad[p] = 1;                                    // :246
        std::vector<int> obs;                            // :247 obs = mObservations
        for (int o = pts[p].obs_begin; o < pts[p].obs_end; o++)
            if (inMap[o]) { obs.push_back(o); inMap[o] = 0; }    // :248 mObservations.clear()
        for (int o : obs) mvpMapPoints[obs_kf[o]][obs_feature[o]] = -1;   // :250-256 pKF->EraseMapPointMatch(leftIndex)
    }
    void MapPoint_EraseObservation(int p, int pKF) {     // MapPoint.cc:192-225
        bool bBad = false;
        for (int o = pts[p].obs_begin; o < pts[p].obs_end; o++)
            if (inMap[o] && obs_kf[o] == pKF) {          // :197 mObservations.count(pKF)
                nObs[p]--;                               // :206 (monocular: leftIndex != -1, mvuRight < 0)
                inMap[o] = 0;                            // :212
                if (nObs[p] <= 2) bBad = true;           // :218-219
                break;
            }
        if (bBad) MapPoint_SetBadFlag(p);                // :223-224
    }
    void KeyFrame_SetBadFlag(int k) {                    // KeyFrame.cc:778-861
        if (kf[k].is_init) return;                       // :781-782
        if (kf[k].not_erase) { kfToBeErased[k] = 1; return; }    // :783-785
        for (std::size_t i = 0; i < mvpMapPoints[k].size(); i++)  // :793-797
            if (mvpMapPoints[k][i] >= 0) MapPoint_EraseObservation(mvpMapPoints[k][i], k);
        kfBad[k] = 1;                                    // :861
    }
};

}  // namespace

// Same arguments as rumi_keyframe_culling without the handle, then the map the loop leaves (each may be NULL): kf_bad, kf_to_be_erased
// [n_kf], pt_bad, pt_nobs [n_pts], obs_in_map [n_obs], mp_after [sum of kfs[k].n, key-frame after key-frame].  The inputs are trusted.
extern "C" int cuo_keyframe_culling(const RumiCullKF *kfs, int32_t n_kf, const int32_t *cand, int32_t n_cand, const RumiCullPoint *pts, int32_t n_pts,
                                    const int32_t *obs_kf, const int32_t *obs_feature, int32_t n_obs, int32_t flags, int32_t *status, int32_t *n_mps,
                                    int32_t *n_redundant, int32_t *culled, int32_t *n_culled, uint8_t *kf_bad, uint8_t *kf_to_be_erased,
                                    uint8_t *pt_bad, int32_t *pt_nobs, uint8_t *obs_in_map, int32_t *mp_after) {
    MapState m;
    m.kf = kfs; m.pts = pts; m.obs_kf = obs_kf; m.obs_feature = obs_feature;
    m.mvpMapPoints.resize(n_kf); m.kfBad.resize(n_kf); m.kfToBeErased.assign(n_kf, 0);
    for (int k = 0; k < n_kf; k++) { m.mvpMapPoints[k].assign(kfs[k].mp, kfs[k].mp + kfs[k].n); m.kfBad[k] = kfs[k].is_bad; }
    m.inMap.assign(n_obs, 0); m.nObs.resize(n_pts); m.ptBad.resize(n_pts);
    for (int p = 0; p < n_pts; p++) {
        m.nObs[p] = pts[p].n_obs_count; m.ptBad[p] = pts[p].is_bad;
        for (int o = pts[p].obs_begin; o < pts[p].obs_end; o++) m.inMap[o] = 1;
    }
    const bool cloudVariant = (flags & RUMI_CULL_CLOUD) != 0, mbAbortBA = (flags & RUMI_CULL_ABORT_BA) != 0;
    for (int c = 0; c < n_cand; c++) { status[c] = RUMI_CULL_NOT_REACHED; n_mps[c] = 0; n_redundant[c] = 0; }
    *n_culled = 0;

    const float redundant_th = 0.9;                                           // :962-964 (!mbInertial)
    int count = 0;                                                            // :971
    for (int c = 0; c < n_cand; c++) {                                        // :985
        count++;                                                              // :986
        const int pKF = cand[c];                                              // :987
        if (cloudVariant && kfs[pKF].is_cloud) { status[c] = RUMI_CULL_SKIPPED_CLOUD; continue; }   // :857-859
        if (kfs[pKF].is_init || m.kfBad[pKF]) {                               // :989-990
            status[c] = kfs[pKF].is_init ? RUMI_CULL_SKIPPED_INIT : RUMI_CULL_SKIPPED_BAD;
            continue;
        }
        const std::vector<int32_t> vpMapPoints = m.mvpMapPoints[pKF];         // :991
        const int thObs = 3;                                                  // :993-994
        int nRedundantObservations = 0, nMPs = 0;                             // :995-996
        for (std::size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {   // :997
            const int pMP = vpMapPoints[i];
            if (pMP < 0) continue;                                            // :999
            if (m.ptBad[pMP]) continue;                                       // :1000
            nMPs++;                                                           // :1006
            if (m.nObs[pMP] > thObs) {                                        // :1007
                const int scaleLevel = kfs[pKF].octave[i];                    // :1008, NLeft == -1
                int nObs = 0;                                                 // :1010
                for (int o = pts[pMP].obs_begin; o < pts[pMP].obs_end; o++) { // :1011, the entries still in mObservations
                    if (!m.inMap[o]) continue;
                    const int pKFi = obs_kf[o];
                    if (pKFi == pKF) continue;                                // :1013-1014
                    const int scaleLeveli = kfs[pKFi].octave[obs_feature[o]]; // :1019
                    if (scaleLeveli <= scaleLevel + 1) {                      // :1030
                        nObs++;
                        if (nObs > thObs) break;                              // :1032-1033
                    }
                }
                if (nObs > thObs) nRedundantObservations++;                   // :1036-1037
            }
        }
        n_mps[c] = nMPs; n_redundant[c] = nRedundantObservations;
        status[c] = RUMI_CULL_KEPT;
        if (nRedundantObservations > redundant_th * nMPs) {                   // :1044
            m.KeyFrame_SetBadFlag(pKF);                                       // :1072
            if (m.kfBad[pKF]) { status[c] = RUMI_CULL_CULLED; culled[(*n_culled)++] = c; }
            else status[c] = RUMI_CULL_TO_BE_ERASED;
        }
        if ((count > 20 && mbAbortBA) || count > 100) break;                  // :1075-1077
    }
    for (int k = 0; k < n_kf; k++) {
        if (kf_bad) kf_bad[k] = m.kfBad[k];
        if (kf_to_be_erased) kf_to_be_erased[k] = m.kfToBeErased[k];
    }
    for (int p = 0; p < n_pts; p++) {
        if (pt_bad) pt_bad[p] = m.ptBad[p];
        if (pt_nobs) pt_nobs[p] = m.nObs[p];
    }
    if (obs_in_map) for (int o = 0; o < n_obs; o++) obs_in_map[o] = m.inMap[o];
    if (mp_after) for (int k = 0; k < n_kf; k++) for (int32_t v : m.mvpMapPoints[k]) *mp_after++ = v;
    return 0;
}
