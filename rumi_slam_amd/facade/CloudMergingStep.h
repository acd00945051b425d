// Facade for the key-point match of CloudMerging::ComputeSubmapSim3 (R/lib_src/CloudMerging.cc:503-551): the loop over mKfMatch12 that looks every
// key-point of key-frame 1 up in key-frame 2 with KeyFrame::GetFeaturesInArea(u, v, 3) and keeps the nearest candidate where both slots hold a map
// point.  All pairs go to the GPU in one call (include/rumi_match.h: rumi_submap_match); this side marshals the key-frames and fills the four maps
// the loop fills.  The rest of ComputeSubmapSim3 already runs through Sim3Scoring.h, Optimizer.h and shells/Sim3Solver.cc.
//
// Each key-frame's grid is rebuilt on the device from mvKeysUn by the Frame::PosInGrid rule with the key-frame's own mnMinX, mnMinY and inverse cell
// sizes.  That equals mGrid for every key-frame built from a Frame (KeyFrame's constructor copies Frame::mGrid, which AssignFeaturesToGrid filled
// by that rule); the cloud map's key-frames are built that way (cloud_edge_main.cpp:944-948).
//
// Templated on the key-frame and map-point types, so that it instantiates against the reference's classes and against the stand-ins of tests/cpp.
#pragma once
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "rumi_match.h"
#include "rumi_status.h"

namespace rumi_facade {

namespace submap_detail {
// One matcher arena per calling thread (handles are not re-entrant); the call's own blocks grow on demand, so there is nothing to double.
inline RumiMatcher *arena() {
    struct Holder { RumiMatcher *h = nullptr; ~Holder() { if (h) rumi_match_destroy(h); } };
    thread_local Holder holder;
    if (!holder.h) {
        const int rc = rumi_match_create(1, 1, -1, &holder.h);
        if (rc != RUMI_OK) { report("MatchSubmapKeyPoints: matcher arena", rc); holder.h = nullptr; }
    }
    return holder.h;
}

struct Marshalled { std::vector<float> keys, un; std::vector<uint8_t> mp; };
}  // namespace submap_detail

// Returns matchMapPointNum.  The four maps are filled as :546-550 fill them, keyed by vpMap1KeyFrames[iter->first]: vpMatchedPoints12 sized to
// key-frame 1's slots (NULL where there is no match), the two pair lists (equal, as in the reference) and matchNum.  Refused, with a report through
// rumi_status.h, 0 returned and the maps left empty: a key-frame with NLeft != -1 (the two-camera branch of GetFeaturesInArea is not built) or a
// grid other than 64 x 48; likewise when the device call fails.
template <class KeyFrameT, class MapPointT>
int MatchSubmapKeyPoints(const std::vector<KeyFrameT *> &vpMap1KeyFrames, const std::vector<KeyFrameT *> &vpMap2KeyFrames, const std::map<int, int> &mKfMatch12,
                         float tolerance, std::map<KeyFrameT *, std::vector<MapPointT *>> &mvpMatchedPoints12,
                         std::map<KeyFrameT *, std::vector<std::pair<int, int>>> &mvpMatchedKeyPoints12,
                         std::map<KeyFrameT *, std::vector<std::pair<int, int>>> &mvpValidMatchedKeyPoints12, std::map<KeyFrameT *, int> &mvpMatchedPointsNum12) {
    static const char *where = "CloudMergingStep::MatchSubmapKeyPoints / rumi_submap_match";
    if (mKfMatch12.empty()) return 0;
    // the frame table: every key-frame once, however many pairs name it
    std::map<KeyFrameT *, int> index;
    std::vector<KeyFrameT *> kfs;
    std::vector<std::vector<MapPointT *>> slots;
    std::vector<int32_t> f1, f2;
    auto frame_of = [&](KeyFrameT *pKF) {
        auto it = index.find(pKF);
        if (it != index.end()) return it->second;
        index[pKF] = (int)kfs.size();
        kfs.push_back(pKF);
        return (int)kfs.size() - 1;
    };
    for (const auto &m : mKfMatch12) {
        KeyFrameT *pKF1 = vpMap1KeyFrames[m.first], *pKF2 = vpMap2KeyFrames[m.second];
        for (KeyFrameT *pKF : {pKF1, pKF2})
            if (pKF->NLeft != -1 || pKF->mnGridCols != 64 || pKF->mnGridRows != 48) {
                // (the reason travels in the call site's name: the status did not come from the library, so its error string says nothing here)
                RUMI_GUARDED("CloudMergingStep::MatchSubmapKeyPoints: a key-frame with NLeft != -1 or a grid other than 64 x 48 (only the monocular 64 x 48 "
                             "lookup is built; no key-point was matched)", &no_growth, RUMI_E_INVALID);
                return 0;
            }
        f1.push_back(frame_of(pKF1)); f2.push_back(frame_of(pKF2));
    }
    std::vector<submap_detail::Marshalled> data(kfs.size());
    std::vector<RumiSubmapFrame> table(kfs.size());
    size_t sumQ = 0;
    for (size_t k = 0; k < kfs.size(); k++) {
        KeyFrameT *pKF = kfs[k];
        slots.push_back(pKF->GetMapPointMatches());
        const size_t n = pKF->mvKeys.size();
        auto &d = data[k];
        d.keys.resize(2 * n); d.un.resize(2 * n); d.mp.resize(n);
        for (size_t i = 0; i < n; i++) {
            d.keys[2 * i] = pKF->mvKeys[i].pt.x; d.keys[2 * i + 1] = pKF->mvKeys[i].pt.y;
            d.un[2 * i] = pKF->mvKeysUn[i].pt.x; d.un[2 * i + 1] = pKF->mvKeysUn[i].pt.y;
            d.mp[i] = i < slots[k].size() && slots[k][i] != nullptr;
        }
        table[k] = RumiSubmapFrame{(int32_t)n, d.keys.data(), d.un.data(), d.mp.data(), (float)pKF->mnMinX, (float)pKF->mnMinY,
                                   pKF->mfGridElementWidthInv, pKF->mfGridElementHeightInv, 0};
    }
    for (int32_t f : f1) sumQ += (size_t)table[f].n;
    std::vector<int32_t> best2(sumQ + 1), pairStart(f1.size() + 1), matches(2 * sumQ + 2);
    RumiMatcher *h = submap_detail::arena();
    if (!h) return 0;                                       // reported by arena()
    if (RUMI_GUARDED(where, &no_growth, rumi_submap_match(h, (int32_t)table.size(), table.data(), (int32_t)f1.size(), f1.data(), f2.data(), tolerance,
                                                          best2.data(), pairStart.data(), matches.data())) != RUMI_OK)
        return 0;
    int p = 0;
    for (const auto &m : mKfMatch12) {
        KeyFrameT *pKF1 = vpMap1KeyFrames[m.first];
        const auto &slots1 = slots[f1[p]], &slots2 = slots[f2[p]];
        std::vector<MapPointT *> vpMatchedPoints12(slots1.size(), static_cast<MapPointT *>(nullptr));
        std::vector<std::pair<int, int>> vpMatchedKeyPoints12;
        for (int k = pairStart[p]; k < pairStart[p + 1]; k++) {
            const int i1 = matches[2 * k], i2 = matches[2 * k + 1];
            vpMatchedPoints12[i1] = slots2[i2];
            vpMatchedKeyPoints12.push_back(std::pair<int, int>(i1, i2));
        }
        mvpMatchedPointsNum12[pKF1] = pairStart[p + 1] - pairStart[p];
        mvpMatchedPoints12[pKF1] = vpMatchedPoints12;
        mvpMatchedKeyPoints12[pKF1] = vpMatchedKeyPoints12;
        mvpValidMatchedKeyPoints12[pKF1] = vpMatchedKeyPoints12;
        p++;
    }
    return pairStart[f1.size()];
}

}  // namespace rumi_facade
