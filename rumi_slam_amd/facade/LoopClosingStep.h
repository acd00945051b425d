// Facade for the BoW stage of LoopClosing::DetectCommonRegionsFromBoW (R/lib_src/LoopClosing.cc:576-651) and of its twin in CloudMerging
// (R/lib_src/CloudMerging.cc:1019-1094): for every BoW candidate, the candidate and its best covisibles are matched against the current key-frame
// with SearchByBoW(KF, KF) and the match vectors are folded into vpMatchedPoints / vpKeyFrameMatchedMP.  All candidates, all members and the folds
// go to the GPU in one call (include/rumi_match.h: rumi_common_regions_bow); this side applies the checks that need no device, marshals the
// key-frames and hands back, per candidate, what the loop body from :655 on reads.  That body (the Sim3 solver, the two SearchByProjection passes,
// OptimizeSim3, the covisible check) stays where it is and runs through the entries it already has.
//
// Templated on the key-frame, map-point and matcher types, so that it instantiates against the reference's classes and against the stand-ins of
// tests/cpp.  Mono key-frames only.
#pragma once
#include <cstdint>
#include <set>
#include <unordered_map>
#include <vector>

#include "rumi_match.h"
#include "rumi_status.h"

namespace rumi_facade {

// What one candidate's pass through :576-651 leaves behind, under the reference's names.
template <class KeyFrameT, class MapPointT> struct BowStageResult {
    KeyFrameT *pKFi = nullptr;                               // the candidate (= pMostBoWMatchesKF, :614)
    std::vector<KeyFrameT *> vpCovKFi;                       // candidate first, the displaced covisible appended (:583-591)
    std::vector<std::vector<MapPointT *>> vvpMatchedMPs;     // [j]: empty for a bad or NULL member (:623), else sized to the current key-frame's slots
    std::vector<MapPointT *> vpMatchedPoints;
    std::vector<KeyFrameT *> vpKeyFrameMatchedMP;
    int numBoWMatches = 0, nIndexMostBoWMatchesKF = 0, nMostBoWNumMatches = 0;
};

namespace loopclosing_detail {
struct Member {
    std::vector<uint32_t> nodes, idx;
    std::vector<int32_t> off, mp;
};
template <class FeatVecT> inline void csr(const FeatVecT &fv, Member &m) {      // DBoW2::FeatureVector = std::map<NodeId, std::vector<unsigned>>
    m.off.push_back(0);
    for (const auto &kv : fv) {
        m.nodes.push_back((uint32_t)kv.first);
        for (unsigned i : kv.second) m.idx.push_back(i);
        m.off.push_back((int32_t)m.idx.size());
    }
}
}  // namespace loopclosing_detail

// Runs :576-651 for every candidate of vpBowCand.  `out` receives one entry per candidate that is neither skipped (NULL or bad, :577) nor aborted
// (one of its members is connected to the current key-frame, :593-605), in vpBowCand's order.  Returns out.size(), or -1 with `out` empty and a
// report through rumi_status.h: a key-frame with NLeft != -1 (the two-camera branches of SearchByBoW are not built), or a failed device call.
// matcherBoW: the caller's ORBmatcher(0.9, true) (:555, facade/ORBmatcher.h): its ratio and orientation flag are read through NNRatio() /
// CheckOrientation(), and the call runs on its per-thread arena (the call's own blocks grow on demand; should a member's FeatureVector node exceed what
// the batch kernel holds, the library runs single searches on that arena, which grows as for ORBmatcher's own calls).
template <class KeyFrameT, class MapPointT, class MatcherT>
int CommonRegionsBoWStage(KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpBowCand, int nNumCovisibles, const MatcherT &matcherBoW,
                          std::vector<BowStageResult<KeyFrameT, MapPointT>> &out) {
    namespace D = loopclosing_detail;
    static const char *where = "LoopClosingStep::CommonRegionsBoWStage / rumi_common_regions_bow";
    out.clear();
    const std::set<KeyFrameT *> spConnectedKeyFrames = pCurrentKF->GetConnectedKeyFrames();
    const std::vector<MapPointT *> vpCurrentMPs = pCurrentKF->GetMapPointMatches();
    bool twoCameras = pCurrentKF->NLeft != -1;

    // ---- the groups: what needs no device ----
    std::unordered_map<KeyFrameT *, int> tableIndex;
    std::vector<KeyFrameT *> table;
    std::vector<int32_t> groupStart(1, 0), memberKf;
    std::vector<std::vector<int>> memberPos;                  // per result: the vpCovKFi position of every member that was sent
    for (KeyFrameT *pKFi : vpBowCand) {
        if (!pKFi || pKFi->isBad()) continue;
        BowStageResult<KeyFrameT, MapPointT> r;
        r.pKFi = pKFi;
        r.vpCovKFi = pKFi->GetBestCovisibilityKeyFrames(nNumCovisibles);
        if (r.vpCovKFi.empty()) r.vpCovKFi.push_back(pKFi);
        else { r.vpCovKFi.push_back(r.vpCovKFi[0]); r.vpCovKFi[0] = pKFi; }
        bool bAbortByNearKF = false;
        for (KeyFrameT *pKFj : r.vpCovKFi)
            if (spConnectedKeyFrames.count(pKFj)) { bAbortByNearKF = true; break; }
        if (bAbortByNearKF) continue;
        std::vector<int> pos;
        for (size_t j = 0; j < r.vpCovKFi.size(); j++) {
            KeyFrameT *pKFj = r.vpCovKFi[j];
            if (!pKFj || pKFj->isBad()) continue;
            twoCameras = twoCameras || pKFj->NLeft != -1;
            auto it = tableIndex.find(pKFj);
            if (it == tableIndex.end()) { it = tableIndex.emplace(pKFj, (int)table.size()).first; table.push_back(pKFj); }
            memberKf.push_back(it->second);
            pos.push_back((int)j);
        }
        groupStart.push_back((int32_t)memberKf.size());
        memberPos.push_back(pos);
        r.vvpMatchedMPs.resize(r.vpCovKFi.size());
        r.vpMatchedPoints.assign(vpCurrentMPs.size(), static_cast<MapPointT *>(nullptr));
        r.vpKeyFrameMatchedMP.assign(vpCurrentMPs.size(), static_cast<KeyFrameT *>(nullptr));
        out.push_back(r);
    }
    if (twoCameras) {
        // (the reason travels in the call site's name: the status did not come from the library, so its error string says nothing here)
        RUMI_GUARDED("LoopClosingStep::CommonRegionsBoWStage: a key-frame with NLeft != -1 (only the monocular SearchByBoW is built; no candidate was matched)",
                     &no_growth, RUMI_E_INVALID);
        out.clear();
        return -1;
    }
    if (out.empty()) return 0;

    // ---- marshal: every distinct member once, one numbering of the map points over all of them ----
    std::unordered_map<MapPointT *, int> idOf;
    std::vector<MapPointT *> byId;
    std::vector<uint8_t> bad;
    std::vector<D::Member> data(table.size());
    std::vector<std::vector<MapPointT *>> slots(table.size());
    std::vector<RumiBowKeyFrame> kfs(table.size());
    for (size_t k = 0; k < table.size(); k++) {
        KeyFrameT *pKF = table[k];
        slots[k] = pKF->GetMapPointMatches();
        D::Member &d = data[k];
        D::csr(pKF->mFeatVec, d);
        d.mp.assign((size_t)pKF->N, -1);
        for (size_t i = 0; i < slots[k].size() && i < d.mp.size(); i++) {
            MapPointT *pMP = slots[k][i];
            if (!pMP) continue;
            auto it = idOf.find(pMP);
            if (it == idOf.end()) { it = idOf.emplace(pMP, (int)byId.size()).first; byId.push_back(pMP); bad.push_back(pMP->isBad()); }
            d.mp[i] = it->second;
        }
        kfs[k].feat = MatcherT::view(*pKF);
        kfs[k].fv = RumiFeatureVector{(int32_t)d.nodes.size(), d.nodes.data(), d.off.data(), d.idx.data()};
        kfs[k].mp = d.mp.data();
    }
    D::Member cur;
    D::csr(pCurrentKF->mFeatVec, cur);
    const RumiFrameFeatures curView = MatcherT::view(*pCurrentKF);
    const RumiFeatureVector curFv{(int32_t)cur.nodes.size(), cur.nodes.data(), cur.off.data(), cur.idx.data()};
    const size_t n = (size_t)pCurrentKF->N, G = out.size(), M = memberKf.size();
    std::vector<uint8_t> curGood(n + 1, 0);
    for (size_t i = 0; i < n && i < vpCurrentMPs.size(); i++) curGood[i] = vpCurrentMPs[i] && !vpCurrentMPs[i]->isBad();
    bad.push_back(0);                                        // (never an empty array)
    std::vector<int32_t> matches12(M * n + 1), nmatches(M + 1), matchedPoint(G * n + 1), matchedMember(G * n + 1), numBow(G + 1), most(2 * G + 2);
    if (!MatcherT::arena()) { out.clear(); return -1; }      // reported by arena()
    if (RUMI_GUARDED(where, &MatcherT::grow_arena,
                     rumi_common_regions_bow(MatcherT::arena(), &curView, &curFv, curGood.data(), (int32_t)kfs.size(), kfs.data(), (int32_t)byId.size(), bad.data(), (int32_t)G,
                                             groupStart.data(), memberKf.data(), matcherBoW.NNRatio(), matcherBoW.CheckOrientation(), matches12.data(),
                                             nmatches.data(), matchedPoint.data(), matchedMember.data(), numBow.data(), most.data())) != RUMI_OK) {
        out.clear();
        return -1;
    }

    // ---- back to pointers; a member's position inside its group becomes its position in vpCovKFi ----
    for (size_t g = 0; g < G; g++) {
        BowStageResult<KeyFrameT, MapPointT> &r = out[g];
        const std::vector<int> &pos = memberPos[g];
        for (size_t jj = 0; jj < pos.size(); jj++) {
            const size_t mem = (size_t)groupStart[g] + jj;
            const std::vector<MapPointT *> &s2 = slots[memberKf[mem]];
            std::vector<MapPointT *> &v = r.vvpMatchedMPs[pos[jj]];
            v.assign(vpCurrentMPs.size(), static_cast<MapPointT *>(nullptr));
            for (size_t k = 0; k < n && k < v.size(); k++) {
                const int f = matches12[mem * n + k];
                if (f >= 0) v[k] = s2[f];
            }
        }
        for (size_t k = 0; k < n && k < r.vpMatchedPoints.size(); k++) {
            const int id = matchedPoint[g * n + k], jj = matchedMember[g * n + k];
            if (id < 0) continue;
            r.vpMatchedPoints[k] = byId[id];
            r.vpKeyFrameMatchedMP[k] = r.vpCovKFi[pos[jj]];
        }
        r.numBoWMatches = numBow[g];
        r.nMostBoWNumMatches = most[2 * g + 1];
        r.nIndexMostBoWMatchesKF = pos.empty() ? 0 : pos[most[2 * g]];
    }
    return (int)out.size();
}

}  // namespace rumi_facade
