// Facade for the BoW stage of LoopClosing::DetectCommonRegionsFromBoW (R/lib_src/LoopClosing.cc:576-651) and of its twin in CloudMerging
// (R/lib_src/CloudMerging.cc:1019-1094): for every BoW candidate, the candidate and its best covisibles are matched against the current key-frame
// with SearchByBoW(KF, KF) and the match vectors are folded into vpMatchedPoints / vpKeyFrameMatchedMP.  All candidates, all members and the folds
// go to the GPU in one call (include/rumi_match.h: rumi_common_regions_bow); this side applies the checks that need no device, marshals the
// key-frames and hands back, per candidate, what the loop body from :655 on reads (CommonRegionsBoWStageResident: the same over a
// CovisibilityGraph that holds the map, by slot -- include/rumi_mapping.h: rumi_common_regions_bow_resident -- with nothing to marshal).  That body (the Sim3 solver, the two SearchByProjection passes,
// OptimizeSim3, the covisible check) stays where it is; its SearchByProjection passes and the covisible check have one-call members below, the
// Sim3 solvers and OptimizeSim3 of all candidates in PlaceRecognitionStages.h (Sim3RansacStage, OptimizeSim3Stage).
//
// Templated on the key-frame, map-point and matcher types, so that it instantiates against the reference's classes and against the stand-ins of
// tests/cpp.  Mono key-frames only.
//
// With RUMI_HAVE_SOPHUS, LoopClosing::SearchAndFuse (R/lib_src/LoopClosing.cc:1996-2065) over a CovisibilityGraph that holds the map becomes
//     rumi::LoopClosingStep step;                                    // = ORBmatcher matcher(0.8)
//     step.SearchAndFuseResident(graph, poses, vpMapPoints);         // poses: (KeyFrame *, Sophus::Sim3f) in CorrectedPosesMap's order
//     step.SearchAndFuseResident(graph, vConectedKFs, vpMapPoints);  // the overload that searches under GetPose(), scale 1
// and the SearchByProjection(KF, Scw, ...) searches of DetectCommonRegionsFromBoW (:716, :738, the covisible check :773-795) become
//     step.SearchByProjectionResident(graph, jobs);                  // one Sim3ProjectionJob per call of the reference's member
//     step.CovisibleCheckResident(graph, pCurrentKF, pMostBoWMatchesKF, gScw, vpCurrentCovKFs, vpMapPoints, &nNumKFs, Converter::toSophus);
//     step.CovisibleCheckResident(graph, pCurrentKF, candidates, vpCurrentCovKFs, Converter::toSophus);   // several candidates, one call
//     step.DetectCommonRegionsFromBoWResident(graph, pCurrentKF, vpBowCand, spConnectedKeyFrames, matcherBoW, mbFixScale, false, thresholds, ...);   // the whole function
// (at the end of this header).
#pragma once
#include <cstdint>
#include <set>
#include <unordered_map>
#include <vector>

#include "rumi_mapping.h"
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
// :576-605 and :623 for every candidate, the part of the stage that needs no device and is the same by host pointers and by slot: the skips, the
// displaced covisible, the abort by a connected key-frame, bad and NULL members left out.  `out` gets one entry per surviving candidate with its
// vectors sized; member / groupStart: the key-frames that are searched, group after group; memberPos[g]: their positions in vpCovKFi.
template <class KeyFrameT, class MapPointT> struct BowGroups {
    std::vector<int32_t> groupStart = std::vector<int32_t>(1, 0);
    std::vector<KeyFrameT *> member;
    std::vector<std::vector<int>> memberPos;
    bool twoCameras = false;
};
template <class KeyFrameT, class MapPointT>
inline void bow_groups(KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpBowCand, const std::set<KeyFrameT *> &spConnectedKeyFrames, int nNumCovisibles,
                       size_t nSlots, std::vector<BowStageResult<KeyFrameT, MapPointT>> &out, BowGroups<KeyFrameT, MapPointT> &G) {
    G.twoCameras = pCurrentKF->NLeft != -1;
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
            G.twoCameras = G.twoCameras || pKFj->NLeft != -1;
            G.member.push_back(pKFj);
            pos.push_back((int)j);
        }
        G.groupStart.push_back((int32_t)G.member.size());
        G.memberPos.push_back(pos);
        r.vvpMatchedMPs.resize(r.vpCovKFi.size());
        r.vpMatchedPoints.assign(nSlots, static_cast<MapPointT *>(nullptr));
        r.vpKeyFrameMatchedMP.assign(nSlots, static_cast<KeyFrameT *>(nullptr));
        out.push_back(r);
    }
}
}  // namespace loopclosing_detail

// Runs :576-651 for every candidate of vpBowCand.  `out` receives one entry per candidate that is neither skipped (NULL or bad, :577) nor aborted
// (one of its members is connected to the current key-frame, :593-605), in vpBowCand's order.  Returns out.size(), or -1 with `out` empty and a
// report through rumi_status.h: a key-frame with NLeft != -1 (the two-camera branches of SearchByBoW are not built), or a failed device call.
// matcherBoW: the caller's ORBmatcher(0.9, true) (:555, facade/ORBmatcher.h): its ratio and orientation flag are read through NNRatio() /
// CheckOrientation(), and the call runs on its per-thread arena (the call's own blocks grow on demand; a member's FeatureVector node of any size up to
// 65535 features is searched in the same launch).
// spConnectedKeyFrames: mpCurrentKF->GetConnectedKeyFrames() as :551 takes it once for the whole function; the overload without it asks the key-frame.
template <class KeyFrameT, class MapPointT, class MatcherT>
int CommonRegionsBoWStage(KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpBowCand, const std::set<KeyFrameT *> &spConnectedKeyFrames, int nNumCovisibles,
                          const MatcherT &matcherBoW, std::vector<BowStageResult<KeyFrameT, MapPointT>> &out) {
    namespace D = loopclosing_detail;
    static const char *where = "LoopClosingStep::CommonRegionsBoWStage / rumi_common_regions_bow";
    out.clear();
    const std::vector<MapPointT *> vpCurrentMPs = pCurrentKF->GetMapPointMatches();
    // ---- the groups: what needs no device ----
    D::BowGroups<KeyFrameT, MapPointT> groups;
    D::bow_groups(pCurrentKF, vpBowCand, spConnectedKeyFrames, nNumCovisibles, vpCurrentMPs.size(), out, groups);
    const bool twoCameras = groups.twoCameras;
    const std::vector<int32_t> &groupStart = groups.groupStart;
    const std::vector<std::vector<int>> &memberPos = groups.memberPos;
    std::unordered_map<KeyFrameT *, int> tableIndex;
    std::vector<KeyFrameT *> table;                          // every distinct member once
    std::vector<int32_t> memberKf;
    for (KeyFrameT *pKFj : groups.member) {
        auto it = tableIndex.find(pKFj);
        if (it == tableIndex.end()) { it = tableIndex.emplace(pKFj, (int)table.size()).first; table.push_back(pKFj); }
        memberKf.push_back(it->second);
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
template <class KeyFrameT, class MapPointT, class MatcherT>
int CommonRegionsBoWStage(KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpBowCand, int nNumCovisibles, const MatcherT &matcherBoW,
                          std::vector<BowStageResult<KeyFrameT, MapPointT>> &out) {
    const std::set<KeyFrameT *> spConnectedKeyFrames = pCurrentKF->GetConnectedKeyFrames();
    return CommonRegionsBoWStage(pCurrentKF, vpBowCand, spConnectedKeyFrames, nNumCovisibles, matcherBoW, out);
}

// The same stage over a CovisibilityGraph that holds the map (rumi_common_regions_bow_resident, include/rumi_mapping.h): the host
// logic above, then graph.FlushDirty(), key-frames to slots and ONE call that sends slot numbers and nothing else of a key-frame -- no walk over
// mFeatVec or GetMapPointMatches() of the members, no renumbering of their points; the device reads features, rows and bad bits in the store,
// and the matched point ids come back to MapPoint* through the graph's own map.  Every field of BowStageResult is filled as the stage above fills
// it, for a graph that is current (rows and bad bits staged: graph.Sync); vvpMatchedMPs[j] is filled only with wantMemberMatches (nothing after
// the union reads it, LoopClosing.cc:608-638, and without it the [members][slots] block stays on the device), else every vvpMatchedMPs[j] is empty.
// GraphT: CovisibilityGraph, or anything with its ok / SlotOf / HasFeatures / FlushDirty / handle / PointAt.
// Returns out.size(), or -1 with `out` cleared and a report: NLeft != -1 on a key-frame, no store, the current key-frame or a member the graph
// has never seen or without SyncFeatures, a current key-frame whose N is not the length of its row in the store, a failed call.  With notResident the third case is not reported: *notResident is set instead, for a
// caller that then takes the stage above (DetectCommonRegionsFromBoWResident).
template <class GraphT, class KeyFrameT, class MapPointT, class MatcherT>
int CommonRegionsBoWStageResident(GraphT &graph, KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpBowCand, const std::set<KeyFrameT *> &spConnectedKeyFrames,
                                  int nNumCovisibles, const MatcherT &matcherBoW, std::vector<BowStageResult<KeyFrameT, MapPointT>> &out, bool wantMemberMatches,
                                  bool *notResident = nullptr) {
    namespace D = loopclosing_detail;
    static const char *where = "LoopClosingStep::CommonRegionsBoWStageResident / rumi_common_regions_bow_resident";
    out.clear();
    if (notResident) *notResident = false;
    const size_t nSlots = pCurrentKF->GetMapPointMatches().size();
    D::BowGroups<KeyFrameT, MapPointT> groups;
    D::bow_groups(pCurrentKF, vpBowCand, spConnectedKeyFrames, nNumCovisibles, nSlots, out, groups);
    if (groups.twoCameras) {
        RUMI_GUARDED("LoopClosingStep::CommonRegionsBoWStageResident: a key-frame with NLeft != -1 (only the monocular SearchByBoW is built; no candidate was matched)",
                     &no_growth, RUMI_E_INVALID);
        out.clear();
        return -1;
    }
    if (out.empty()) return 0;
    if (!graph.ok()) { report(where, RUMI_E_INVALID, "no store; no candidate was matched"); out.clear(); return -1; }
    std::vector<int32_t> memberSlot;
    bool resident = graph.SlotOf(pCurrentKF) >= 0 && graph.HasFeatures(pCurrentKF);
    for (KeyFrameT *pKFj : groups.member) {
        resident = resident && graph.SlotOf(pKFj) >= 0 && graph.HasFeatures(pKFj);
        memberSlot.push_back(graph.SlotOf(pKFj));
    }
    if (!resident) {
        if (notResident) *notResident = true;
        else report(where, RUMI_E_INVALID, "a key-frame the graph has never seen or without resident features (graph.Sync, graph.SyncFeatures); nothing was uploaded, no candidate was matched");
        out.clear();
        return -1;
    }
    // the entry writes rows of the store's feature count for the current slot: the buffers below are sized by N, so the two must agree
    if (rumi_covis_row_length(graph.handle(), graph.SlotOf(pCurrentKF)) != (int32_t)pCurrentKF->N) {
        report(where, RUMI_E_INVALID, "the current key-frame's N differs from the row the store holds for it (graph.Sync after the key-frame changed); no candidate was matched");
        out.clear();
        return -1;
    }
    if (graph.FlushDirty() != RUMI_OK) { out.clear(); return -1; }
    const size_t n = (size_t)pCurrentKF->N, G = out.size(), M = memberSlot.size();
    memberSlot.push_back(-1);                                // (never an empty array)
    std::vector<int32_t> matches12(wantMemberMatches ? M * n + 1 : 0), nmatches(M + 1), matchedPoint(G * n + 1), matchedMember(G * n + 1), numBow(G + 1), most(2 * G + 2);
    if (!MatcherT::arena()) { out.clear(); return -1; }      // reported by arena()
    if (RUMI_GUARDED(where, &MatcherT::grow_arena,
                     rumi_common_regions_bow_resident(MatcherT::arena(), graph.handle(), graph.SlotOf(pCurrentKF), (int32_t)G, groups.groupStart.data(), memberSlot.data(),
                                                      matcherBoW.NNRatio(), matcherBoW.CheckOrientation(), wantMemberMatches ? matches12.data() : nullptr,
                                                      nmatches.data(), matchedPoint.data(), matchedMember.data(), numBow.data(), most.data())) != RUMI_OK) {
        out.clear();
        return -1;
    }
    // ---- back to pointers; a member's position inside its group becomes its position in vpCovKFi ----
    for (size_t g = 0; g < G; g++) {
        BowStageResult<KeyFrameT, MapPointT> &r = out[g];
        const std::vector<int> &pos = groups.memberPos[g];
        for (size_t jj = 0; wantMemberMatches && jj < pos.size(); jj++) {
            const size_t mem = (size_t)groups.groupStart[g] + jj;
            const std::vector<MapPointT *> s2 = groups.member[mem]->GetMapPointMatches();
            std::vector<MapPointT *> &v = r.vvpMatchedMPs[pos[jj]];
            v.assign(nSlots, static_cast<MapPointT *>(nullptr));
            for (size_t k = 0; k < n && k < v.size(); k++) {
                const int f = matches12[mem * n + k];
                if (f >= 0 && (size_t)f < s2.size()) v[k] = s2[f];
            }
        }
        for (size_t k = 0; k < n && k < r.vpMatchedPoints.size(); k++) {
            const int id = matchedPoint[g * n + k], jj = matchedMember[g * n + k];
            if (id < 0) continue;
            r.vpMatchedPoints[k] = graph.PointAt(id);
            r.vpKeyFrameMatchedMP[k] = r.vpCovKFi[pos[jj]];
        }
        r.numBoWMatches = numBow[g];
        r.nMostBoWNumMatches = most[2 * g + 1];
        r.nIndexMostBoWMatchesKF = pos.empty() ? 0 : pos[most[2 * g]];
    }
    return (int)out.size();
}

}  // namespace rumi_facade

#ifdef RUMI_HAVE_SOPHUS
#include <cstring>
#include <mutex>
#include <type_traits>
#include <utility>

#include "ORBmatcher.h"
#include "PlaceRecognitionStages.h"
#include "rumi_mapping.h"

namespace RUMI_FACADE_NAMESPACE {

// LoopClosing::SearchAndFuse (R/lib_src/LoopClosing.cc:1996-2028 and :2030-2065) over a CovisibilityGraph that holds the map: graph.FlushDirty();
// ONE device call answers every (key-frame, loop point) search from the store as it stands (rumi_search_and_fuse_resident, include/rumi_mapping.h);
// then the reference's own objects replay :2003-2026 key-frame by key-frame.  At a key-frame's turn spAlreadyFound is taken, isBad() is asked
// per point, GetMapPoint(bestIdx) is read live (a point added earlier in the same key-frame is the occupant), AddObservation / AddMapPoint
// happen at once, vpReplacePoints is filled and the Replace loop runs after the key-frame under the map's update mutex.
// Replace ends with ComputeDistinctiveDescriptors() on the survivor, always the loop point here (MapPoint.cc:321): a loop point whose
// GetDescriptor() a Replace changed is searched again, on its live descriptor, for every key-frame that follows, before its turn (one small
// rumi_fuse_candidates call per such key-frame, without the reprojection gate; *nSearchedAgain counts the pairs).  DESIGN.md 4v has the
// argument why nothing else the device read can change.  The touched key-frames and points are staged again (Sync, MarkDirty), so the graph
// is current when the member returns.
// Returns the key-frames' nFused together, or -1 with a report and nothing mutated: NLeft != -1 on any key-frame, a key-frame or point the
// graph has never seen, a key-frame without resident features or a searched point without attributes, more key-frames than
// RUMI_FUSE_MAX_TARGETS, a failed device call.  The caller keeps the reference's member for those.  (A second search that fails ends the
// member with -1 after the key-frames replayed so far, which stay, staged.)
class LoopClosingStep : public ORBmatcher {
public:
    LoopClosingStep() : ORBmatcher(0.8f, true) {}            // `ORBmatcher matcher(0.8)`, LoopClosing.cc:1997

    // kfs: an ordered range of (KeyFrameT *, Sophus::Sim3f) -- CorrectedPosesMap with its g2o::Sim3 through Converter::toSophus, in the order the
    // map iterates (:2003-2009) -- or a std::vector<KeyFrameT *>, each searched under `Sim3f(GetPose().unit_quaternion(), GetPose().translation())`
    // with scale 1 (:2041-2043).  Sim3T is Sophus::Sim3f; a parameter so that tests/cpp's stand-in, which lacks that constructor, can stand in.
    template <class Sim3T = Sophus::Sim3f, class GraphT, class RangeT, class MapPointT>
    int SearchAndFuseResident(GraphT &graph, const RangeT &kfs, std::vector<MapPointT *> &vpMapPoints, int *nSearchedAgain = nullptr) {
        return saf_dispatch<Sim3T>(graph, kfs, vpMapPoints, nSearchedAgain, typename std::is_pointer<typename RangeT::value_type>::type());
    }

    // ---- The SearchByProjection(KeyFrame*, Sim3f&, points, ...) searches of DetectCommonRegionsFromBoW (LoopClosing.cc:716, :738, :773-795;
    // CloudMerging.cc:1157, 1179, 1226 are the same text) over a CovisibilityGraph that holds the map: the jobs of a stage in ONE device call
    // (rumi_search_by_projection_sim3_resident, include/rumi_mapping.h).  The member changes no map, so there is no replay.
    // One call of the reference's member.  vpPointsKFs / vpMatchedKF: both set for the overload of ORBmatcher.cc:473-579, both null for
    // :372-471.  *vpMatched (and *vpMatchedKF) are what the call sites hand over: all NULL; the member sizes them to the key-frame's
    // features and fills them as the overload would have.  A point list that several jobs name is sent once.
    template <class KeyFrameT, class MapPointT> struct Sim3ProjectionJob {
        KeyFrameT *pKF;
        Sophus::Sim3f Scw;
        const std::vector<MapPointT *> *vpPoints;
        const std::vector<KeyFrameT *> *vpPointsKFs;
        int th;
        float ratioHamming;
        std::vector<MapPointT *> *vpMatched;
        std::vector<KeyFrameT *> *vpMatchedKF;
        int *nmatches;
    };

    // Serves :716 and :738 across all candidates that reached those lines.  Returns the number of jobs, or -1 with a report and nothing
    // written: NLeft != -1, a key-frame the graph has never seen or without SyncFeatures, a point the graph has never seen, a searched point
    // without attributes (found by the device call), a failed device call (more jobs than RUMI_FUSE_MAX_TARGETS among them).
    template <class GraphT, class KeyFrameT, class MapPointT>
    int SearchByProjectionResident(GraphT &graph, const std::vector<Sim3ProjectionJob<KeyFrameT, MapPointT>> &jobs) {
        static const char *where = "LoopClosingStep::SearchByProjectionResident";
        if (!graph.ok()) { rumi_facade::report(where, RUMI_E_INVALID, "no store; nothing was searched"); return -1; }
        std::vector<RumiSim3ProjJob> rec;
        std::vector<int32_t> ids;
        std::vector<std::pair<const std::vector<MapPointT *> *, int32_t>> sent;      // a list and where it starts in ids
        size_t rows = 0;
        for (const auto &J : jobs) {
            KeyFrameT *pKF = J.pKF;
            if (pKF->NLeft != -1) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame with NLeft != -1: only the monocular SearchByProjection is built; nothing was searched");
                return -1;
            }
            if (graph.SlotOf(pKF) < 0 || !graph.HasFeatures(pKF)) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame the graph has never seen or without resident features (graph.Sync, graph.SyncFeatures); nothing was uploaded, nothing was searched");
                return -1;
            }
            int32_t start = -1;
            for (const auto &s : sent) if (s.first == J.vpPoints) start = s.second;
            if (start < 0) {
                start = (int32_t)ids.size();
                for (MapPointT *pMP : *J.vpPoints) {
                    if (!pMP) { ids.push_back(-1); continue; }
                    if (!graph.HasPoint(pMP)) {
                        rumi_facade::report(where, RUMI_E_INVALID, "a point the graph has never seen (graph.Sync, graph.SyncAttributes); nothing was uploaded, nothing was searched");
                        return -1;
                    }
                    ids.push_back(graph.IdOf(pMP));
                }
                sent.emplace_back(J.vpPoints, start);
            }
            Sophus::Sim3f Scw = J.Scw;                                              // ORBmatcher.cc:380-381 / :481-482, as searchSim3 (ORBmatcher.h) forms them
            const Sophus::SE3f Tcw = Sophus::SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale());
            const Eigen::Vector3f Ow = Tcw.inverse().translation();
            const auto q = Tcw.unit_quaternion();
            RumiSim3ProjJob r;
            r.kf_slot = graph.SlotOf(pKF);
            r.kf.Tcw7[0] = q.x(); r.kf.Tcw7[1] = q.y(); r.kf.Tcw7[2] = q.z(); r.kf.Tcw7[3] = q.w();
            for (int c = 0; c < 3; c++) { r.kf.Tcw7[4 + c] = Tcw.translation()(c); r.kf.Ow[c] = Ow(c); }
            r.kf.bounds[0] = pKF->mnMinX; r.kf.bounds[1] = pKF->mnMinY; r.kf.bounds[2] = pKF->mnMaxX; r.kf.bounds[3] = pKF->mnMaxY;
            r.kf.log_scale_factor = pKF->mfLogScaleFactor;
            r.point_start = start; r.point_count = (int32_t)J.vpPoints->size();
            r.th = J.th; r.ratio_hamming = J.ratioHamming; r.explicit_invz = J.vpPointsKFs ? 1 : 0;
            rec.push_back(r);
            rows += (size_t)pKF->N;
        }
        if (jobs.empty()) return 0;
        if (graph.FlushDirty() != RUMI_OK) return -1;
        const int nJ = (int)jobs.size();
        std::vector<int32_t> matched(rows + 1), start((size_t)nJ + 1), nm((size_t)nJ);
        ids.push_back(-1);                                                          // (never an empty array)
        if (!arena()) return -1;                                                    // reported by arena()
        if (RUMI_GUARDED("LoopClosingStep / rumi_search_by_projection_sim3_resident", &ORBmatcher::grow_arena,
                         rumi_search_by_projection_sim3_resident(arena(), graph.handle(), rec.data(), nJ, ids.data(), (int32_t)ids.size() - 1, matched.data(),
                                                                 start.data(), (int32_t)rows, nm.data())) != RUMI_OK)
            return -1;
        for (int j = 0; j < nJ; j++) {                                              // :465 / :573-574 from the returned positions
            const auto &J = jobs[j];
            const int N = J.pKF->N;
            J.vpMatched->assign((size_t)N, static_cast<MapPointT *>(nullptr));
            if (J.vpMatchedKF) J.vpMatchedKF->assign((size_t)N, static_cast<KeyFrameT *>(nullptr));
            for (int f = 0; f < N; f++) {
                const int i = matched[(size_t)start[j] + f];
                if (i < 0) continue;
                (*J.vpMatched)[f] = (*J.vpPoints)[i];
                if (J.vpMatchedKF && J.vpPointsKFs) (*J.vpMatchedKF)[f] = (*J.vpPointsKFs)[i];
            }
            if (J.nmatches) *J.nmatches = nm[j];
        }
        return nJ;
    }

    // The loop :773-795 for one candidate: `while (nNumKFs < 3 && j < vpCurrentCovKFs.size())` over DetectCommonRegionsFromLastKF (:855-866)
    // -> FindMatchesByProjection (:868-914).  The list of :871-905 is built ONCE: it depends on the matched key-frame alone (spCheckKFs and
    // spCurrentCovisbles, the only things the covisible enters, reach nothing that leaves the function).  gSjw is formed per covisible as
    // :779-781 do and every covisible is searched in one call (th 3, ratio 1.5, :911); then the while loop is replayed over the counts with
    // the threshold 30 of :860-861.  The covisibles after the third valid one are searched SPECULATIVELY and passed over: the reference would
    // not have searched them, and nothing of their answers leaves this member.  vpMapPoints is left as the member leaves it, cleared and
    // refilled through the reference parameter (:893-905); with no covisible it is untouched, as in the reference.
    // toSophus: Converter::toSophus (g2o::Sim3 -> Sophus::Sim3f).  Returns the covisibles the loop visited, or -1 with a report, nNumKFs and
    // vpMapPoints untouched (the refusals of SearchByProjectionResident).
    template <class GraphT, class KeyFrameT, class MapPointT, class G2oSim3T, class ToSophusT>
    int CovisibleCheckResident(GraphT &graph, KeyFrameT *pCurrentKF, KeyFrameT *pMostBoWMatchesKF, const G2oSim3T &gScw,
                               const std::vector<KeyFrameT *> &vpCurrentCovKFs, std::vector<MapPointT *> &vpMapPoints, int *nNumKFs, ToSophusT toSophus) {
        std::vector<CovisibleCheckCandidate<KeyFrameT, MapPointT, G2oSim3T>> one(1, CovisibleCheckCandidate<KeyFrameT, MapPointT, G2oSim3T>{pMostBoWMatchesKF, gScw, &vpMapPoints, nNumKFs, 0});
        if (CovisibleCheckResident(graph, pCurrentKF, one, vpCurrentCovKFs, toSophus) < 0) return -1;
        return one[0].visited;
    }

    // The same loop for SEVERAL candidates that reached :768 (each with its own pMostBoWMatchesKF and gScw): the covisibles of the current key-frame
    // are the same for all of them, so every (candidate, covisible) search is a job of ONE device call, each candidate's list sent once; then
    // `nNumKFs < 3` is replayed per candidate over its counts.  Per candidate what the single member leaves: *vpMapPoints, *nNumKFs, and `visited`
    // = the covisibles its loop visited.  A candidate that arrives with nNumKFs >= 3 visits nothing: no list is built and nothing is searched for
    // it.  Returns the number of candidates, or -1 with a report and every candidate untouched (`visited` included).
    template <class KeyFrameT, class MapPointT, class G2oSim3T> struct CovisibleCheckCandidate {
        KeyFrameT *pMostBoWMatchesKF;
        G2oSim3T gScw;
        std::vector<MapPointT *> *vpMapPoints;
        int *nNumKFs;
        int visited;
    };
    template <class GraphT, class KeyFrameT, class MapPointT, class G2oSim3T, class ToSophusT>
    int CovisibleCheckResident(GraphT &graph, KeyFrameT *pCurrentKF, std::vector<CovisibleCheckCandidate<KeyFrameT, MapPointT, G2oSim3T>> &candidates,
                               const std::vector<KeyFrameT *> &vpCurrentCovKFs, ToSophusT toSophus) {
        const size_t nK = candidates.size(), nC = vpCurrentCovKFs.size();
        std::vector<uint8_t> runs(nK, 0);                                            // the candidates whose loop has anything to visit
        bool any = false;
        for (size_t k = 0; k < nK; k++) { runs[k] = nC > 0 && *candidates[k].nNumKFs < 3; any = any || runs[k]; }
        if (!any) { for (auto &c : candidates) c.visited = 0; return (int)nK; }
        std::vector<std::vector<MapPointT *>> vpLists(nK);                           // :871-905 per candidate
        for (size_t k = 0; k < nK; k++) {
            if (!runs[k]) continue;
            KeyFrameT *pMostBoWMatchesKF = candidates[k].pMostBoWMatchesKF;
            int nNumCovisibles = 10;
            std::vector<KeyFrameT *> vpCovKFm = pMostBoWMatchesKF->GetBestCovisibilityKeyFrames(nNumCovisibles);
            int nInitialCov = vpCovKFm.size();
            vpCovKFm.push_back(pMostBoWMatchesKF);
            if (nInitialCov < nNumCovisibles) {
                for (int i = 0; i < nInitialCov; ++i) {
                    std::vector<KeyFrameT *> vpKFs = vpCovKFm[i]->GetBestCovisibilityKeyFrames(nNumCovisibles);
                    vpCovKFm.insert(vpCovKFm.end(), vpKFs.begin(), vpKFs.end());
                }
            }
            std::set<MapPointT *> spMapPoints;
            for (KeyFrameT *pKFi : vpCovKFm) {
                for (MapPointT *pMPij : pKFi->GetMapPointMatches()) {
                    if (!pMPij || pMPij->isBad()) continue;
                    if (spMapPoints.find(pMPij) == spMapPoints.end()) { spMapPoints.insert(pMPij); vpLists[k].push_back(pMPij); }
                }
            }
        }
        std::vector<std::vector<MapPointT *>> vvpMatched(nK * nC);
        std::vector<int> num(nK * nC, 0);
        std::vector<Sim3ProjectionJob<KeyFrameT, MapPointT>> jobs;
        for (size_t k = 0; k < nK; k++)
            for (size_t j = 0; runs[k] && j < nC; j++) {
                KeyFrameT *pKFj = vpCurrentCovKFs[j];
                const Sophus::SE3f Tjc = pKFj->GetPose() * pCurrentKF->GetPoseInverse();     // :779: .cast<double>() widens each component
                const auto q = Tjc.unit_quaternion(); const auto t = Tjc.translation();
                G2oSim3T gSjc(Eigen::Quaterniond((double)q.w(), (double)q.x(), (double)q.y(), (double)q.z()), Eigen::Vector3d((double)t(0), (double)t(1), (double)t(2)), 1.0);
                G2oSim3T gSjw = gSjc * candidates[k].gScw;
                jobs.push_back(Sim3ProjectionJob<KeyFrameT, MapPointT>{pKFj, toSophus(gSjw), &vpLists[k], nullptr, 3, 1.5f, &vvpMatched[k * nC + j], nullptr, &num[k * nC + j]});
            }
        if (SearchByProjectionResident(graph, jobs) < 0) return -1;
        for (size_t k = 0; k < nK; k++) {
            if (!runs[k]) { candidates[k].visited = 0; continue; }
            size_t j = 0;                                                           // :775-795 over the counts
            int n = *candidates[k].nNumKFs;
            while (n < 3 && j < nC) {
                if (num[k * nC + j] >= 30) n++;                                     // :860-863
                j++;
            }
            if (j > 0) *candidates[k].vpMapPoints = vpLists[k];                     // every visited covisible leaves the same list
            *candidates[k].nNumKFs = n;
            candidates[k].visited = (int)j;
        }
        return (int)nK;
    }

    // ---- LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:542-853; CloudMerging.cc:1019 ff. is the same text) stage by stage over the members
    // above and PlaceRecognitionStages.h: (1) CommonRegionsBoWStageResident (CommonRegionsBoWStage by host pointers when a key-frame it searches is not resident), (2) Sim3RansacStage, (3) :716 of every candidate whose solver converged,
    // (4) OptimizeSim3Stage for numProjMatches >= nProjMatches, (5) :738 for numOptMatches >= nSim3Inliers, (6) the covisible check of every
    // candidate with numProjOptMatches >= nProjOptMatches, (7) the replay of :802-810 in candidate order (strict `<`: the first candidate wins a
    // tie) and :824-841 with SetNotErase().  Six device calls (more only when the RANSAC needs another round) whatever the number of candidates;
    // they are separate calls, not a fused kernel.  The outputs are the reference's reference parameters and are written at :824-841 only.
    // bInertialWithoutBA2: `mpTracker->mSensor == System::IMU_MONOCULAR && !GetIniertialBA2()` of :659 / :724 -- not built: refused.
    // Returns 1 / 0 = the function's true / false, or -1 with a report and every output untouched: that case, NLeft != -1, the refusals of the
    // members it calls.  (rand() has moved by then if the RANSAC stage ran.)
    struct PlaceRecognitionThresholds { int nBoWMatches = 20, nBoWInliers = 15, nSim3Inliers = 20, nProjMatches = 50, nProjOptMatches = 80, nNumCovisibles = 10; };
    template <class GraphT, class KeyFrameT, class MapPointT, class MatcherT, class G2oSim3T, class ToSophusT>
    int DetectCommonRegionsFromBoWResident(GraphT &graph, KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpBowCand, const std::set<KeyFrameT *> &spConnectedKeyFrames,
                                           const MatcherT &matcherBoW, bool mbFixScale, bool bInertialWithoutBA2, const PlaceRecognitionThresholds &th,
                                           KeyFrameT *&pMatchedKF2, KeyFrameT *&pLastCurrentKF, G2oSim3T &g2oScw, int &nNumCoincidences, std::vector<MapPointT *> &vpMPs,
                                           std::vector<MapPointT *> &vpMatchedMPs, ToSophusT toSophus) {
        static const char *where = "LoopClosingStep::DetectCommonRegionsFromBoWResident";
        if (bInertialWithoutBA2) { rumi_facade::report(where, RUMI_E_INVALID, "IMU_MONOCULAR before the second inertial BA is not built; nothing was searched"); return -1; }
        if (pCurrentKF->NLeft != -1) { rumi_facade::report(where, RUMI_E_INVALID, "a key-frame with NLeft != -1: only the monocular path is built; nothing was searched"); return -1; }
        std::vector<rumi_facade::BowStageResult<KeyFrameT, MapPointT>> bow;                            // (1) :576-651
        bool notResident = false;                                                                      // by slot when the graph holds the features of every key-frame searched
        int nBow = rumi_facade::CommonRegionsBoWStageResident(graph, pCurrentKF, vpBowCand, spConnectedKeyFrames, th.nNumCovisibles, matcherBoW, bow, false, &notResident);
        if (nBow < 0 && notResident) nBow = rumi_facade::CommonRegionsBoWStage(pCurrentKF, vpBowCand, spConnectedKeyFrames, th.nNumCovisibles, matcherBoW, bow);
        if (nBow < 0) return -1;
        std::vector<rumi_facade::Sim3RansacOutcome> ransac;                                            // (2) :655-676
        if (rumi_facade::Sim3RansacStage(pCurrentKF, bow, mbFixScale, th.nBoWMatches, th.nBoWInliers, ransac) < 0) return -1;
        struct Cand {
            KeyFrameT *pKFi;
            G2oSim3T gScm, gScw;
            std::vector<MapPointT *> vpMapPoints, vpMatchedMP, vpMatchedMP2;
            std::vector<KeyFrameT *> vpKeyFrames, vpMatchedKF;
            int numProjMatches = 0, numOptMatches = 0, numProjOptMatches = 0, nNumKFs = 0;
        };
        std::vector<Cand> cs;
        cs.reserve(bow.size());                                                                        // the jobs below point into it
        using Job = Sim3ProjectionJob<KeyFrameT, MapPointT>;
        std::vector<Job> jobs;
        for (size_t k = 0; k < bow.size(); k++) {                                                      // :676-716
            if (!ransac[k].bConverge) continue;
            cs.emplace_back();
            Cand &c = cs.back();
            c.pKFi = bow[k].pKFi;
            KeyFrameT *pMostBoWMatchesKF = c.pKFi;
            std::vector<KeyFrameT *> vpCovKFi = pMostBoWMatchesKF->GetBestCovisibilityKeyFrames(th.nNumCovisibles);
            vpCovKFi.push_back(pMostBoWMatchesKF);
            std::set<MapPointT *> spMapPoints;
            for (KeyFrameT *pCovKFi : vpCovKFi)
                for (MapPointT *pCovMPij : pCovKFi->GetMapPointMatches()) {
                    if (!pCovMPij || pCovMPij->isBad()) continue;
                    if (spMapPoints.find(pCovMPij) == spMapPoints.end()) { spMapPoints.insert(pCovMPij); c.vpMapPoints.push_back(pCovMPij); c.vpKeyFrames.push_back(pCovKFi); }
                }
            Eigen::Matrix3f R; Eigen::Vector3f t;
            for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) R(r, q) = ransac[k].R[r * 3 + q]; t(r) = ransac[k].t[r]; }
            c.gScm = G2oSim3T(R.template cast<double>(), t.template cast<double>(), (double)ransac[k].s);                                        // :706-708
            const G2oSim3T gSmw(pMostBoWMatchesKF->GetRotation().template cast<double>(), pMostBoWMatchesKF->GetTranslation().template cast<double>(), 1.0);
            c.gScw = c.gScm * gSmw;
            jobs.push_back(Job{pCurrentKF, toSophus(c.gScw), &c.vpMapPoints, &c.vpKeyFrames, 8, 1.5f, &c.vpMatchedMP, &c.vpMatchedKF, &c.numProjMatches});
        }
        if (SearchByProjectionResident(graph, jobs) < 0) return -1;                                    // (3) :716
        std::vector<rumi_facade::OptimizeSim3Job<KeyFrameT, MapPointT, G2oSim3T>> opt;
        for (Cand &c : cs)
            if (c.numProjMatches >= th.nProjMatches) opt.push_back(rumi_facade::OptimizeSim3Job<KeyFrameT, MapPointT, G2oSim3T>{pCurrentKF, c.pKFi, &c.vpMatchedMP, &c.gScm, 10.f, mbFixScale, true, &c.numOptMatches});
        if (rumi_facade::OptimizeSim3Stage(opt) < 0) return -1;                                        // (4) :728
        jobs.clear();
        for (Cand &c : cs) {
            if (c.numProjMatches < th.nProjMatches || c.numOptMatches < th.nSim3Inliers) continue;
            const G2oSim3T gSmw(c.pKFi->GetRotation().template cast<double>(), c.pKFi->GetTranslation().template cast<double>(), 1.0);                    // :731-733
            c.gScw = c.gScm * gSmw;
            jobs.push_back(Job{pCurrentKF, toSophus(c.gScw), &c.vpMapPoints, nullptr, 5, 1.0f, &c.vpMatchedMP2, nullptr, &c.numProjOptMatches});
        }
        if (SearchByProjectionResident(graph, jobs) < 0) return -1;                                    // (5) :738
        std::vector<CovisibleCheckCandidate<KeyFrameT, MapPointT, G2oSim3T>> covis;
        std::vector<Cand *> reached;
        for (Cand &c : cs)
            if (c.numProjMatches >= th.nProjMatches && c.numOptMatches >= th.nSim3Inliers && c.numProjOptMatches >= th.nProjOptMatches) {
                covis.push_back(CovisibleCheckCandidate<KeyFrameT, MapPointT, G2oSim3T>{c.pKFi, c.gScw, &c.vpMapPoints, &c.nNumKFs, 0});
                reached.push_back(&c);
            }
        const std::vector<KeyFrameT *> vpCurrentCovKFs = pCurrentKF->GetBestCovisibilityKeyFrames(th.nNumCovisibles);                                   // :773
        if (CovisibleCheckResident(graph, pCurrentKF, covis, vpCurrentCovKFs, toSophus) < 0) return -1;                                                // (6) :775-795
        int nBestMatchesReproj = 0, nBestNumCoindicendes = 0;                                          // (7) :802-810
        Cand *best = nullptr;
        for (Cand *c : reached)
            if (nBestMatchesReproj < c->numProjOptMatches) { nBestMatchesReproj = c->numProjOptMatches; nBestNumCoindicendes = c->nNumKFs; best = c; }
        if (nBestMatchesReproj > 0) {                                                                  // :824-841
            pLastCurrentKF = pCurrentKF;
            nNumCoincidences = nBestNumCoindicendes;
            pMatchedKF2 = best->pKFi;
            set_not_erase(pMatchedKF2, 0);
            g2oScw = best->gScw;
            vpMPs = best->vpMapPoints;
            vpMatchedMPs = best->vpMatchedMP2;
            return nNumCoincidences >= 3 ? 1 : 0;
        }
        return 0;
    }

protected:
    // pKF->SetNotErase() where the data model has the member (the reference's KeyFrame does), else its flag
    template <class K> static auto set_not_erase(K *k, int) -> decltype(k->SetNotErase(), void()) { k->SetNotErase(); }
    template <class K> static void set_not_erase(K *k, long) { k->mbNotErase = true; }

    template <class Sim3T, class GraphT, class KeyFrameT, class MapPointT>
    int saf_dispatch(GraphT &graph, const std::vector<KeyFrameT *> &vConectedKFs, std::vector<MapPointT *> &vpMapPoints, int *nSearchedAgain, std::true_type) {
        std::vector<std::pair<KeyFrameT *, Sim3T>> poses;
        for (KeyFrameT *pKF : vConectedKFs) {
            const Sophus::SE3f Tcw = pKF->GetPose();
            Sim3T Scw(Tcw.unit_quaternion(), Tcw.translation());
            Scw.setScale(1.f);
            poses.emplace_back(pKF, Scw);
        }
        return saf_dispatch<Sim3T>(graph, poses, vpMapPoints, nSearchedAgain, std::false_type());
    }

    template <class Sim3T, class GraphT, class PosesT, class MapPointT>
    int saf_dispatch(GraphT &graph, const PosesT &poses, std::vector<MapPointT *> &vpMapPoints, int *nSearchedAgain, std::false_type) {
        using KeyFrameT = typename std::remove_pointer<typename std::decay<decltype(poses.begin()->first)>::type>::type;
        static const char *where = "LoopClosingStep::SearchAndFuseResident";
        if (nSearchedAgain) *nSearchedAgain = 0;
        if (!graph.ok()) { rumi_facade::report(where, RUMI_E_INVALID, "no store; nothing was fused"); return -1; }
        // ---- 1. what can refuse, before anything is touched
        std::vector<KeyFrameT *> vpKFs;
        std::vector<int32_t> slots;
        std::vector<RumiFuseKF> rec;
        for (const auto &kv : poses) {
            KeyFrameT *pKF = kv.first;
            if (pKF->NLeft != -1) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame with NLeft != -1: only the monocular Fuse is built; nothing was fused");
                return -1;
            }
            if (graph.SlotOf(pKF) < 0 || !graph.HasFeatures(pKF)) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame the graph has never seen or without resident features (graph.Sync, graph.SyncFeatures); nothing was uploaded, nothing was fused");
                return -1;
            }
            auto Scw = kv.second;                                                   // ORBmatcher.cc:1190-1191, as Fuse (ORBmatcher.h) forms them
            const Sophus::SE3f Tcw = Sophus::SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale());
            const Eigen::Vector3f Ow = Tcw.inverse().translation();
            const auto q = Tcw.unit_quaternion();
            RumiFuseKF r;
            r.Tcw7[0] = q.x(); r.Tcw7[1] = q.y(); r.Tcw7[2] = q.z(); r.Tcw7[3] = q.w();
            for (int c = 0; c < 3; c++) { r.Tcw7[4 + c] = Tcw.translation()(c); r.Ow[c] = Ow(c); }
            r.bounds[0] = pKF->mnMinX; r.bounds[1] = pKF->mnMinY; r.bounds[2] = pKF->mnMaxX; r.bounds[3] = pKF->mnMaxY;
            r.log_scale_factor = pKF->mfLogScaleFactor;
            vpKFs.push_back(pKF); slots.push_back(graph.SlotOf(pKF)); rec.push_back(r);
        }
        const int nK = (int)vpKFs.size(), nP = (int)vpMapPoints.size();
        if (nK > RUMI_FUSE_MAX_TARGETS) { rumi_facade::report(where, RUMI_E_INVALID, "more key-frames than RUMI_FUSE_MAX_TARGETS; nothing was fused"); return -1; }
        std::vector<int32_t> ids((size_t)nP + 1, -1);
        for (int i = 0; i < nP; i++) {
            MapPointT *pMP = vpMapPoints[i];
            if (!pMP) continue;
            if (!graph.HasPoint(pMP)) {
                rumi_facade::report(where, RUMI_E_INVALID, "a loop point the graph has never seen (graph.Sync, graph.SyncAttributes); nothing was uploaded, nothing was fused");
                return -1;
            }
            ids[i] = graph.IdOf(pMP);
        }
        if (nK == 0 || nP == 0) return 0;
        // ---- 2. one call
        if (graph.FlushDirty() != RUMI_OK) return -1;
        const float th = 4.0f;                                                      // :2012, :2049
        std::vector<RumiFuseHit> hits((size_t)(nP > 1024 ? nP : 1024));
        std::vector<int32_t> per(nK);
        int32_t nHits = 0;
        if (!arena()) return -1;                                                    // reported by arena()
        auto grow = [&]() {                                                         // a hit list that was too short is not the arena's fault
            if ((size_t)nHits > hits.size()) { hits.resize((size_t)nHits); return true; }
            return ORBmatcher::grow_arena();
        };
        if (RUMI_GUARDED("LoopClosingStep / rumi_search_and_fuse_resident", grow,
                         rumi_search_and_fuse_resident(arena(), graph.handle(), slots.data(), rec.data(), nK, ids.data(), nP, th, hits.data(), (int32_t)hits.size(),
                                                       &nHits, per.data())) != RUMI_OK)
            return -1;
        // ---- 3. the replay of :2003-2026
        std::set<KeyFrameT *> touchedKFs;
        std::set<MapPointT *> touchedPts, changed;
        auto stage = [&]() {
            for (KeyFrameT *k : touchedKFs) graph.Sync(k);
            for (MapPointT *p : touchedPts) graph.Sync(p);
            for (MapPointT *p : changed) graph.MarkDirty(p);
        };
        int nFused = 0;
        size_t h0 = 0;
        for (int kk = 0; kk < nK; kk++) {
            KeyFrameT *pKF = vpKFs[kk];
            std::vector<int32_t> best((size_t)nP, -1);
            for (size_t h = h0; h < h0 + (size_t)per[kk]; h++) best[hits[h].point] = hits[h].feature;
            h0 += (size_t)per[kk];
            const auto spAlreadyFound = pKF->GetMapPoints();                        // ORBmatcher.cc:1194, at the key-frame's turn
            if (!changed.empty()) {                                                 // loop points whose descriptor a Replace changed: their answers are stale
                std::vector<int> at;
                std::vector<MapPointT *> again;
                for (int i = 0; i < nP; i++) {
                    MapPointT *p = vpMapPoints[i];
                    if (p && changed.count(p) && !p->isBad() && !spAlreadyFound.count(p)) { at.push_back(i); again.push_back(p); }
                }
                if (!again.empty()) {
                    std::vector<int32_t> sub;
                    if (!fuse_search(pKF, rec[kk].Tcw7, rec[kk].Ow, again, [](MapPointT *) { return false; }, th, 0, sub)) { stage(); return -1; }
                    for (size_t j = 0; j < at.size(); j++) best[at[j]] = sub[j];
                    if (nSearchedAgain) *nSearchedAgain += (int)at.size();
                }
            }
            std::vector<MapPointT *> vpReplacePoints((size_t)nP, static_cast<MapPointT *>(nullptr));
            for (int iMP = 0; iMP < nP; iMP++) {                                    // ORBmatcher.cc:1201-1288
                MapPointT *pMP = vpMapPoints[iMP];
                if (!pMP) continue;
                if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
                if (best[iMP] < 0) continue;
                MapPointT *pMPinKF = pKF->GetMapPoint(best[iMP]);
                if (pMPinKF) {
                    if (!pMPinKF->isBad()) vpReplacePoints[iMP] = pMPinKF;
                } else {
                    pMP->AddObservation(pKF, best[iMP]);
                    pKF->AddMapPoint(pMP, best[iMP]);
                    touchedKFs.insert(pKF); touchedPts.insert(pMP);
                }
                nFused++;
            }
            std::unique_lock<std::mutex> lock(pKF->GetMap()->mMutexMapUpdate);      // LoopClosing.cc:2015-2023
            for (int i = 0; i < nP; i++) {
                MapPointT *pRep = vpReplacePoints[i];
                if (!pRep) continue;
                MapPointT *stays = vpMapPoints[i];
                for (const auto &o : pRep->GetObservations()) touchedKFs.insert(o.first);
                const cv::Mat before = stays->GetDescriptor().clone();
                pRep->Replace(stays);
                const cv::Mat after = stays->GetDescriptor();
                if (std::memcmp(before.ptr(0), after.ptr(0), 32) != 0) changed.insert(stays);
                touchedPts.insert(pRep); touchedPts.insert(stays);
            }
        }
        stage();
        return nFused;
    }
};

}  // namespace RUMI_FACADE_NAMESPACE

namespace rumi { using LoopClosingStep = RUMI_FACADE_NAMESPACE::LoopClosingStep; }
#endif  // RUMI_HAVE_SOPHUS
