// LocalMapping::CreateNewMapPoints (R/lib_src/LocalMapping.cc:354-647, monocular pinhole) over the MI355X C ABI (include/rumi_mapping.h).
// A member template over the data-model types, like the rest of facade/: it compiles against the reference's KeyFrame / MapPoint / Atlas (the
// member names used are theirs) and against the mock types of tests/cpp.  Everything here is marshalling and the replay of the map mutations:
// one C call searches, triangulates and gates every neighbour; the points come back in the order the reference creates them.
//
// In LocalMapping.cc the body of CreateNewMapPoints from `float th = 0.6f;` (:373) to its end becomes
//     rumi::LocalMappingStep step;                                   // = ORBmatcher matcher(0.6f, false)
//     step.CreateNewMapPoints<MapPoint>(mpCurrentKeyFrame, vpNeighKFs, mpAtlas, mlpRecentAddedMapPoints, mbFarPoints, mThFarPoints,
//                                       [this] { return CheckNewKeyFrames(); }, bCoarse);
// (the neighbour list, its inertial extension :362-371 and bCoarse :423 stay the caller's).
//
// LocalMapping::KeyFrameCulling (:953-1079) and CloudKeyFrameCulling (:820-951) become
//     step.KeyFrameCulling(mpCurrentKeyFrame, mbInertial, mbMonocular, mbAbortBA);
//     step.CloudKeyFrameCulling(mpCurrentKeyFrame, mbInertial, mbMonocular, mbAbortBA);
// one device call judges the whole covisible list (rumi_keyframe_culling); SetBadFlag() is then applied in the returned order.
//
// LocalMapping::SearchInNeighbors (:649-743), with a CovisibilityGraph that holds the map, becomes
//     step.SearchInNeighborsResident<MapPoint>(graph, mpCurrentKeyFrame, mbMonocular, mbInertial, mbAbortBA);
// one device call answers every search of both passes (rumi_search_in_neighbors_resident); the reference's own objects replay the mutations.
// With a CovisibilityGraph that holds the map, step.KeyFrameCullingResident(graph, ...) / CloudKeyFrameCullingResident(graph, ...) send the
// candidates' slots instead of the neighbourhood's tables (rumi_keyframe_culling_resident).
#pragma once
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "MapPointRefresh.h"
#include "ORBmatcher.h"
#include "rumi_mapping.h"

namespace RUMI_FACADE_NAMESPACE {

class LocalMappingStep : public ORBmatcher {
public:
    // LocalMapping.cc:373-375: `ORBmatcher matcher(th = 0.6f, false)`
    explicit LocalMappingStep(bool checkOri = false) : ORBmatcher(0.6f, checkOri) {}

#ifdef RUMI_HAVE_SOPHUS
    // MapPointT is the type the reference constructs (`new MapPoint(x3D, mpCurrentKeyFrame, mpAtlas->GetCurrentMap())`, :629).
    // CheckNewKeyFrames is asked before every neighbour but the first (:398-399); when it answers true the points of the neighbours so far
    // stay and the rest are dropped, which is what the reference's early return leaves (the results of the first i neighbours do not depend
    // on later ones).  Returns the number of points created, -1 when the device call failed (reported through rumi_status.h).
    // deferRefresh: when not NULL, the two per-point members (:639-641) are not called here; the created points are appended to it and the
    // caller refreshes them in one batch (rumi_facade::RefreshMapPoints, MapPointRefresh.h) -- same results, as neither member reads
    // another point.  NULL, the default, keeps the per-point calls.
    template <class MapPointT, class KeyFrameT, class AtlasT, class RecentListT, class CheckFn>
    int CreateNewMapPoints(KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpNeighKFs, AtlasT *pAtlas, RecentListT &mlpRecentAddedMapPoints,
                           bool bFarPoints, float thFarPoints, CheckFn CheckNewKeyFrames, bool bCoarse = false,
                           std::vector<MapPointT *> *deferRefresh = nullptr) {
        const int nn = (int)vpNeighKFs.size();
        if (nn == 0) return 0;
        if (nn > RUMI_NEWPTS_MAX_NEIGH) {
            rumi_facade::report("LocalMappingStep::CreateNewMapPoints", RUMI_E_INVALID, "more neighbours than RUMI_NEWPTS_MAX_NEIGH; no point was created");
            return -1;
        }
        for (KeyFrameT *pKF : vpNeighKFs)
            if (has_stereo(pKF) || has_stereo(pCurrentKF)) {   // stereo / two-camera branches (:446-504, 518-545, 576-607) are not built: say so, do not run them as mono
                rumi_facade::report("LocalMappingStep::CreateNewMapPoints", RUMI_E_INVALID, "a key-frame has stereo key-points (mvuRight >= 0): only the monocular branch is built; no point was created");
                return -1;
            }
        std::vector<Marshalled> hold(nn + 1);
        std::vector<RumiNewPointsKF> kf(nn + 1);
        marshal(pCurrentKF, false, hold[0], kf[0]);
        const Sophus::SE3f T1w = pCurrentKF->GetPose();
        const Eigen::Vector3f Cw = pCurrentKF->GetCameraCenter();
        const Eigen::Matrix3f K1 = pCurrentKF->mpCamera->toK_();
        for (int k = 0; k < nn; k++) {
            KeyFrameT *pKF2 = vpNeighKFs[k];
            marshal(pKF2, true, hold[1 + k], kf[1 + k]);
            // the epipole and F12 with the reference's own expressions, as SearchForTriangulation above forms them (ORBmatcher.cc:815-818,
            // GeometricTools::ComputeF12 / Pinhole::epipolarConstrain)
            const Sophus::SE3f T2w = pKF2->GetPose(), Tw2 = pKF2->GetPoseInverse();
            const Eigen::Vector3f C2 = T2w * Cw;
            const Eigen::Vector2f ep = pKF2->mpCamera->project(C2);
            const Sophus::SE3f T12 = T1w * Tw2;
            const Eigen::Matrix3f R12 = T12.rotationMatrix();
            const Eigen::Vector3f t12 = T12.translation();
            const Eigen::Matrix3f t12x = Sophus::SO3f::hat(t12);
            const Eigen::Matrix3f K2 = pKF2->mpCamera->toK_();
            const Eigen::Matrix3f F12 = K1.transpose().inverse() * t12x * R12 * K2.inverse();
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) kf[1 + k].F12[r * 3 + c] = F12(r, c);
            kf[1 + k].epipole2[0] = ep(0); kf[1 + k].epipole2[1] = ep(1);
        }
        RumiNewPointsParams prm;
        prm.coarse = bCoarse; prm.check_orientation = mbCheckOrientation; prm.far_points = bFarPoints; prm.th_far_points = thFarPoints;
        prm.ratio_factor = 1.5f * pCurrentKF->mfScaleFactor;                    // :391
        std::vector<RumiNewPoint> pts((size_t)(pCurrentKF->N > 0 ? pCurrentKF->N : 1));
        std::vector<int32_t> per(nn);
        std::vector<uint8_t> skipped(nn);
        int32_t nOut = 0;
        if (RUMI_GUARDED("LocalMappingStep / rumi_create_new_map_points", &ORBmatcher::grow_arena,
                         rumi_create_new_map_points(arena(), &kf[0], &kf[1], nn, &prm, pts.data(), (int32_t)pts.size(), &nOut, per.data(),
                                                    skipped.data())) != RUMI_OK)
            return -1;
        return replay<MapPointT>(pCurrentKF, vpNeighKFs, pAtlas, mlpRecentAddedMapPoints, CheckNewKeyFrames, pts, per, deferRefresh, nullptr);
    }

    // The same member over key-frames resident in a CovisibilityGraph (CovisibilityGraph.h): every key-frame's features were staged once by
    // graph.SyncFeatures, its map-point row and the points' positions are what graph.Sync / MarkDirty keep current, so only the poses travel
    // (rumi_create_new_map_points_resident).  FlushDirty() runs first.  A key-frame without resident features is refused with a report -- it
    // is not uploaded behind the caller's back.  The host replay is CreateNewMapPoints'; afterwards the touched key-frames and the created
    // points are staged again (Sync, MarkDirty), so the graph is current when the member returns.  `created`: as deferRefresh above.
    template <class MapPointT, class GraphT, class KeyFrameT, class AtlasT, class RecentListT, class CheckFn>
    int CreateNewMapPointsResident(GraphT &graph, KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpNeighKFs, AtlasT *pAtlas,
                                   RecentListT &mlpRecentAddedMapPoints, bool bFarPoints, float thFarPoints, CheckFn CheckNewKeyFrames,
                                   bool bCoarse = false, std::vector<MapPointT *> *created = nullptr) {
        static const char *where = "LocalMappingStep::CreateNewMapPointsResident";
        const int nn = (int)vpNeighKFs.size();
        if (nn == 0) return 0;
        if (nn > RUMI_NEWPTS_MAX_NEIGH) {
            rumi_facade::report(where, RUMI_E_INVALID, "more neighbours than RUMI_NEWPTS_MAX_NEIGH; no point was created");
            return -1;
        }
        if (!graph.ok()) { rumi_facade::report(where, RUMI_E_INVALID, "no store; no point was created"); return -1; }
        std::vector<int32_t> slots(nn);
        for (int k = -1; k < nn; k++) {
            KeyFrameT *pKF = k < 0 ? pCurrentKF : vpNeighKFs[k];
            if (has_stereo(pKF)) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame has stereo key-points (mvuRight >= 0): only the monocular branch is built; no point was created");
                return -1;
            }
            if (!graph.HasFeatures(pKF)) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame without resident features (CovisibilityGraph::SyncFeatures was never called for it); no point was created");
                return -1;
            }
            if (k >= 0) slots[k] = graph.SlotOf(pKF);
        }
        if (graph.FlushDirty() != RUMI_OK) return -1;
        std::vector<RumiNewPointsPose> pose(nn + 1);
        pose_of(pCurrentKF, pose[0]);
        const Sophus::SE3f T1w = pCurrentKF->GetPose();
        const Eigen::Vector3f Cw = pCurrentKF->GetCameraCenter();
        const Eigen::Matrix3f K1 = pCurrentKF->mpCamera->toK_();
        for (int k = 0; k < nn; k++) {                                          // F12 and the epipole: the expressions of CreateNewMapPoints above
            KeyFrameT *pKF2 = vpNeighKFs[k];
            pose_of(pKF2, pose[1 + k]);
            const Sophus::SE3f T2w = pKF2->GetPose(), Tw2 = pKF2->GetPoseInverse();
            const Eigen::Vector3f C2 = T2w * Cw;
            const Eigen::Vector2f ep = pKF2->mpCamera->project(C2);
            const Sophus::SE3f T12 = T1w * Tw2;
            const Eigen::Matrix3f R12 = T12.rotationMatrix();
            const Eigen::Vector3f t12 = T12.translation();
            const Eigen::Matrix3f t12x = Sophus::SO3f::hat(t12);
            const Eigen::Matrix3f K2 = pKF2->mpCamera->toK_();
            const Eigen::Matrix3f F12 = K1.transpose().inverse() * t12x * R12 * K2.inverse();
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) pose[1 + k].F12[r * 3 + c] = F12(r, c);
            pose[1 + k].epipole2[0] = ep(0); pose[1 + k].epipole2[1] = ep(1);
        }
        RumiNewPointsParams prm;
        prm.coarse = bCoarse; prm.check_orientation = mbCheckOrientation; prm.far_points = bFarPoints; prm.th_far_points = thFarPoints;
        prm.ratio_factor = 1.5f * pCurrentKF->mfScaleFactor;                    // :391
        std::vector<RumiNewPoint> pts((size_t)(pCurrentKF->N > 0 ? pCurrentKF->N : 1));
        std::vector<int32_t> per(nn);
        std::vector<uint8_t> skipped(nn);
        int32_t nOut = 0;
        if (RUMI_GUARDED("LocalMappingStep / rumi_create_new_map_points_resident", &ORBmatcher::grow_arena,
                         rumi_create_new_map_points_resident(arena(), graph.handle(), graph.SlotOf(pCurrentKF), &pose[0], slots.data(), &pose[1], nn, &prm,
                                                             pts.data(), (int32_t)pts.size(), &nOut, per.data(), skipped.data())) != RUMI_OK)
            return -1;
        std::vector<MapPointT *> made;
        const int n = replay<MapPointT>(pCurrentKF, vpNeighKFs, pAtlas, mlpRecentAddedMapPoints, CheckNewKeyFrames, pts, per, created, &made);
        if (!made.empty()) {                                                    // rows of the touched key-frames, observers and attributes of the new points
            std::vector<KeyFrameT *> touched{pCurrentKF};
            for (MapPointT *p : made) graph.MarkDirty(p);
            for (int i = 0, next = 0; i < nn && next < (int)made.size(); next += per[i++])
                if (per[i] > 0) touched.push_back(vpNeighKFs[i]);
            for (KeyFrameT *k : touched)
                if (graph.Sync(k) != RUMI_OK) break;
        }
        return n;
    }

    // LocalMapping::SearchInNeighbors (R/lib_src/LocalMapping.cc:649-743), monocular and non-inertial, over a CovisibilityGraph that holds
    // the map.  The target list is built as :651-677 builds it (stamps, isBad skips, the mbAbortBA break); FlushDirty(); ONE device call
    // answers every search of the forward and of the reverse pass from the store as it stands (rumi_search_in_neighbors_resident); then the
    // reference's own objects replay both passes in order, every gate re-evaluated at its turn, as Fuse above does for one target.
    // MapPoint::Replace ends with ComputeDistinctiveDescriptors() on the survivor (MapPoint.cc:321): a point of the current key-frame whose
    // GetDescriptor() a Replace changed is searched again, on its live descriptor, for every target that follows (one small
    // rumi_fuse_candidates call per such target; *nSearchedAgain counts the pairs).  A reverse candidate that is not bad, not in the current
    // key-frame and missing from the call's table contradicts the store: reported (RUMI_E_INVALID, counted) and skipped, never searched on
    // the host.  Then RefreshKeyFramePoints (:730-739) and graph.UpdateConnections({current}) (:742).  The touched key-frames and points are
    // staged again (Sync, MarkDirty), so the graph is current when the member returns.
    // Returns the two passes' nFused together, or -1 with a report and nothing mutated: mbInertial (the temporal extension :680-691),
    // NLeft != -1 on any key-frame, a key-frame the graph has never seen or without SyncFeatures, more targets than RUMI_FUSE_MAX_TARGETS,
    // a failed device call.  The caller keeps the reference's member for those.
    template <class MapPointT, class GraphT, class KeyFrameT>
    int SearchInNeighborsResident(GraphT &graph, KeyFrameT *pCurrentKF, bool bMonocular, bool bInertial, const volatile bool &bAbortBA,
                                  int *nSearchedAgain = nullptr, int *nContradictions = nullptr) {
        static const char *where = "LocalMappingStep::SearchInNeighborsResident";
        if (nSearchedAgain) *nSearchedAgain = 0;
        if (nContradictions) *nContradictions = 0;
        if (bInertial) {
            rumi_facade::report(where, RUMI_E_INVALID, "mbInertial: the temporal extension (LocalMapping.cc:680-691) is not built; nothing was fused");
            return -1;
        }
        if (!graph.ok()) { rumi_facade::report(where, RUMI_E_INVALID, "no store; nothing was fused"); return -1; }
        // ---- 1. the targets (:651-677).  The stamps are written once nothing can refuse any more; until then `in` stands for them.
        std::vector<KeyFrameT *> vpTargetKFs;
        std::set<KeyFrameT *> in;
        auto taken = [&](KeyFrameT *k) { return k->isBad() || k->mnFuseTargetForKF == pCurrentKF->mnId || in.count(k) > 0; };
        for (KeyFrameT *pKFi : pCurrentKF->GetBestCovisibilityKeyFrames(bMonocular ? 30 : 10)) {
            if (taken(pKFi)) continue;
            vpTargetKFs.push_back(pKFi); in.insert(pKFi);
        }
        for (int i = 0, imax = (int)vpTargetKFs.size(); i < imax; i++) {
            for (KeyFrameT *pKFi2 : vpTargetKFs[i]->GetBestCovisibilityKeyFrames(20)) {
                if (taken(pKFi2) || pKFi2->mnId == pCurrentKF->mnId) continue;
                vpTargetKFs.push_back(pKFi2); in.insert(pKFi2);
            }
            if (bAbortBA) break;
        }
        const int nT = (int)vpTargetKFs.size();
        if (nT > RUMI_FUSE_MAX_TARGETS) { rumi_facade::report(where, RUMI_E_INVALID, "more targets than RUMI_FUSE_MAX_TARGETS; nothing was fused"); return -1; }
        std::vector<int32_t> slots(nT > 0 ? nT : 1);
        for (int k = -1; k < nT; k++) {
            KeyFrameT *pKF = k < 0 ? pCurrentKF : vpTargetKFs[k];
            if (pKF->NLeft != -1) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame with NLeft != -1: only the monocular Fuse is built; nothing was fused");
                return -1;
            }
            if (graph.SlotOf(pKF) < 0 || !graph.HasFeatures(pKF)) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame the graph has never seen or without resident features (graph.Sync, graph.SyncFeatures); nothing was uploaded, nothing was fused");
                return -1;
            }
            if (k >= 0) slots[k] = graph.SlotOf(pKF);
        }
        // ---- 2., 3. one call
        if (graph.FlushDirty() != RUMI_OK) return -1;
        std::vector<RumiFuseKF> rec(nT + 1);
        size_t revCap = 0;
        for (int k = 0; k <= nT; k++) {
            KeyFrameT *pKF = k ? vpTargetKFs[k - 1] : pCurrentKF;
            fuse_pose(pKF, rec[k].Tcw7, rec[k].Ow);
            rec[k].bounds[0] = pKF->mnMinX; rec[k].bounds[1] = pKF->mnMinY; rec[k].bounds[2] = pKF->mnMaxX; rec[k].bounds[3] = pKF->mnMaxY;
            rec[k].log_scale_factor = pKF->mfLogScaleFactor;
            if (k) revCap += (size_t)pKF->N;
        }
        const int nCur = pCurrentKF->N;
        const float th = 3.0f;                                                  // Fuse's default, as :699 and :726 call it
        std::vector<int32_t> fwd((size_t)nT * nCur + 1), revPoint(revCap + 1), revBest(revCap + 1);
        int32_t nRev = 0;
        if (RUMI_GUARDED("LocalMappingStep / rumi_search_in_neighbors_resident", &ORBmatcher::grow_arena,
                         rumi_search_in_neighbors_resident(arena(), graph.handle(), graph.SlotOf(pCurrentKF), &rec[0], slots.data(), rec.data() + 1, nT, th,
                                                           fwd.data(), revPoint.data(), revBest.data(), (int32_t)revCap, &nRev)) != RUMI_OK)
            return -1;
        for (KeyFrameT *pKFi : vpTargetKFs) pKFi->mnFuseTargetForKF = pCurrentKF->mnId;
        // ---- 4. the forward pass (:694-701)
        FuseTouched<KeyFrameT, MapPointT> touched;
        const std::vector<MapPointT *> vpMapPointMatches = pCurrentKF->GetMapPointMatches();   // copied once (:695)
        int nFused = 0;
        bool failed = false;
        for (int t = 0; t < nT && !failed; t++) {
            KeyFrameT *pKFi = vpTargetKFs[t];
            std::vector<int32_t> best(fwd.begin() + (size_t)t * nCur, fwd.begin() + (size_t)(t + 1) * nCur);
            if (!touched.changed.empty()) {                                     // survivors whose descriptor a Replace changed: their answers are stale
                std::vector<int> at;
                std::vector<MapPointT *> again;
                for (int i = 0; i < nCur && i < (int)vpMapPointMatches.size(); i++) {
                    MapPointT *p = vpMapPointMatches[i];
                    if (p && touched.changed.count(p) && !p->isBad() && !p->IsInKeyFrame(pKFi)) { at.push_back(i); again.push_back(p); }
                }
                if (!again.empty()) {
                    float T7[7], Ow[3];
                    fuse_pose(pKFi, T7, Ow);
                    std::vector<int32_t> sub;
                    if (!fuse_search(pKFi, T7, Ow, again, [](MapPointT *) { return false; }, th, 1, sub)) { failed = true; break; }
                    for (size_t j = 0; j < at.size(); j++) best[at[j]] = sub[j];
                    if (nSearchedAgain) *nSearchedAgain += (int)at.size();
                }
            }
            nFused += fuse_replay(pKFi, vpMapPointMatches, best, touched);
        }
        // ---- 5. (:703), and a second search that failed: what was replayed stays, as it does when the reference returns here
        if (failed || bAbortBA) { touched.stage(graph); return failed ? -1 : nFused; }
        // ---- 6. the reverse candidates (:706-724), on the map as the forward pass left it
        std::vector<MapPointT *> vpFuseCandidates;
        for (KeyFrameT *pKFi : vpTargetKFs)
            for (MapPointT *pMP : pKFi->GetMapPointMatches()) {
                if (!pMP) continue;
                if (pMP->isBad() || pMP->mnFuseCandidateForKF == pCurrentKF->mnId) continue;
                pMP->mnFuseCandidateForKF = pCurrentKF->mnId;
                vpFuseCandidates.push_back(pMP);
            }
        // ---- 7. the reverse pass (:726) from the call's table
        std::unordered_map<int32_t, int32_t> table;
        for (int j = 0; j < nRev; j++) table[revPoint[j]] = revBest[j];
        std::vector<int32_t> best(vpFuseCandidates.size(), -1);
        int contradictions = 0;
        for (size_t i = 0; i < vpFuseCandidates.size(); i++) {
            MapPointT *pMP = vpFuseCandidates[i];
            if (pMP->isBad() || pMP->IsInKeyFrame(pCurrentKF)) continue;        // Fuse skips it whatever the table says
            auto it = table.find(graph.IdOf(pMP));
            if (it != table.end()) best[i] = it->second;
            else contradictions++;                                              // not searched at the call: skipped, not searched here
        }
        if (contradictions) {
            rumi_facade::report(where, RUMI_E_INVALID, "reverse candidates that the store did not hold in a target row at the call (graph.Sync missing somewhere); they were skipped");
            if (nContradictions) *nContradictions = contradictions;
        }
        nFused += fuse_replay(pCurrentKF, vpFuseCandidates, best, touched);
        // ---- 8. Update points (:730-739)
        rumi_facade::RefreshKeyFramePoints(pCurrentKF);
        for (MapPointT *pMP : pCurrentKF->GetMapPointMatches())
            if (pMP && !pMP->isBad()) graph.MarkDirty(pMP);
        // ---- 9. (:742)
        touched.stage(graph);
        graph.UpdateConnections(std::vector<KeyFrameT *>{pCurrentKF}, false);
        return nFused;
    }
#endif  // RUMI_HAVE_SOPHUS

    // The reference's loop over GetVectorCovisibleKeyFrames() after UpdateBestCovisibles(), non-inertial and monocular.  mbAbortBA is read once,
    // here (the reference reads it at every candidate).  Returns the number of key-frames culled (SetBadFlag() went through), -1 when no
    // key-frame or point was touched: mbInertial or !mbMonocular (the inertial branch :1045-1070 and the stereo depth gate :1001-1004 are not
    // built; refused before anything is called), a stereo observation or key-frame (NLeft != -1), or the device call failed -- all reported
    // through rumi_status.h.  The last two are found while the covisible list is read, so UpdateBestCovisibles() (:959) has run by then, as it
    // has at the top of the reference's member the caller falls back to.
    // KeyFrame needs one getter the reference lacks: bool GetNotErase() { return mbNotErase; }.
    template <class KeyFrameT> int KeyFrameCulling(KeyFrameT *pCurrentKF, bool bInertial, bool bMonocular, bool bAbortBA) {
        return culling(pCurrentKF, bInertial, bMonocular, bAbortBA, false);
    }
    template <class KeyFrameT> int CloudKeyFrameCulling(KeyFrameT *pCurrentKF, bool bInertial, bool bMonocular, bool bAbortBA) {
        return culling(pCurrentKF, bInertial, bMonocular, bAbortBA, true);
    }

    // The same two members over a CovisibilityGraph (CovisibilityGraph.h) that holds the map: the candidates travel as slots with their three
    // flags, everything else is read where it lies on the device (rumi_keyframe_culling_resident).  The graph must be current: graph.Sync of
    // the key-frames and points the mutators touched, graph.SyncFeatures of every key-frame that observes a point of a candidate.  SetBadFlag()
    // is applied in the returned order; its Sync hooks stage the edits for the next query.  Refuses what the members above
    // refuse, and a candidate the graph has never seen: nothing is staged or uploaded on the caller's behalf.  Returns as above.
    template <class GraphT, class KeyFrameT> int KeyFrameCullingResident(GraphT &graph, KeyFrameT *pCurrentKF, bool bInertial, bool bMonocular, bool bAbortBA) {
        return culling_resident(graph, pCurrentKF, bInertial, bMonocular, bAbortBA, false);
    }
    template <class GraphT, class KeyFrameT> int CloudKeyFrameCullingResident(GraphT &graph, KeyFrameT *pCurrentKF, bool bInertial, bool bMonocular, bool bAbortBA) {
        return culling_resident(graph, pCurrentKF, bInertial, bMonocular, bAbortBA, true);
    }

protected:
#ifdef RUMI_HAVE_SOPHUS
    // What the replay of Fuse changed: key-frames whose rows and points whose observers or bad flag the store must see again, and the
    // survivors of a Replace whose descriptor it changed.
    template <class KeyFrameT, class MapPointT> struct FuseTouched {
        std::set<KeyFrameT *> kfs;
        std::set<MapPointT *> pts, changed;
        template <class GraphT> void stage(GraphT &graph) {
            for (KeyFrameT *k : kfs) graph.Sync(k);
            for (MapPointT *p : pts) graph.Sync(p);
            for (MapPointT *p : changed) graph.MarkDirty(p);
            kfs.clear(); pts.clear();
        }
    };

    template <class KeyFrameT> static void fuse_pose(KeyFrameT *pKF, float *T7, float *Ow) {      // as Fuse (ORBmatcher.h) forms them
        const auto Tcw = pKF->GetPose();
        const auto q = Tcw.unit_quaternion();
        const auto t = Tcw.translation();
        T7[0] = q.x(); T7[1] = q.y(); T7[2] = q.z(); T7[3] = q.w(); T7[4] = t(0); T7[5] = t(1); T7[6] = t(2);
        const Eigen::Vector3f c = pKF->GetCameraCenter();
        Ow[0] = c(0); Ow[1] = c(1); Ow[2] = c(2);
    }

    // ORBmatcher.cc:1045-1056 and :1162-1174 over `pts` with the search's answers in `best`: the loop of Fuse (ORBmatcher.h), which also notes
    // what it touched and compares the survivor's descriptor around every Replace.
    template <class KeyFrameT, class MapPointT>
    static int fuse_replay(KeyFrameT *pKF, const std::vector<MapPointT *> &pts, const std::vector<int32_t> &best, FuseTouched<KeyFrameT, MapPointT> &touched) {
        int nFused = 0;
        for (size_t i = 0; i < pts.size() && i < best.size(); i++) {
            MapPointT *pMP = pts[i];
            if (!pMP) continue;
            if (pMP->isBad()) continue;
            else if (pMP->IsInKeyFrame(pKF)) continue;
            if (best[i] < 0) continue;
            MapPointT *pMPinKF = pKF->GetMapPoint(best[i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    const bool keepInKF = pMPinKF->Observations() > pMP->Observations();
                    MapPointT *gone = keepInKF ? pMP : pMPinKF, *stays = keepInKF ? pMPinKF : pMP;
                    for (const auto &o : gone->GetObservations()) touched.kfs.insert(o.first);
                    const cv::Mat before = stays->GetDescriptor().clone();
                    gone->Replace(stays);
                    const cv::Mat after = stays->GetDescriptor();
                    if (std::memcmp(before.ptr(0), after.ptr(0), 32) != 0) touched.changed.insert(stays);     // (after the forward pass only MarkDirty reads it)
                    touched.pts.insert(gone); touched.pts.insert(stays);
                }
            } else {
                pMP->AddObservation(pKF, best[i]);
                pKF->AddMapPoint(pMP, best[i]);
                touched.kfs.insert(pKF); touched.pts.insert(pMP);
            }
            nFused++;
        }
        return nFused;
    }
#endif

    // One culling handle per calling thread (handles are not re-entrant), destroyed with its blocks when the thread ends.
    struct CullHandle {
        RumiCull *h = nullptr;
        CullHandle() = default;
        CullHandle(const CullHandle &) = delete;
        CullHandle &operator=(const CullHandle &) = delete;
        ~CullHandle() { rumi_cull_destroy(h); }
    };
    static RumiCull *cull_handle() {
        thread_local CullHandle holder;
        if (!holder.h) {
            const int rc = rumi_cull_create(-1, &holder.h);
            if (rc != RUMI_OK) { rumi_facade::report("LocalMappingStep::KeyFrameCulling: handle", rc); holder.h = nullptr; }
        }
        return holder.h;
    }

    template <class KeyFrameT> int culling(KeyFrameT *pCurrentKF, bool bInertial, bool bMonocular, bool bAbortBA, bool cloudVariant) {
        static const char *where = "LocalMappingStep::KeyFrameCulling";
        if (bInertial || !bMonocular) {
            rumi_facade::report(where, RUMI_E_INVALID, "mbInertial or a non-monocular sensor: only the non-inertial monocular loop is built; no key-frame was culled");
            return -1;
        }
        pCurrentKF->UpdateBestCovisibles();                                     // :959
        const auto vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();   // :960
        using KFPtr = typename std::decay<decltype(vpLocalKeyFrames)>::type::value_type;
        using MPPtr = typename std::decay<decltype(vpLocalKeyFrames[0]->GetMapPointMatches())>::type::value_type;
        std::vector<KFPtr> kfs;
        std::unordered_map<const void *, int32_t> kfIndex, mpIndex;
        std::vector<MPPtr> mps;
        auto kf_of = [&](KFPtr pKF) {
            auto it = kfIndex.find(pKF);
            if (it != kfIndex.end()) return it->second;
            kfs.push_back(pKF);
            return kfIndex[pKF] = (int32_t)kfs.size() - 1;
        };
        // the candidates, all of their points, and every key-frame those points list
        std::vector<int32_t> cand;
        for (KFPtr pKF : vpLocalKeyFrames) cand.push_back(kf_of(pKF));
        const size_t nCandKF = kfs.size();
        std::vector<std::vector<int32_t>> mp(nCandKF), octave;
        for (size_t k = 0; k < nCandKF; k++) {
            const auto vpMapPoints = kfs[k]->GetMapPointMatches();              // :991
            mp[k].assign(vpMapPoints.size(), -1);
            for (size_t i = 0; i < vpMapPoints.size(); i++) {
                MPPtr pMP = vpMapPoints[i];
                if (!pMP) continue;
                auto it = mpIndex.find(pMP);
                if (it == mpIndex.end()) { mps.push_back(pMP); it = mpIndex.emplace(pMP, (int32_t)mps.size() - 1).first; }
                mp[k][i] = it->second;
            }
        }
        std::vector<RumiCullPoint> pts(mps.size());
        std::vector<int32_t> obsKf, obsFeature;
        for (size_t p = 0; p < mps.size(); p++) {
            const auto observations = mps[p]->GetObservations();               // std::map: the order :1011 iterates in
            pts[p].obs_begin = (int32_t)obsKf.size();
            for (const auto &o : observations) {
                const int leftIndex = std::get<0>(o.second), rightIndex = std::get<1>(o.second);
                if (rightIndex != -1 || leftIndex == -1 || o.first->NLeft != -1) {
                    rumi_facade::report(where, RUMI_E_INVALID, "a stereo observation (right index or NLeft != -1): only the monocular loop is built; no key-frame was culled");
                    return -1;
                }
                const int32_t k = kf_of(o.first);
                if ((size_t)k >= mp.size()) mp.resize((size_t)k + 1);
                if (mp[k].empty()) mp[k].assign(o.first->mvKeysUn.size(), -1);
                // a key-frame outside the covisible list is never culled: of its slots only those the table's points name matter
                if ((size_t)k >= nCandKF && leftIndex < (int)mp[k].size() && o.first->GetMapPoint(leftIndex) == mps[p]) mp[k][leftIndex] = (int32_t)p;
                obsKf.push_back(k);
                obsFeature.push_back(leftIndex);
            }
            pts[p].obs_end = (int32_t)obsKf.size();
            pts[p].n_obs_count = mps[p]->Observations();
            pts[p].is_bad = mps[p]->isBad();
            pts[p].pad_[0] = pts[p].pad_[1] = pts[p].pad_[2] = 0;
        }
        mp.resize(kfs.size());
        octave.resize(kfs.size());
        std::vector<RumiCullKF> table(kfs.size());
        for (size_t k = 0; k < kfs.size(); k++) {
            KFPtr pKF = kfs[k];
            if (pKF->NLeft != -1) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame with NLeft != -1: only the monocular loop is built; no key-frame was culled");
                return -1;
            }
            mp[k].resize(pKF->mvKeysUn.size(), -1);
            octave[k].resize(pKF->mvKeysUn.size());
            for (size_t i = 0; i < octave[k].size(); i++) octave[k][i] = pKF->mvKeysUn[i].octave;   // :1008, :1019
            RumiCullKF &o = table[k];
            o.octave = octave[k].data(); o.mp = mp[k].data(); o.n = (int32_t)octave[k].size();
            o.is_bad = pKF->isBad(); o.is_init = pKF->mnId == pKF->GetMap()->GetInitKFid();
            o.not_erase = pKF->GetNotErase(); o.is_cloud = pKF->isCloud();
        }
        const int nc = (int)cand.size();
        std::vector<int32_t> status(nc), nMPs(nc), nRedundant(nc), culled(nc);
        int32_t nCulled = 0;
        RumiCull *h = cull_handle();
        if (!h) return -1;
        const int flags = (cloudVariant ? RUMI_CULL_CLOUD : 0) | (bAbortBA ? RUMI_CULL_ABORT_BA : 0);
        if (RUMI_GUARDED("LocalMappingStep / rumi_keyframe_culling", &rumi_facade::no_growth,
                         rumi_keyframe_culling(h, table.data(), (int32_t)table.size(), cand.data(), nc, pts.data(), (int32_t)pts.size(), obsKf.data(),
                                               obsFeature.data(), (int32_t)obsKf.size(), flags, status.data(), nMPs.data(), nRedundant.data(),
                                               culled.data(), &nCulled)) != RUMI_OK)
            return -1;
        for (int c = 0; c < nc; c++)                                            // :1072, in the loop's order; a not_erase key-frame only gets mbToBeErased
            if (status[c] == RUMI_CULL_CULLED || status[c] == RUMI_CULL_TO_BE_ERASED) vpLocalKeyFrames[c]->SetBadFlag();
        return nCulled;
    }

    template <class GraphT, class KeyFrameT>
    int culling_resident(GraphT &graph, KeyFrameT *pCurrentKF, bool bInertial, bool bMonocular, bool bAbortBA, bool cloudVariant) {
        static const char *where = "LocalMappingStep::KeyFrameCullingResident";
        if (bInertial || !bMonocular) {
            rumi_facade::report(where, RUMI_E_INVALID, "mbInertial or a non-monocular sensor: only the non-inertial monocular loop is built; no key-frame was culled");
            return -1;
        }
        if (!graph.ok()) { rumi_facade::report(where, RUMI_E_INVALID, "no store; no key-frame was culled"); return -1; }
        pCurrentKF->UpdateBestCovisibles();                                     // :959
        const auto vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();   // :960
        const int nc = (int)vpLocalKeyFrames.size();
        std::vector<RumiCullCandidate> cand(nc);
        for (int c = 0; c < nc; c++) {
            auto pKF = vpLocalKeyFrames[c];
            if (pKF->NLeft != -1) {
                rumi_facade::report(where, RUMI_E_INVALID, "a key-frame with NLeft != -1: only the monocular loop is built; no key-frame was culled");
                return -1;
            }
            const int slot = graph.SlotOf(pKF);
            if (slot < 0) {
                rumi_facade::report(where, RUMI_E_INVALID, "a candidate the graph has never seen (graph.Sync, graph.SyncFeatures); nothing was uploaded, no key-frame was culled");
                return -1;
            }
            cand[c].slot = slot;
            cand[c].is_init = pKF->mnId == pKF->GetMap()->GetInitKFid();
            cand[c].not_erase = pKF->GetNotErase();
            cand[c].is_cloud = pKF->isCloud();
            cand[c].pad_ = 0;
        }
        if (nc == 0) return 0;
        std::vector<int32_t> status(nc), nMPs(nc), nRedundant(nc), culled(nc);
        int32_t nCulled = 0;
        RumiCull *h = cull_handle();
        if (!h) return -1;
        const int flags = (cloudVariant ? RUMI_CULL_CLOUD : 0) | (bAbortBA ? RUMI_CULL_ABORT_BA : 0);
        if (RUMI_GUARDED("LocalMappingStep / rumi_keyframe_culling_resident", &rumi_facade::no_growth,
                         rumi_keyframe_culling_resident(h, graph.handle(), cand.data(), nc, flags, status.data(), nMPs.data(), nRedundant.data(),
                                                        culled.data(), &nCulled)) != RUMI_OK)
            return -1;
        for (int c = 0; c < nc; c++)                                            // :1072, in the loop's order; a not_erase key-frame only gets mbToBeErased
            if (status[c] == RUMI_CULL_CULLED || status[c] == RUMI_CULL_TO_BE_ERASED) vpLocalKeyFrames[c]->SetBadFlag();
        return nCulled;
    }

#ifdef RUMI_HAVE_SOPHUS
    struct Marshalled { Csr fv; std::vector<int32_t> mp; std::vector<float> pos; };

    // :628-644 for every returned point, in the returned order, neighbour by neighbour; stops where CheckNewKeyFrames answers true (:398-399).
    // made: when not NULL, every point created here.
    template <class MapPointT, class KeyFrameT, class AtlasT, class RecentListT, class CheckFn>
    static int replay(KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpNeighKFs, AtlasT *pAtlas, RecentListT &mlpRecentAddedMapPoints,
                      CheckFn &CheckNewKeyFrames, const std::vector<RumiNewPoint> &pts, const std::vector<int32_t> &per,
                      std::vector<MapPointT *> *deferRefresh, std::vector<MapPointT *> *made) {
        int created = 0, next = 0;
        for (int i = 0; i < (int)vpNeighKFs.size(); i++) {
            if (i > 0 && CheckNewKeyFrames()) return created;                   // :398-399
            KeyFrameT *pKF2 = vpNeighKFs[i];
            for (int j = 0; j < per[i]; j++, next++) {
                const RumiNewPoint &P = pts[next];
                const Eigen::Vector3f x3D(P.x3D[0], P.x3D[1], P.x3D[2]);
                MapPointT *pMP = new MapPointT(x3D, pCurrentKF, pAtlas->GetCurrentMap());
                pMP->AddObservation(pCurrentKF, P.idx1);
                pMP->AddObservation(pKF2, P.idx2);
                pCurrentKF->AddMapPoint(pMP, P.idx1);
                pKF2->AddMapPoint(pMP, P.idx2);
                if (deferRefresh) deferRefresh->push_back(pMP);
                else {
                    pMP->ComputeDistinctiveDescriptors();
                    pMP->UpdateNormalAndDepth();
                }
                pAtlas->AddMapPoint(pMP);
                mlpRecentAddedMapPoints.push_back(pMP);
                if (made) made->push_back(pMP);
                created++;
            }
        }
        return created;
    }

    template <class KeyFrameT> static void pose_of(KeyFrameT *pKF, RumiNewPointsPose &o) {
        const Sophus::SE3f Tcw = pKF->GetPose();                                // as marshal() below
        const Eigen::Matrix3f R = Tcw.rotationMatrix();
        const Eigen::Vector3f t = Tcw.translation(), Ow = pKF->GetCameraCenter();
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o.Tcw[r * 4 + c] = R(r, c); o.Tcw[r * 4 + 3] = t(r); o.Ow[r] = Ow(r); }
        for (float &f : o.F12) f = 0.f;
        o.epipole2[0] = o.epipole2[1] = 0.f;
    }

    template <class KeyFrameT> static bool has_stereo(KeyFrameT *pKF) {
        for (float u : pKF->mvuRight) if (u >= 0) return true;
        return false;
    }

    template <class KeyFrameT> static void marshal(KeyFrameT *pKF, bool neighbour, Marshalled &h, RumiNewPointsKF &o) {
        o.feat = view(*pKF);
        h.fv = csr(pKF->mFeatVec);
        o.fv = RumiFeatureVector{(int32_t)h.fv.nodes.size(), h.fv.nodes.data(), h.fv.off.data(), h.fv.idx.data()};
        const auto vp = pKF->GetMapPointMatches();
        h.mp.assign(pKF->N, -1);
        h.pos.assign(neighbour ? (size_t)pKF->N * 3 : 0, 0.f);
        for (size_t i = 0; i < vp.size() && i < h.mp.size(); i++) {
            if (!vp[i]) continue;
            h.mp[i] = 0;
            if (neighbour) {                                                    // KeyFrame::ComputeSceneMedianDepth reads GetWorldPos() of every point (KeyFrame.cc:966-973)
                const Eigen::Vector3f X = vp[i]->GetWorldPos();
                for (int c = 0; c < 3; c++) h.pos[3 * i + c] = X(c);
            }
        }
        o.kf_mp = h.mp.data();
        o.mp_pos = neighbour ? h.pos.data() : nullptr;
        o.K4[0] = pKF->fx; o.K4[1] = pKF->fy; o.K4[2] = pKF->cx; o.K4[3] = pKF->cy;
        const Sophus::SE3f Tcw = pKF->GetPose();                                // eigTcw = sophTcw.matrix3x4() = [R | t] (:377-381, 427-431)
        const Eigen::Matrix3f R = Tcw.rotationMatrix();
        const Eigen::Vector3f t = Tcw.translation(), Ow = pKF->GetCameraCenter();
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o.Tcw[r * 4 + c] = R(r, c); o.Tcw[r * 4 + 3] = t(r); o.Ow[r] = Ow(r); }
        for (float &f : o.F12) f = 0.f;
        o.epipole2[0] = o.epipole2[1] = 0.f;
    }
#endif  // RUMI_HAVE_SOPHUS
};

}  // namespace RUMI_FACADE_NAMESPACE

namespace rumi { using LocalMappingStep = RUMI_FACADE_NAMESPACE::LocalMappingStep; }
