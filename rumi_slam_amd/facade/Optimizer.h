// Drop-in for the two hot members of the all-static ORB_SLAM3::Optimizer (R/include/cloud_edge_slam_lib/Optimizer.h:53,55)
// over the MI355X C ABI (include/rumi_opt.h).  Templates over the data-model types, same member names as the reference:
// graph gathering (Optimizer.cc:763-897, :1011-1271), locking (MapPoint::mGlobalMutex, Map::mMutexMapUpdate) and the
// write-back / observation erasing (:993-1000, :1325-1354) stay here on the host; the arithmetic runs on the GPU.
#pragma once
#include <algorithm>
#include <cstdio>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "rumi_opt.h"
#include "rumi_status.h"
#ifdef RUMI_HAVE_SOPHUS
#include <cstring>
#include <type_traits>
#include "MapPointRefresh.h"     // LocalBundleAdjustmentResident hands UpdateNormalAndDepth of the window to RefreshMapPointsResident
#endif

// capacity of the per-thread optimiser arenas (key-frames incl. fixed ones, map points, observations of one call)
#ifndef RUMI_OPT_MAX_KF
#define RUMI_OPT_MAX_KF 512
#endif
#ifndef RUMI_OPT_MAX_MP
#define RUMI_OPT_MAX_MP (1 << 17)
#endif
#ifndef RUMI_OPT_MAX_EDGES
#define RUMI_OPT_MAX_EDGES (1 << 20)
#endif

// The classes live in ORB_SLAM3 when these headers REPLACE the reference's (member templates deduce the reference's own types at every call
// site), or in a namespace of their own when the reference's headers stay and facade/shells/*.cc forward to them (-DRUMI_FACADE_NAMESPACE=...).
#ifndef RUMI_FACADE_NAMESPACE
#define RUMI_FACADE_NAMESPACE ORB_SLAM3
#endif
namespace RUMI_FACADE_NAMESPACE {

class Optimizer {
    // pFrame->mvuRight[i] >= 0 where the data model has stereo coordinates (the reference's Frame does; monocular mocks may not)
    template <class F> static auto has_right_impl(const F &f, int i, int) -> decltype(f.mvuRight[i] >= 0, bool()) { return !f.mvuRight.empty() && f.mvuRight[i] >= 0; }
    template <class F> static bool has_right_impl(const F &, int, long) { return false; }
    template <class F> static bool has_right_coordinate(const F &f, int i) { return has_right_impl(f, i, 0); }

public:
    static RumiOptimizer *&arena_slot() { thread_local RumiOptimizer *o = nullptr; return o; }
    static int &arena_scale() { thread_local int s = 1; return s; }
    static RumiOptimizer *arena() {
        RumiOptimizer *&o = arena_slot();
        if (!o) {
            const int k = arena_scale();
            const int rc = rumi_opt_create((1 << 16) * k, 64 * k, RUMI_OPT_MAX_KF * k, RUMI_OPT_MAX_MP * k, RUMI_OPT_MAX_EDGES * k, -1, &o);
            if (rc != RUMI_OK) { rumi_facade::report("Optimizer: optimiser arena", rc); o = nullptr; }
        }
        return o;
    }
    static bool grow_arena() {                      // a call that exceeds the arena re-creates it twice as large (rumi_status.h)
        if (arena_scale() >= 16) return false;
        if (arena_slot()) { rumi_opt_destroy(arena_slot()); arena_slot() = nullptr; }
        arena_scale() *= 2;
        return arena() != nullptr;
    }

    // int static PoseOptimization(Frame *pFrame)          Optimizer.cc:723-1001 (mono branch)
    template <class FrameT> static int PoseOptimization(FrameT *pFrame) {
        using MapPointT = typename std::remove_pointer<typename std::decay<decltype(pFrame->mvpMapPoints[0])>::type>::type;
        const int N = pFrame->N;
        std::vector<float> Xw, obs, w;
        std::vector<int> index;
        int nStereo = 0;
        {
            std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);
            for (int i = 0; i < N; i++) {
                MapPointT *pMP = pFrame->mvpMapPoints[i];
                if (!pMP) continue;
                if (has_right_coordinate(*pFrame, i)) { nStereo++; continue; }   // EdgeStereoSE3ProjectXYZOnlyPose (:801-841): not built; reported below
                pFrame->mvbOutlier[i] = false;
                const auto &kpUn = pFrame->mvKeysUn[i];
                const auto P = pMP->GetWorldPos();
                Xw.push_back(P(0)); Xw.push_back(P(1)); Xw.push_back(P(2));
                obs.push_back(kpUn.pt.x); obs.push_back(kpUn.pt.y);
                w.push_back(pFrame->mvInvLevelSigma2[kpUn.octave]);
                index.push_back(i);
            }
        }
        if (nStereo > 0)
            rumi_facade::report("Optimizer::PoseOptimization", RUMI_E_INVALID, "observations with a right-image coordinate (mvuRight >= 0) reached the monocular PoseOptimization and were left out: the stereo edge is not built (DESIGN.md section 7)");
        const int n = (int)index.size();
        if (n < 3) return 0;
        const auto Tcw = pFrame->GetPose();
        const auto q = Tcw.unit_quaternion();
        const auto t = Tcw.translation();
        float T7[7] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2)};
        const float K4[4] = {pFrame->fx, pFrame->fy, pFrame->cx, pFrame->cy};
        std::vector<uint8_t> outlier(n);
        int32_t nGood = 0;
        if (RUMI_GUARDED("Optimizer / rumi_pose_optimization", &Optimizer::grow_arena, rumi_pose_optimization(arena(), Xw.data(), obs.data(), w.data(), n, K4, T7, outlier.data(), &nGood)) != RUMI_OK) return 0;
        for (int k = 0; k < n; k++) pFrame->mvbOutlier[index[k]] = outlier[k] != 0;
#ifdef RUMI_HAVE_SOPHUS
        pFrame->SetPose(Sophus::SE3f(Eigen::Quaternionf(T7[3], T7[0], T7[1], T7[2]), Eigen::Vector3f(T7[4], T7[5], T7[6])));   // :996-998
#else
        pFrame->SetPoseFromQuatTrans(T7);      // mock data model of tests/cpp (no Eigen / Sophus in this image)
#endif
        return nGood;
    }

    // void static LocalBundleAdjustment(KeyFrame *pMainKF, vector<KeyFrame *> vpAdjustKF, vector<KeyFrame *> vpFixedKF, bool *pbStopFlag)
    // — merge / welding-window BA, Optimizer.cc:3768-4183 (monocular observations).  Needs the members the reference uses there:
    // mnBALocalForMerge on KeyFrame and MapPoint, KeyFrame::GetMapPoints(), GetMapPoint(idx).
    template <class KeyFrameT>
    static void LocalBundleAdjustment(KeyFrameT *pMainKF, std::vector<KeyFrameT *> vpAdjustKF, std::vector<KeyFrameT *> vpFixedKF, bool *pbStopFlag) {
        using MapPointT = typename std::remove_pointer<typename std::decay<decltype(pMainKF->GetMapPointMatches()[0])>::type>::type;
        auto *pCurrentMap = pMainKF->GetMap();
        std::vector<MapPointT *> vpMPs;
        std::vector<KeyFrameT *> kfs;
        std::unordered_map<KeyFrameT *, int> kfId;
        std::vector<float> kfPose;
        std::vector<uint8_t> kfFixed;
        unsigned long maxKFid = 0;
        auto add_kf = [&](KeyFrameT *k, bool fixed) {                                         // :3793-3860
            if (k->isBad() || k->GetMap() != pCurrentMap) return;
            k->mnBALocalForMerge = pMainKF->mnId;
            kfId[k] = (int)kfs.size(); kfs.push_back(k);
            const auto T = k->GetPose(); const auto q = T.unit_quaternion(); const auto t = T.translation();
            const float p[7] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2)};
            kfPose.insert(kfPose.end(), p, p + 7);
            kfFixed.push_back(fixed);
            if ((unsigned long)k->mnId > maxKFid) maxKFid = (unsigned long)k->mnId;
            for (MapPointT *pMPi : k->GetMapPoints())
                if (pMPi && !pMPi->isBad() && pMPi->GetMap() == pCurrentMap && pMPi->mnBALocalForMerge != pMainKF->mnId) {
                    vpMPs.push_back(pMPi);
                    pMPi->mnBALocalForMerge = pMainKF->mnId;
                }
        };
        for (KeyFrameT *k : vpFixedKF) add_kf(k, true);
        for (KeyFrameT *k : vpAdjustKF) add_kf(k, false);
        // points that turned bad in between are skipped with their edges (:3877-3879); the rest in vpMPs order
        std::vector<MapPointT *> mps;
        std::vector<float> mpPos, eObs, eW;
        std::vector<int32_t> eMp, eKf;
        std::vector<KeyFrameT *> edgeKF;
        for (MapPointT *pMPi : vpMPs) {
            if (pMPi->isBad()) continue;
            const int p = (int)mps.size();
            mps.push_back(pMPi);
            const auto P = pMPi->GetWorldPos();
            mpPos.push_back(P(0)); mpPos.push_back(P(1)); mpPos.push_back(P(2));
            for (const auto &ob : pMPi->GetObservations()) {                                  // :3891-3925
                KeyFrameT *pKF = ob.first;
                const int idx = std::get<0>(ob.second);
                if (pKF->isBad() || (unsigned long)pKF->mnId > maxKFid || pKF->mnBALocalForMerge != pMainKF->mnId || !pKF->GetMapPoint(idx)) continue;
                if (!(pKF->mvuRight[idx] < 0)) continue;                                       // monocular observations only
                auto it = kfId.find(pKF);
                if (it == kfId.end()) continue;
                const auto &kpUn = pKF->mvKeysUn[idx];
                eMp.push_back(p); eKf.push_back(it->second);
                eObs.push_back(kpUn.pt.x); eObs.push_back(kpUn.pt.y);
                eW.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
                edgeKF.push_back(pKF);
            }
        }
        if (pbStopFlag && *pbStopFlag) return;                                                // :3982-3984
        if (kfs.empty()) return;
        const float K4[4] = {pMainKF->fx, pMainKF->fy, pMainKF->cx, pMainKF->cy};
        std::vector<uint8_t> erase(eMp.size() + 1);
        int32_t stats[4];
        if (RUMI_GUARDED("Optimizer / rumi_merge_ba", &Optimizer::grow_arena, rumi_merge_ba(arena(), (int)kfs.size(), kfPose.data(), kfFixed.data(), (int)mps.size(), mpPos.data(), (int)eMp.size(), eMp.data(),
                          eKf.data(), eObs.data(), eW.data(), K4, reinterpret_cast<const volatile uint8_t *>(pbStopFlag), erase.data(), stats)) != RUMI_OK) {
            return;
        }
        std::unique_lock<std::mutex> lock(pMainKF->GetMap()->mMutexMapUpdate);                // :4076
        for (size_t e = 0; e < eMp.size(); e++) {                                             // :4042-4085
            MapPointT *pMP = mps[eMp[e]];
            if (pMP->isBad() || !erase[e]) continue;
            edgeKF[e]->EraseMapPointMatch(pMP);
            pMP->EraseObservation(edgeKF[e]);
        }
        for (size_t k = 0; k < kfs.size(); k++) {                                             // :4108-4167: vpAdjustKF only
            if (kfFixed[k] || kfs[k]->isBad()) continue;
            const float *T7 = &kfPose[k * 7];
#ifdef RUMI_HAVE_SOPHUS
            kfs[k]->SetPose(Sophus::SE3f(Eigen::Quaternionf(T7[3], T7[0], T7[1], T7[2]), Eigen::Vector3f(T7[4], T7[5], T7[6])));
#else
            kfs[k]->SetPoseFromQuatTrans(T7);
#endif
        }
        for (size_t p = 0; p < mps.size(); p++) {                                             // :4169-4177
            if (mps[p]->isBad()) continue;
#ifdef RUMI_HAVE_SOPHUS
            mps[p]->SetWorldPos(Eigen::Vector3f(mpPos[3 * p], mpPos[3 * p + 1], mpPos[3 * p + 2]));
#else
            mps[p]->SetWorldPosXYZ(mpPos[3 * p], mpPos[3 * p + 1], mpPos[3 * p + 2]);
#endif
            mps[p]->UpdateNormalAndDepth();
        }
    }

    // void static LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap, int &num_fixedKF, int &num_OptKF, int &num_MPs, int &num_edges)
    template <class KeyFrameT, class MapT>
    static void LocalBundleAdjustment(KeyFrameT *pKF, bool *pbStopFlag, MapT *pMap, int &num_fixedKF, int &num_OptKF, int &num_MPs, int &num_edges) {
        using MapPointT = typename std::remove_pointer<typename std::decay<decltype(pKF->GetMapPointMatches()[0])>::type>::type;
        // Local KeyFrames: first breadth search from the current key-frame (:1004-1017)
        std::list<KeyFrameT *> lLocalKeyFrames;
        lLocalKeyFrames.push_back(pKF);
        pKF->mnBALocalForKF = pKF->mnId;
        auto *pCurrentMap = pKF->GetMap();
        for (KeyFrameT *pKFi : pKF->GetVectorCovisibleKeyFrames()) {
            pKFi->mnBALocalForKF = pKF->mnId;
            if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lLocalKeyFrames.push_back(pKFi);
        }
        // Local MapPoints seen in local key-frames (:1019-1039)
        num_fixedKF = 0;
        std::list<MapPointT *> lLocalMapPoints;
        for (KeyFrameT *pKFi : lLocalKeyFrames) {
            if (pKFi->mnId == pMap->GetInitKFid()) num_fixedKF = 1;
            for (MapPointT *pMP : pKFi->GetMapPointMatches())
                if (pMP && !pMP->isBad() && pMP->GetMap() == pCurrentMap && pMP->mnBALocalForKF != pKF->mnId) {
                    lLocalMapPoints.push_back(pMP);
                    pMP->mnBALocalForKF = pKF->mnId;
                }
        }
        // Fixed key-frames: see local map points but are not local (:1041-1055)
        std::list<KeyFrameT *> lFixedCameras;
        for (MapPointT *pMP : lLocalMapPoints)
            for (const auto &ob : pMP->GetObservations()) {
                KeyFrameT *pKFi = ob.first;
                if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                    pKFi->mnBAFixedForKF = pKF->mnId;
                    if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lFixedCameras.push_back(pKFi);
                }
            }
        num_fixedKF = (int)lFixedCameras.size() + num_fixedKF;
        if (num_fixedKF == 0) return;                                                        // :1057-1060

        // flatten: vertices then edges in the reference's construction order (:1088-1271)
        std::vector<KeyFrameT *> kfs;
        std::unordered_map<KeyFrameT *, int> kfId;
        std::vector<float> kfPose;
        std::vector<uint8_t> kfFixed;
        auto add_kf = [&](KeyFrameT *k, bool fixed) {
            kfId[k] = (int)kfs.size(); kfs.push_back(k);
            const auto T = k->GetPose(); const auto q = T.unit_quaternion(); const auto t = T.translation();
            const float p[7] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2)};
            kfPose.insert(kfPose.end(), p, p + 7);
            kfFixed.push_back(fixed);
        };
        for (KeyFrameT *k : lLocalKeyFrames) add_kf(k, k->mnId == pMap->GetInitKFid());
        num_OptKF = (int)lLocalKeyFrames.size();
        for (KeyFrameT *k : lFixedCameras) add_kf(k, true);
        std::vector<MapPointT *> mps(lLocalMapPoints.begin(), lLocalMapPoints.end());
        std::vector<float> mpPos, eObs, eW;
        std::vector<int32_t> eMp, eKf;
        std::vector<KeyFrameT *> edgeKF;
        for (size_t p = 0; p < mps.size(); p++) {
            const auto P = mps[p]->GetWorldPos();
            mpPos.push_back(P(0)); mpPos.push_back(P(1)); mpPos.push_back(P(2));
            for (const auto &ob : mps[p]->GetObservations()) {
                KeyFrameT *pKFi = ob.first;
                if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;
                const int leftIndex = std::get<0>(ob.second);
                if (leftIndex == -1 || !(pKFi->mvuRight[leftIndex] < 0)) continue;             // monocular observations only
                auto it = kfId.find(pKFi);
                if (it == kfId.end()) continue;
                const auto &kpUn = pKFi->mvKeysUn[leftIndex];
                eMp.push_back((int32_t)p); eKf.push_back(it->second);
                eObs.push_back(kpUn.pt.x); eObs.push_back(kpUn.pt.y);
                eW.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
                edgeKF.push_back(pKFi);
            }
        }
        num_MPs = (int)mps.size();
        num_edges = (int)eMp.size();
        if (pbStopFlag && *pbStopFlag) return;                                                // :1274-1276
        const float K4[4] = {pKF->fx, pKF->fy, pKF->cx, pKF->cy};
        std::vector<uint8_t> erase(eMp.size() + 1);
        int32_t stats[4];
        if (RUMI_GUARDED("Optimizer / rumi_local_ba", &Optimizer::grow_arena, rumi_local_ba(arena(), (int)kfs.size(), kfPose.data(), kfFixed.data(), (int)mps.size(), mpPos.data(), (int)eMp.size(), eMp.data(),
                          eKf.data(), eObs.data(), eW.data(), K4, reinterpret_cast<const volatile uint8_t *>(pbStopFlag), erase.data(), stats)) != RUMI_OK)
            return;
        if (stats[3]) return;
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                             // :1325
        for (size_t e = 0; e < eMp.size(); e++) {
            MapPointT *pMP = mps[eMp[e]];
            if (pMP->isBad() || !erase[e]) continue;
            edgeKF[e]->EraseMapPointMatch(pMP);
            pMP->EraseObservation(edgeKF[e]);
        }
        for (size_t k = 0; k < kfs.size(); k++)
            if ((int)k < num_OptKF) {                                                        // :1338-1344
                const float *T7 = &kfPose[k * 7];
#ifdef RUMI_HAVE_SOPHUS
                kfs[k]->SetPose(Sophus::SE3f(Eigen::Quaternionf(T7[3], T7[0], T7[1], T7[2]), Eigen::Vector3f(T7[4], T7[5], T7[6])));
#else
                kfs[k]->SetPoseFromQuatTrans(T7);
#endif
            }
        for (size_t p = 0; p < mps.size(); p++) {
#ifdef RUMI_HAVE_SOPHUS
            mps[p]->SetWorldPos(Eigen::Vector3f(mpPos[3 * p], mpPos[3 * p + 1], mpPos[3 * p + 2]));                              // :1347-1351
#else
            mps[p]->SetWorldPosXYZ(mpPos[3 * p], mpPos[3 * p + 1], mpPos[3 * p + 2]);
#endif
            mps[p]->UpdateNormalAndDepth();
        }
        pMap->IncreaseChangeIndex();
    }

#ifdef RUMI_HAVE_SOPHUS
    // The same member over a CovisibilityGraph that holds the map (rumi_local_ba_resident, include/rumi_opt.h): the walk of the live objects
    // above (:1003-1271) is replaced by one device call that names slots; the host replays :1327-1351 on the objects in the returned order.
    // The store must be current for the window: Sync of its key-frames and points, SyncFeatures, SyncAttributes, SyncReferences, SyncCentres,
    // SyncPoses and SyncPointMaps.  Afterwards the store is synced by what changed here (rows and observer rows of the erased
    // observations, references, centres; positions and poses are already there), and UpdateNormalAndDepth of all window points goes as one
    // RefreshMapPointsResident (normal and depth) instead of the per-point loop.  A raised stop flag returns before anything is written,
    // the counters included.  Errors are reported (rumi_status.h) and nothing is written; no fixed key-frame returns silently as upstream.
    template <class GraphT, class KeyFrameT, class MapT>
    static void LocalBundleAdjustmentResident(GraphT &graph, KeyFrameT *pKF, bool *pbStopFlag, MapT *pMap, int &num_fixedKF, int &num_OptKF, int &num_MPs, int &num_edges) {
        using MapPointT = typename std::remove_pointer<typename std::decay<decltype(pKF->GetMapPointMatches()[0])>::type>::type;
        static const char *where = "Optimizer::LocalBundleAdjustmentResident";
        const int32_t cur = graph.SlotOf(pKF);
        std::vector<int32_t> neigh;
        int32_t init = -1;
        bool seen = cur >= 0;
        if (seen && pKF->mnId == pMap->GetInitKFid()) init = cur;
        for (KeyFrameT *pKFi : pKF->GetVectorCovisibleKeyFrames()) {
            const int32_t s = graph.SlotOf(pKFi);
            seen = seen && s >= 0;
            neigh.push_back(s);
            if (pKFi->mnId == pMap->GetInitKFid()) init = s;             // a local key-frame is a fixed vertex iff it is the initial one (:1094)
        }
        if (!seen) { rumi_facade::report(where, RUMI_E_INVALID, "the current key-frame or a covisible one has not been synced to the graph"); return; }
        const int kfCap = graph.KeyFrameCount(), mpCap = graph.PointCount();
        thread_local std::vector<int32_t> erased(3 << 12);
        std::vector<int32_t> kfSlots(kfCap), mpIds(mpCap);
        std::vector<float> kfPose((size_t)kfCap * 7), mpPos((size_t)mpCap * 3);
        RumiLbaResidentOut out{};
        int rc;
        for (;;) {
            out = RumiLbaResidentOut{};
            out.kf_cap = kfCap; out.mp_cap = mpCap; out.erase_cap = (int32_t)(erased.size() / 3);
            out.kf_slots = kfSlots.data(); out.kf_pose7 = kfPose.data(); out.mp_ids = mpIds.data(); out.mp_pos3 = mpPos.data(); out.erased = erased.data();
            rc = rumi_local_ba_resident(arena(), graph.handle(), cur, neigh.data(), (int32_t)neigh.size(), init, reinterpret_cast<const volatile uint8_t *>(pbStopFlag), &out);
            if (rc != RUMI_E_CAPACITY) break;
            const char *msg = rumi_last_error();
            if (msg && std::strstr(msg, "erase_cap")) { if (erased.size() > ((size_t)3 << 26)) break; erased.resize(erased.size() * 2); }   // nothing was written: solve again
            else if (!grow_arena()) break;
        }
        if (rc == RUMI_E_INVALID && rumi_last_error() && std::strncmp(rumi_last_error(), "LM-LBA", 6) == 0) return;                 // :1057-1060
        if (rc != RUMI_OK) { rumi_facade::report(where, rc); return; }
        if (out.stats[3]) return;                                                            // :1274-1276
        num_fixedKF = out.num_fixedKF; num_OptKF = out.num_OptKF; num_MPs = out.num_MPs; num_edges = out.num_edges;
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                             // :1325
        std::vector<KeyFrameT *> rowChanged, locals;
        std::vector<MapPointT *> obsChanged, window;
        std::set<KeyFrameT *> inK;
        std::set<MapPointT *> inP;
        for (int i = 0; i < out.n_erased; i++) {                                             // :1327-1334, in edge order
            KeyFrameT *pKFi = graph.KeyFrameAt(erased[3 * i]);
            MapPointT *pMPi = graph.PointAt(erased[3 * i + 1]);
            if (pMPi->isBad()) continue;                                                     // went bad since the call (:1289)
            pKFi->EraseMapPointMatch(pMPi);
            pMPi->EraseObservation(pKFi);
            if (inK.insert(pKFi).second) rowChanged.push_back(pKFi);
            if (inP.insert(pMPi).second) obsChanged.push_back(pMPi);
        }
        for (int k = 0; k < out.num_OptKF; k++) {                                            // :1338-1344
            const float *T7 = &kfPose[(size_t)k * 7];
            KeyFrameT *pKFi = graph.KeyFrameAt(kfSlots[k]);
            pKFi->SetPose(Sophus::SE3f(Eigen::Quaternionf(T7[3], T7[0], T7[1], T7[2]), Eigen::Vector3f(T7[4], T7[5], T7[6])));
            locals.push_back(pKFi);
        }
        for (int p = 0; p < out.num_MPs; p++) {                                              // :1347-1350
            MapPointT *pMP = graph.PointAt(mpIds[p]);
            pMP->SetWorldPos(Eigen::Vector3f(mpPos[3 * p], mpPos[3 * p + 1], mpPos[3 * p + 2]));
            window.push_back(pMP);
        }
        // the store, by what changed: the device call left positions and poses there already
        bool ok = true;
        for (KeyFrameT *k : rowChanged) ok = ok && graph.Sync(k) == RUMI_OK;
        for (MapPointT *p : obsChanged) ok = ok && graph.Sync(p) == RUMI_OK;
        ok = ok && graph.SyncReferences(obsChanged) == RUMI_OK && graph.SyncCentres(locals) == RUMI_OK;
        if (ok) rumi_facade::RefreshMapPointsResident(graph, window, RUMI_REFRESH_NORMAL_DEPTH);   // :1351, every window point in one call
        pMap->IncreaseChangeIndex();
    }

    // void static BundleAdjustment(const vector<KeyFrame *> &vpKFs, const vector<MapPoint *> &vpMP, int nIterations = 5, bool *pbStopFlag = NULL,
    //                              const unsigned long nLoopKF = 0, const bool bRobust = true)                Optimizer.cc:54-351 (monocular edges)
    template <class KeyFrameT, class MapPointT>
    static void BundleAdjustment(const std::vector<KeyFrameT *> &vpKFs, const std::vector<MapPointT *> &vpMP, int nIterations = 5, bool *pbStopFlag = nullptr,
                                 const unsigned long nLoopKF = 0, const bool bRobust = true) {
        std::vector<bool> vbNotIncludedMP(vpMP.size(), false);
        auto *pMap = vpKFs[0]->GetMap();
        std::vector<KeyFrameT *> kfs;
        std::unordered_map<KeyFrameT *, int> kfId;
        std::vector<float> kfPose;
        std::vector<uint8_t> kfFixed;
        unsigned long maxKFid = 0;
        for (KeyFrameT *pKF : vpKFs) {                                                        // :103-115
            if (pKF->isBad()) continue;
            kfId[pKF] = (int)kfs.size(); kfs.push_back(pKF);
            const auto T = pKF->GetPose(); const auto q = T.unit_quaternion(); const auto t = T.translation();
            const float p7[7] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2)};
            kfPose.insert(kfPose.end(), p7, p7 + 7);
            kfFixed.push_back(pKF->mnId == pMap->GetInitKFid());
            if ((unsigned long)pKF->mnId > maxKFid) maxKFid = pKF->mnId;
        }
        std::vector<MapPointT *> mps;
        std::vector<size_t> mpIndex;
        std::vector<float> mpPos, eObs, eW;
        std::vector<int32_t> eMp, eKf;
        for (size_t i = 0; i < vpMP.size(); i++) {                                            // :123-253
            MapPointT *pMP = vpMP[i];
            if (pMP->isBad()) continue;
            const auto P = pMP->GetWorldPos();
            int nEdges = 0;
            for (const auto &ob : pMP->GetObservations()) {
                KeyFrameT *pKF = ob.first;
                if (pKF->isBad() || (unsigned long)pKF->mnId > maxKFid) continue;
                auto it = kfId.find(pKF);
                if (it == kfId.end()) continue;                                               // optimizer.vertex(pKF->mnId) == NULL
                nEdges++;
                const int leftIndex = std::get<0>(ob.second);
                if (leftIndex == -1 || !(pKF->mvuRight[leftIndex] < 0)) continue;             // monocular observations only
                const auto &kpUn = pKF->mvKeysUn[leftIndex];
                eMp.push_back((int32_t)mps.size()); eKf.push_back(it->second);
                eObs.push_back(kpUn.pt.x); eObs.push_back(kpUn.pt.y);
                eW.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
            }
            if (nEdges == 0) { vbNotIncludedMP[i] = true; continue; }                         // :251-254: the vertex is removed again
            mps.push_back(pMP); mpIndex.push_back(i);
            mpPos.push_back(P(0)); mpPos.push_back(P(1)); mpPos.push_back(P(2));
        }
        if (kfs.empty()) return;
        const float K4[4] = {kfs[0]->fx, kfs[0]->fy, kfs[0]->cx, kfs[0]->cy};
        int32_t stats[4];
        if (RUMI_GUARDED("Optimizer / rumi_bundle_adjustment", &Optimizer::grow_arena, rumi_bundle_adjustment(arena(), (int)kfs.size(), kfPose.data(), kfFixed.data(), (int)mps.size(), mpPos.data(), (int)eMp.size(), eMp.data(), eKf.data(),
                                   eObs.data(), eW.data(), K4, reinterpret_cast<const volatile uint8_t *>(pbStopFlag), nIterations, bRobust, stats)) != RUMI_OK) {
            return;
        }
        const bool direct = nLoopKF == (unsigned long)pMap->GetOriginKF()->mnId;
        for (size_t k = 0; k < kfs.size(); k++) {                                             // :264-327
            const float *T7 = &kfPose[k * 7];
            const Sophus::SE3f T(Eigen::Quaternionf(T7[3], T7[0], T7[1], T7[2]), Eigen::Vector3f(T7[4], T7[5], T7[6]));
            if (direct) kfs[k]->SetPose(T);
            else { kfs[k]->mTcwGBA = T; kfs[k]->mnBAGlobalForKF = nLoopKF; }
        }
        for (size_t p = 0; p < mps.size(); p++) {                                             // :330-349
            const Eigen::Vector3f X(mpPos[3 * p], mpPos[3 * p + 1], mpPos[3 * p + 2]);
            if (direct) { mps[p]->SetWorldPos(X); mps[p]->UpdateNormalAndDepth(); }
            else { mps[p]->mPosGBA = X; mps[p]->mnBAGlobalForKF = nLoopKF; }
        }
    }

    // void static GlobalBundleAdjustemnt(Map *pMap, int nIterations = 5, bool *pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true)   :48-52
    template <class MapT>
    static void GlobalBundleAdjustemnt(MapT *pMap, int nIterations = 5, bool *pbStopFlag = nullptr, const unsigned long nLoopKF = 0, const bool bRobust = true) {
        BundleAdjustment(pMap->GetAllKeyFrames(), pMap->GetAllMapPoints(), nIterations, pbStopFlag, nLoopKF, bRobust);
    }
#endif

#ifdef RUMI_HAVE_SOPHUS
    // Gathers one correspondence of OptimizeSim3 / OptimizeCloudSim3 (Optimizer.cc:1972-2100, :2246-2392); false when the reference skips it.
    struct Sim3Gather {
        std::vector<float> P1c, P2c, obs1, obs2, w1, w2;
        std::vector<uint8_t> skip12, skip21;
        std::vector<int32_t> pairOf;
        std::vector<size_t> index;             // vnIndexEdge
        int n() const { return (int)w1.size(); }
    };
    template <class KeyFrameT, class MapPointT>
    static bool sim3_gather(Sim3Gather &g, KeyFrameT *pKF1, KeyFrameT *pKF2, MapPointT *pMP1, MapPointT *pMP2, size_t i, int pair, bool bAllPoints) {
        if (!pMP1 || !pMP2) return false;                                              // "match without map point": vertices only, no edges (:2016-2031)
        if (pMP1->isBad() || pMP2->isBad()) return false;                              // :2011-2014
        const int i2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));
        const auto P3D1c = pKF1->GetRotation() * pMP1->GetWorldPos() + pKF1->GetTranslation();   // :1990, :1997
        const auto P3D2c = pKF2->GetRotation() * pMP2->GetWorldPos() + pKF2->GetTranslation();
        if (i2 < 0 && !bAllPoints) return false;                                       // :2033-2036
        if (P3D2c(2) < 0) return false;                                                // :2038-2041
        const auto &kpUn1 = pKF1->mvKeysUn[i];
        float ox, oy; int octave2;
        if (i2 >= 0) { const auto &kpUn2 = pKF2->mvKeysUn[i2]; ox = kpUn2.pt.x; oy = kpUn2.pt.y; octave2 = kpUn2.octave; }
        else { const float invz = 1 / P3D2c(2); ox = P3D2c(0) * invz; oy = P3D2c(1) * invz; octave2 = pMP2->mnTrackScaleLevel; }   // :2065-2071
        for (int c = 0; c < 3; c++) { g.P1c.push_back(P3D1c(c)); g.P2c.push_back(P3D2c(c)); }
        g.obs1.push_back(kpUn1.pt.x); g.obs1.push_back(kpUn1.pt.y); g.obs2.push_back(ox); g.obs2.push_back(oy);
        g.w1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]); g.w2.push_back(pKF2->mvInvLevelSigma2[octave2]);
        g.skip12.push_back(pMP2->isEdge); g.skip21.push_back(pMP1->isEdge);
        g.pairOf.push_back(pair); g.index.push_back(i);
        return true;
    }
    template <class Sim3T> static void sim3_to8(const Sim3T &S, double *o) {
        const auto q = S.rotation(); const auto t = S.translation();
        o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); o[3] = q.w(); o[4] = t(0); o[5] = t(1); o[6] = t(2); o[7] = S.scale();
    }
    template <class Sim3T> static Sim3T sim3_from8(const double *S) {
        return Sim3T(Eigen::Quaterniond(S[3], S[0], S[1], S[2]), Eigen::Vector3d(S[4], S[5], S[6]), S[7]);
    }

    // static int OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
    //                         const bool bFixScale, Eigen::Matrix<double, 7, 7> &mAcumHessian, const bool bAllPoints)      Optimizer.cc:1920-2167
    template <class KeyFrameT, class MapPointT, class Sim3T, class HessianT>
    static int OptimizeSim3(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches1, Sim3T &g2oS12, const float th2, const bool bFixScale,
                            HessianT &mAcumHessian, const bool bAllPoints = false) {
        const int N = (int)vpMatches1.size();
        const auto vpMapPoints1 = pKF1->GetMapPointMatches();
        Sim3Gather g;
        for (int i = 0; i < N; i++) {
            if (!vpMatches1[i]) continue;
            sim3_gather(g, pKF1, pKF2, vpMapPoints1[i], vpMatches1[i], (size_t)i, 0, bAllPoints);
        }
        // the isEdge tests belong to the cloud variant only: here both edges always exist
        const float K1[4] = {pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy}, K2[4] = {pKF2->fx, pKF2->fy, pKF2->cx, pKF2->cy};
        double S[8];
        sim3_to8(g2oS12, S);
        std::vector<uint8_t> status(g.n() + 1);
        int32_t res[3] = {0, 0, 1};
        if (RUMI_GUARDED("Optimizer / rumi_optimize_sim3", &Optimizer::grow_arena, rumi_optimize_sim3(arena(), g.n(), nullptr, 0, nullptr, nullptr, g.P1c.data(), g.P2c.data(), g.obs1.data(), g.obs2.data(), g.w1.data(), g.w2.data(),
                               nullptr, nullptr, K1, K2, th2, bFixScale, 1, S, status.data(), res)) != RUMI_OK) {
            std::fprintf(stderr, "OptimizeSim3: %s\n", rumi_last_error());
            return 0;
        }
        for (int k = 0; k < g.n(); k++)
            if (status[k] == 1 || (!res[2] && status[k] == 2)) vpMatches1[g.index[k]] = static_cast<MapPointT *>(nullptr);   // :2112, :2156
        if (res[2]) return 0;                                                          // :2135-2136: g2oS12 keeps its value
        mAcumHessian.setZero();                                                        // :2144 (never accumulated upstream)
        g2oS12 = sim3_from8<Sim3T>(S);                                                 // :2163-2164
        return res[0];
    }

    // static float OptimizeCloudSim3(const vector<KeyFrame *> &map1KFs, const vector<KeyFrame *> &map2KFs, const vector<vector<MapPoint *>> &avpMatches,
    //                                g2o::Sim3 &gSw1w2, const float th2, const bool bFixScale, Eigen::Matrix<double, 7, 7> &mAcumHessian,
    //                                const bool bAllPoints)                                                              Optimizer.cc:2169-2471
    template <class KeyFrameT, class MapPointT, class Sim3T, class HessianT>
    static float OptimizeCloudSim3(const std::vector<KeyFrameT *> &map1KFs, const std::vector<KeyFrameT *> &map2KFs,
                                   const std::vector<std::vector<MapPointT *>> &avpMatches, Sim3T &gSw1w2, const float th2, const bool bFixScale,
                                   HessianT &mAcumHessian, const bool bAllPoints = false) {
        Sim3Gather g;
        std::vector<double> A, B;
        for (size_t k = 0; k < map2KFs.size(); ++k) {
            KeyFrameT *pKF1 = map1KFs[k], *pKF2 = map2KFs[k];
            const Sim3T gSc1w(pKF1->GetRotation().template cast<double>(), pKF1->GetTranslation().template cast<double>(), 1.0);   // :2231-2232
            const Sim3T gSc2w(pKF2->GetRotation().template cast<double>(), pKF2->GetTranslation().template cast<double>(), 1.0);
            double a[8], b[8];
            sim3_to8(gSc1w, a); sim3_to8(gSc2w, b);
            A.insert(A.end(), a, a + 8); B.insert(B.end(), b, b + 8);
            const auto &vpMatches1 = avpMatches[k];
            const auto vpMapPoints1 = pKF1->GetMapPointMatches();
            for (size_t i = 0; i < vpMatches1.size(); i++) {
                if (!vpMapPoints1[i] || !vpMatches1[i]) continue;                       // :2251-2252
                sim3_gather(g, pKF1, pKF2, vpMapPoints1[i], vpMatches1[i], i, (int)k, bAllPoints);
            }
        }
        if (map2KFs.empty()) return 0.f;
        const float K1[4] = {map1KFs[0]->fx, map1KFs[0]->fy, map1KFs[0]->cx, map1KFs[0]->cy};   // vSim3->pCamera1 = map1KFs[0]->mpCamera (:2192-2193)
        const float K2[4] = {map2KFs[0]->fx, map2KFs[0]->fy, map2KFs[0]->cx, map2KFs[0]->cy};
        double S[8];
        sim3_to8(gSw1w2, S);
        std::vector<uint8_t> status(g.n() + 1);
        int32_t res[3] = {0, 0, 1};
        if (RUMI_GUARDED("Optimizer / rumi_optimize_sim3", &Optimizer::grow_arena, rumi_optimize_sim3(arena(), g.n(), g.pairOf.data(), (int32_t)map2KFs.size(), A.data(), B.data(), g.P1c.data(), g.P2c.data(), g.obs1.data(),
                               g.obs2.data(), g.w1.data(), g.w2.data(), g.skip12.data(), g.skip21.data(), K1, K2, th2, bFixScale, 0, S, status.data(), res)) != RUMI_OK) {
            std::fprintf(stderr, "OptimizeCloudSim3: %s\n", rumi_last_error());
            return 0.f;
        }
        gSw1w2 = sim3_from8<Sim3T>(S);                                                 // :2397 (before the early return) and :2466
        if (res[2]) return 0;                                                          // :2437-2438
        mAcumHessian.setZero();                                                        // :2446
        return (float)res[0] / (float)g.n();                                           // :2468
    }
    // ---- Optimizer::OptimizeEssentialGraph, both overloads (Optimizer.cc:1357-1623, :1625-1918), over rumi_essential_graph and
    //      rumi_sim3_correct_points.  The graph is gathered as upstream gathers it, measurements are formed in double on the host. ----
    struct EssentialGraphFlat {                 // the flattened graph; vertex k is key-frame id[k]
        std::vector<unsigned long> id;
        std::vector<double> S, meas;
        std::vector<uint8_t> fixed, fix_scale;
        std::vector<int32_t> v0, v1;
        int32_t stats[4] = {0, 0, 0, 0};
        int add_vertex(unsigned long kfId, const double *S8, bool fix, bool fs) {
            id.push_back(kfId); S.insert(S.end(), S8, S8 + 8); fixed.push_back(fix); fix_scale.push_back(fs);
            return (int)id.size() - 1;
        }
        void add_edge(int i, int j, const double *Sji) { v0.push_back(i); v1.push_back(j); meas.insert(meas.end(), Sji, Sji + 8); }   // setVertex(0, i), setVertex(1, j)
    };
    // tests set this to receive a copy of the graph the next call gathers (per thread)
    static EssentialGraphFlat *&essential_graph_record() { thread_local EssentialGraphFlat *r = nullptr; return r; }

private:
    // g2o::Sim3 on (qx qy qz qw tx ty tz s) doubles: operator* (sim3.h:266-272), inverse (:233-236), Sim3(q, t, 1.0) of a float pose
    static void eg_rot(const double *q, const double *v, double *o) {
        const double ux = 2 * (q[1] * v[2] - q[2] * v[1]), uy = 2 * (q[2] * v[0] - q[0] * v[2]), uz = 2 * (q[0] * v[1] - q[1] * v[0]);
        o[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy); o[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz); o[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
    }
    static void eg_mul(const double *a, const double *b, double *o) {
        double r[3];
        eg_rot(a, b + 4, r);
        const double q[4] = {a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                             a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]};
        for (int k = 0; k < 4; k++) o[k] = q[k];
        for (int k = 0; k < 3; k++) o[4 + k] = a[7] * r[k] + a[4 + k];
        o[7] = a[7] * b[7];
    }
    static void eg_inv(const double *a, double *o) {
        const double c[4] = {-a[0], -a[1], -a[2], a[3]}, k = -1. / a[7], t[3] = {k * a[4], k * a[5], k * a[6]};
        double r[3];
        eg_rot(c, t, r);
        for (int i = 0; i < 4; i++) o[i] = c[i];
        for (int i = 0; i < 3; i++) o[4 + i] = r[i];
        o[7] = 1. / a[7];
    }
    static void eg_identity(double *o) { o[0] = o[1] = o[2] = 0; o[3] = 1; o[4] = o[5] = o[6] = 0; o[7] = 1; }
    template <class SE3T> static void eg_from_pose(const SE3T &T, double *o) {          // Tcw.cast<double>() -> g2o::Sim3(q, t, 1.0)
        const auto q = T.unit_quaternion(); const auto t = T.translation();
        o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); o[3] = q.w(); o[4] = t(0); o[5] = t(1); o[6] = t(2); o[7] = 1.0;
    }
    template <class SE3T> static void eg_pose7(const SE3T &T, float *o) {
        const auto q = T.unit_quaternion(); const auto t = T.translation();
        o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); o[3] = q.w(); o[4] = t(0); o[5] = t(1); o[6] = t(2);
    }
    static bool eg_solve(EssentialGraphFlat &g, const char *where) {
        if (EssentialGraphFlat *r = essential_graph_record()) *r = g;
        std::vector<double> trace(21);
        const int rc = RUMI_GUARDED(where, &Optimizer::grow_arena, rumi_essential_graph(arena(), (int32_t)g.id.size(), g.S.data(), g.fixed.data(), g.fix_scale.data(),
                                    (int32_t)g.v0.size(), g.v0.data(), g.v1.data(), g.meas.data(), 20, nullptr, g.stats, trace.data()));
        if (EssentialGraphFlat *r = essential_graph_record()) for (int k = 0; k < 4; k++) r->stats[k] = g.stats[k];
        return rc == RUMI_OK;
    }

public:
    // void static OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
    //                                    const LoopClosing::KeyFrameAndPose &CorrectedSim3, const map<KeyFrame *, set<KeyFrame *>> &LoopConnections,
    //                                    const bool &bFixScale)                                                  Optimizer.cc:1357-1623
    // Bad key-frames get no vertex (:1390) and, unlike upstream (which would dereference a null vertex), are passed over wherever they would
    // be an edge's end.  The inertial edge of :1550-1565 is not built: a key-frame with bImu and mPrevKF is reported and goes without it.
    template <class MapT, class KeyFrameT, class PoseMapT, class ConnT>
    static void OptimizeEssentialGraph(MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const PoseMapT &NonCorrectedSim3, const PoseMapT &CorrectedSim3,
                                       const ConnT &LoopConnections, const bool &bFixScale) {
        const auto vpKFs = pMap->GetAllKeyFrames();
        const auto vpMPs = pMap->GetAllMapPoints();
        const int minFeat = 100;
        EssentialGraphFlat g;
        std::map<unsigned long, int> vertexOf;
        for (size_t i = 0; i < vpKFs.size(); i++) {                                   // :1387-1419
            KeyFrameT *pKF = vpKFs[i];
            if (pKF->isBad()) continue;
            double S[8];
            const auto it = CorrectedSim3.find(pKF);
            if (it != CorrectedSim3.end()) sim3_to8(it->second, S); else eg_from_pose(pKF->GetPose(), S);
            vertexOf[pKF->mnId] = g.add_vertex(pKF->mnId, S, (long)pKF->mnId == (long)pMap->GetInitKFid(), bFixScale);
        }
        const std::vector<double> vScw = g.S;                                          // vScw[nIDi], by vertex
        auto vertex = [&](KeyFrameT *p) { const auto f = vertexOf.find(p->mnId); return f == vertexOf.end() ? -1 : f->second; };
        auto non_corrected = [&](KeyFrameT *p, int v, double *o) {                     // NonCorrectedSim3 if it holds the key-frame, else vScw
            const auto f = NonCorrectedSim3.find(p);
            if (f != NonCorrectedSim3.end()) sim3_to8(f->second, o); else for (int k = 0; k < 8; k++) o[k] = vScw[8 * (size_t)v + k];
        };
        std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
        for (auto mit = LoopConnections.begin(); mit != LoopConnections.end(); ++mit) {   // loop edges, :1425-1463
            KeyFrameT *pKF = mit->first;
            const int vi = vertex(pKF);
            if (vi < 0) continue;
            const unsigned long nIDi = pKF->mnId;
            double Swi[8], Sji[8];
            eg_inv(&vScw[8 * (size_t)vi], Swi);
            for (auto sit = mit->second.begin(); sit != mit->second.end(); ++sit) {
                const unsigned long nIDj = (*sit)->mnId;
                if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
                const int vj = vertex(*sit);
                if (vj < 0) continue;
                eg_mul(&vScw[8 * (size_t)vj], Swi, Sji);
                g.add_edge(vi, vj, Sji);
                sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
            }
        }
        bool inertial = false;
        for (size_t i = 0; i < vpKFs.size(); i++) {                                   // normal edges, :1465-1566
            KeyFrameT *pKF = vpKFs[i];
            const int vi = vertex(pKF);
            if (vi < 0 || pKF->isBad()) continue;
            double Siw[8], Swi[8], Sjw[8], Sji[8];
            non_corrected(pKF, vi, Siw);
            eg_inv(Siw, Swi);
            KeyFrameT *pParentKF = pKF->GetParent();
            if (pParentKF && vertex(pParentKF) >= 0) {                                 // spanning tree
                const int vj = vertex(pParentKF);
                non_corrected(pParentKF, vj, Sjw);
                eg_mul(Sjw, Swi, Sji);
                g.add_edge(vi, vj, Sji);
            }
            const auto sLoopEdges = pKF->GetLoopEdges();                               // earlier loop edges
            for (auto sit = sLoopEdges.begin(); sit != sLoopEdges.end(); ++sit) {
                KeyFrameT *pLKF = *sit;
                const int vl = vertex(pLKF);
                if (pLKF->mnId < pKF->mnId && vl >= 0) {
                    non_corrected(pLKF, vl, Sjw);
                    eg_mul(Sjw, Swi, Sji);
                    g.add_edge(vi, vl, Sji);
                }
            }
            const auto vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);           // covisibility graph
            for (auto vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); ++vit) {
                KeyFrameT *pKFn = *vit;
                if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn)) {
                    if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                        if (sInsertedEdges.count(std::make_pair(std::min<unsigned long>(pKF->mnId, pKFn->mnId), std::max<unsigned long>(pKF->mnId, pKFn->mnId)))) continue;
                        const int vn = vertex(pKFn);
                        if (vn < 0) continue;
                        non_corrected(pKFn, vn, Sjw);
                        eg_mul(Sjw, Swi, Sji);
                        g.add_edge(vi, vn, Sji);
                    }
                }
            }
            if (pKF->bImu && pKF->mPrevKF) inertial = true;
        }
        if (inertial) rumi_facade::report("Optimizer::OptimizeEssentialGraph", RUMI_E_INVALID, "key-frames with bImu and mPrevKF: the inertial edge (Optimizer.cc:1550-1565) is not built and was left out (DESIGN.md section 7)");
        if (!eg_solve(g, "Optimizer / rumi_essential_graph")) return;
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
        const int nV = (int)g.id.size();
        std::vector<double> vCorrectedSwc((size_t)nV * 8);
        for (size_t i = 0; i < vpKFs.size(); i++) {                                   // SE3 pose recovering, :1575-1587: [sR t; 0 1] -> [R t/s; 0 1]
            KeyFrameT *pKFi = vpKFs[i];
            const int v = vertex(pKFi);
            if (v < 0) continue;
            const double *S = &g.S[8 * (size_t)v];
            eg_inv(S, &vCorrectedSwc[8 * (size_t)v]);
            const float s = (float)S[7];
            pKFi->SetPose(Sophus::SE3f(Eigen::Quaternionf((float)S[3], (float)S[0], (float)S[1], (float)S[2]),
                                       Eigen::Vector3f((float)S[4] / s, (float)S[5] / s, (float)S[6] / s)));
        }
        std::vector<float> X;                                                          // correct points, :1590-1619
        std::vector<int32_t> ref;
        std::vector<size_t> which;
        for (size_t i = 0; i < vpMPs.size(); i++) {
            auto *pMP = vpMPs[i];
            if (pMP->isBad()) continue;
            long nIDr;
            if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = (long)pMP->mnCorrectedReference;
            else {
                KeyFrameT *pRefKF = pMP->GetReferenceKeyFrame();
                if (!pRefKF) continue;
                nIDr = (long)pRefKF->mnId;
            }
            const auto f = vertexOf.find((unsigned long)nIDr);
            if (f == vertexOf.end()) continue;
            const auto P = pMP->GetWorldPos();
            X.push_back(P(0)); X.push_back(P(1)); X.push_back(P(2));
            ref.push_back(f->second); which.push_back(i);
        }
        if (!which.empty()) {
            if (RUMI_GUARDED("Optimizer / rumi_sim3_correct_points", &Optimizer::grow_arena, rumi_sim3_correct_points(arena(), 0, (int32_t)which.size(), X.data(), ref.data(), nV, vScw.data(), vCorrectedSwc.data())) != RUMI_OK) return;
            for (size_t k = 0; k < which.size(); k++) {
                auto *pMP = vpMPs[which[k]];
                pMP->SetWorldPos(Eigen::Vector3f(X[3 * k], X[3 * k + 1], X[3 * k + 2]));
                pMP->UpdateNormalAndDepth();
            }
        }
        pMap->IncreaseChangeIndex();
    }

    // void static OptimizeEssentialGraph(KeyFrame *pCurKF, vector<KeyFrame *> &vpFixedKFs, vector<KeyFrame *> &vpFixedCorrectedKFs,
    //                                    vector<KeyFrame *> &vpNonFixedKFs, vector<MapPoint *> &vpNonCorrectedMPs)      Optimizer.cc:1625-1918
    // Three vertex groups (:1654-1746): fixed (good pose, _fix_scale), fixed and corrected (good and bad pose: the estimate is the corrected pose,
    // vScw the one before the merge), free (bad pose).  An edge exists where both ends have a good pose (measured from the corrected poses)
    // or else both a bad one (from the poses before the merge) (:1757-1859).  A key-frame listed twice is visited twice, as upstream.
    template <class KeyFrameT, class MapPointT>
    static void OptimizeEssentialGraph(KeyFrameT *pCurKF, std::vector<KeyFrameT *> &vpFixedKFs, std::vector<KeyFrameT *> &vpFixedCorrectedKFs,
                                       std::vector<KeyFrameT *> &vpNonFixedKFs, std::vector<MapPointT *> &vpNonCorrectedMPs) {
        auto *pMap = pCurKF->GetMap();
        const int minFeat = 100;
        EssentialGraphFlat g;
        std::map<unsigned long, int> vertexOf;
        std::vector<double> vScw, vCorrectedSwc;                                       // by vertex; a default g2o::Sim3 where upstream never assigns
        std::vector<uint8_t> good, bad;
        auto push = [&](KeyFrameT *pKFi, const double *Siw, bool fix, bool fs, const double *Scw, const double *Swc, bool isGood, bool isBad) {
            vertexOf[pKFi->mnId] = g.add_vertex(pKFi->mnId, Siw, fix, fs);
            double I[8];
            eg_identity(I);
            vScw.insert(vScw.end(), Scw ? Scw : I, (Scw ? Scw : I) + 8);
            vCorrectedSwc.insert(vCorrectedSwc.end(), Swc ? Swc : I, (Swc ? Swc : I) + 8);
            good.push_back(isGood); bad.push_back(isBad);
        };
        for (KeyFrameT *pKFi : vpFixedKFs) {
            if (pKFi->isBad()) continue;
            double Siw[8], Swi[8];
            eg_from_pose(pKFi->GetPose(), Siw); eg_inv(Siw, Swi);
            push(pKFi, Siw, true, true, nullptr, Swi, true, false);
        }
        std::set<unsigned long> sIdKF;
        for (KeyFrameT *pKFi : vpFixedCorrectedKFs) {
            if (pKFi->isBad()) continue;
            double Siw[8], Swi[8], Sbef[8];
            eg_from_pose(pKFi->GetPose(), Siw); eg_inv(Siw, Swi); eg_from_pose(pKFi->mTcwBefMerge, Sbef);
            push(pKFi, Siw, true, false, Sbef, Swi, true, true);
            sIdKF.insert(pKFi->mnId);
        }
        for (KeyFrameT *pKFi : vpNonFixedKFs) {
            if (pKFi->isBad()) continue;
            if (sIdKF.count(pKFi->mnId)) continue;
            double Siw[8];
            eg_from_pose(pKFi->GetPose(), Siw);
            push(pKFi, Siw, false, false, Siw, nullptr, false, true);
            sIdKF.insert(pKFi->mnId);
        }
        std::vector<KeyFrameT *> vpKFs;
        vpKFs.insert(vpKFs.end(), vpFixedKFs.begin(), vpFixedKFs.end());
        vpKFs.insert(vpKFs.end(), vpFixedCorrectedKFs.begin(), vpFixedCorrectedKFs.end());
        vpKFs.insert(vpKFs.end(), vpNonFixedKFs.begin(), vpNonFixedKFs.end());
        const std::set<KeyFrameT *> spKFs(vpKFs.begin(), vpKFs.end());
        auto vertex = [&](KeyFrameT *p) { const auto f = vertexOf.find(p->mnId); return f == vertexOf.end() ? -1 : f->second; };
        // the relation rule of :1772-1779 and its two repeats: the other end's pose as the measurement takes it, or false
        auto relation = [&](int vi, int vj, double *Sjw) {
            if (good[vi] && good[vj]) { eg_inv(&vCorrectedSwc[8 * (size_t)vj], Sjw); return true; }
            if (bad[vi] && bad[vj]) { for (int k = 0; k < 8; k++) Sjw[k] = vScw[8 * (size_t)vj + k]; return true; }
            return false;
        };
        for (KeyFrameT *pKFi : vpKFs) {
            const int vi = vertex(pKFi);
            if (vi < 0) continue;
            double Swi[8], Sjw[8], Sji[8];
            eg_identity(Swi);
            if (bad[vi]) eg_inv(&vScw[8 * (size_t)vi], Swi);
            KeyFrameT *pParentKFi = pKFi->GetParent();
            if (pParentKFi && spKFs.find(pParentKFi) != spKFs.end() && vertex(pParentKFi) >= 0) {
                const int vj = vertex(pParentKFi);
                if (relation(vi, vj, Sjw)) { eg_mul(Sjw, Swi, Sji); g.add_edge(vi, vj, Sji); }
            }
            const auto sLoopEdges = pKFi->GetLoopEdges();
            for (auto sit = sLoopEdges.begin(); sit != sLoopEdges.end(); ++sit) {
                KeyFrameT *pLKF = *sit;
                if (spKFs.find(pLKF) != spKFs.end() && pLKF->mnId < pKFi->mnId && vertex(pLKF) >= 0) {
                    const int vl = vertex(pLKF);
                    if (relation(vi, vl, Sjw)) { eg_mul(Sjw, Swi, Sji); g.add_edge(vi, vl, Sji); }
                }
            }
            const auto vpConnectedKFs = pKFi->GetCovisiblesByWeight(minFeat);
            for (auto vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); ++vit) {
                KeyFrameT *pKFn = *vit;
                if (pKFn && pKFn != pParentKFi && !pKFi->hasChild(pKFn) && !sLoopEdges.count(pKFn) && spKFs.find(pKFn) != spKFs.end()) {
                    if (!pKFn->isBad() && pKFn->mnId < pKFi->mnId && vertex(pKFn) >= 0) {
                        const int vn = vertex(pKFn);
                        if (relation(vi, vn, Sjw)) { eg_mul(Sjw, Swi, Sji); g.add_edge(vi, vn, Sji); }
                    }
                }
            }
        }
        if (!eg_solve(g, "Optimizer / rumi_essential_graph (merge)")) return;
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
        for (KeyFrameT *pKFi : vpNonFixedKFs) {                                        // :1873-1888
            if (pKFi->isBad()) continue;
            const int v = vertex(pKFi);
            if (v < 0) continue;
            const double *S = &g.S[8 * (size_t)v], s = S[7];
            pKFi->mTcwBefMerge = pKFi->GetPose();
            pKFi->mTwcBefMerge = pKFi->GetPoseInverse();
            pKFi->SetPose(Sophus::SE3f(Eigen::Quaternionf((float)S[3], (float)S[0], (float)S[1], (float)S[2]),
                                       Eigen::Vector3f((float)(S[4] / s), (float)(S[5] / s), (float)(S[6] / s))));
        }
        const int nV = (int)g.id.size();
        std::vector<float> tabA((size_t)nV * 7, 0.f), tabB((size_t)nV * 7, 0.f), X;
        for (int v = 0; v < nV; v++) tabA[7 * (size_t)v + 3] = tabB[7 * (size_t)v + 3] = 1.f;
        std::vector<uint8_t> tabSet((size_t)nV, 0);
        std::vector<int32_t> ref;
        std::vector<size_t> which;
        bool foreign = false;
        for (size_t i = 0; i < vpNonCorrectedMPs.size(); i++) {                       // :1891-1916
            MapPointT *pMPi = vpNonCorrectedMPs[i];
            if (pMPi->isBad()) continue;
            KeyFrameT *pRefKF = pMPi->GetReferenceKeyFrame();
            while (pRefKF && pRefKF->isBad()) { pMPi->EraseObservation(pRefKF); pRefKF = pMPi->GetReferenceKeyFrame(); }
            if (!pRefKF) continue;
            const int v = vertex(pRefKF);
            if (v < 0 || !bad[v]) { foreign = true; continue; }                        // "MapPoint has a reference KF from another map"
            if (!tabSet[v]) { eg_pose7(pRefKF->GetPoseInverse(), &tabA[7 * (size_t)v]); eg_pose7(pRefKF->mTwcBefMerge, &tabB[7 * (size_t)v]); tabSet[v] = 1; }
            const auto P = pMPi->GetWorldPos();
            X.push_back(P(0)); X.push_back(P(1)); X.push_back(P(2));
            ref.push_back(v); which.push_back(i);
        }
        if (foreign) std::fprintf(stderr, "[rumi] Optimizer::OptimizeEssentialGraph: map points whose reference key-frame has no pose from before the merge were left alone\n");
        if (which.empty()) return;
        if (RUMI_GUARDED("Optimizer / rumi_sim3_correct_points (merge)", &Optimizer::grow_arena, rumi_sim3_correct_points(arena(), 1, (int32_t)which.size(), X.data(), ref.data(), nV, tabA.data(), tabB.data())) != RUMI_OK) return;
        for (size_t k = 0; k < which.size(); k++) {
            MapPointT *pMPi = vpNonCorrectedMPs[which[k]];
            pMPi->SetWorldPos(Eigen::Vector3f(X[3 * k], X[3 * k + 1], X[3 * k + 2]));
            pMPi->UpdateNormalAndDepth();
        }
    }
#endif
};

}  // namespace RUMI_FACADE_NAMESPACE
