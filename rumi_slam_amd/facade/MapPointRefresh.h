// MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (R/lib_src/MapPoint.cc:353-427, 450-518) for a list of points
// as ONE device call (include/rumi_mapping.h, rumi_refresh_map_points).  Function templates over the data-model types, like the rest of
// facade/: they compile against the reference's KeyFrame / MapPoint and against the mock types of tests/cpp.
//
// Neither member reads another MapPoint, so the per-point calls at the end of a map-changing loop can be collected and issued after the loop
// with identical results.  In LocalMapping.cc:
//   ProcessNewKeyFrame :291-305    ->  rumi_facade::AssociateAndRefresh(mpCurrentKeyFrame, mlpRecentAddedMapPoints);
//   SearchInNeighbors  :730-739    ->  rumi_facade::RefreshKeyFramePoints(mpCurrentKeyFrame);
//   CreateNewMapPoints             ->  LocalMappingStep::CreateNewMapPoints(..., &created) and rumi_facade::RefreshMapPoints(created)
// MapPoint needs two one-line setters the reference lacks: SetDescriptor(const cv::Mat&) and
// SetDistanceRange(float min, float max); SetNormalVector exists.
#pragma once
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "cv_shim.h"
#include "rumi_mapping.h"
#include "rumi_status.h"

namespace rumi_facade {

// One refresh handle per calling thread (handles are not re-entrant).
inline RumiRefresh *refresh_handle() {
    thread_local RumiRefresh *r = nullptr;
    if (!r) {
        const int rc = rumi_refresh_create(-1, &r);
        if (rc != RUMI_OK) { report("MapPointRefresh: handle", rc); r = nullptr; }
    }
    return r;
}

#ifdef RUMI_HAVE_SOPHUS
// `what` = RUMI_REFRESH_DESCRIPTOR | RUMI_REFRESH_NORMAL_DEPTH (both by default).  NULL and isBad() points are skipped, as both members
// return at once for them (:362, :458).  Returns the number of points refreshed, -1 when nothing was written: the device call failed, or an
// observation is a stereo one (right index != -1, or a key-frame with NLeft != -1) -- only the monocular branches are built; both are
// reported through rumi_status.h.
template <class MapPointT> int RefreshMapPoints(const std::vector<MapPointT *> &vpMPs, int what = RUMI_REFRESH_DESCRIPTOR | RUMI_REFRESH_NORMAL_DEPTH) {
    using ObsT = decltype(std::declval<MapPointT &>().GetObservations());
    using KFPtr = typename ObsT::key_type;
    std::vector<MapPointT *> live;
    std::vector<KFPtr> kfs;
    std::unordered_map<const void *, int32_t> kfIndex;
    std::vector<RumiRefreshPoint> pts;
    std::vector<int32_t> obsKf, obsFeature;
    auto index_of = [&](KFPtr pKF) {
        auto it = kfIndex.find(pKF);
        if (it != kfIndex.end()) return it->second;
        kfs.push_back(pKF);
        return kfIndex[pKF] = (int32_t)kfs.size() - 1;
    };
    for (MapPointT *pMP : vpMPs) {
        if (!pMP || pMP->isBad()) continue;
        const ObsT observations = pMP->GetObservations();        // std::map: the order both members iterate in
        KFPtr pRefKF = pMP->GetReferenceKeyFrame();
        const Eigen::Vector3f Pos = pMP->GetWorldPos();
        RumiRefreshPoint P;
        for (int c = 0; c < 3; c++) P.pos[c] = Pos(c);
        P.obs_begin = (int32_t)obsKf.size();
        P.ref_kf = 0; P.ref_feature = 0; P.ref_level = 0;
        for (const auto &o : observations) {
            const int leftIndex = std::get<0>(o.second), rightIndex = std::get<1>(o.second);
            if (rightIndex != -1 || leftIndex == -1 || o.first->NLeft != -1) {
                report("MapPointRefresh::RefreshMapPoints", RUMI_E_INVALID, "a stereo observation (right index or NLeft != -1): only the monocular branches are built; no point was refreshed");
                return -1;
            }
            obsKf.push_back(index_of(o.first));
            obsFeature.push_back(leftIndex);
            if (o.first == pRefKF) P.ref_feature = leftIndex;
        }
        P.obs_end = (int32_t)obsKf.size();
        if (P.obs_end > P.obs_begin) {
            if (pRefKF->NLeft != -1) {
                report("MapPointRefresh::RefreshMapPoints", RUMI_E_INVALID, "a stereo reference key-frame (NLeft != -1): only the monocular branches are built; no point was refreshed");
                return -1;
            }
            // `observations[pRefKF]` (:495) on the member's copy inserts a default entry when the reference key-frame does not observe the
            // point; with NLeft == -1 the level is then read at index 0 (:498-499), which is what ref_feature = 0 asks for
            P.ref_kf = index_of(pRefKF);
            P.ref_level = pRefKF->mvKeysUn[P.ref_feature].octave;   // :499
        }
        pts.push_back(P);
        live.push_back(pMP);
    }
    const int n = (int)pts.size();
    if (n == 0) return 0;
    std::vector<RumiRefreshKF> table(kfs.size());
    for (size_t k = 0; k < kfs.size(); k++) {
        KFPtr pKF = kfs[k];
        RumiRefreshKF &o = table[k];
        o.desc = pKF->mDescriptors.ptr(0); o.n = pKF->N;
        o.nlevels = pKF->mnScaleLevels; o.scale_factors = pKF->mvScaleFactors.data();
        const Eigen::Vector3f Ow = pKF->GetCameraCenter();
        for (int c = 0; c < 3; c++) o.Ow[c] = Ow(c);
        o.is_bad = pKF->isBad();
        o.pad_[0] = o.pad_[1] = o.pad_[2] = 0;
    }
    std::vector<int32_t> bestObs(n), bestMedian(n);
    std::vector<float> normal((size_t)n * 3), minD(n), maxD(n);
    std::vector<uint8_t> updated(n);
    RumiRefresh *h = refresh_handle();
    if (!h) return -1;
    if (RUMI_GUARDED("MapPointRefresh / rumi_refresh_map_points", &no_growth,
                     rumi_refresh_map_points(h, table.data(), (int32_t)table.size(), pts.data(), n, obsKf.data(), obsFeature.data(), (int32_t)obsKf.size(),
                                             what, bestObs.data(), bestMedian.data(), normal.data(), minD.data(), maxD.data(), updated.data())) != RUMI_OK)
        return -1;
    for (int i = 0; i < n; i++) {
        MapPointT *pMP = live[i];
        if ((what & RUMI_REFRESH_DESCRIPTOR) && bestObs[i] >= 0) {                       // :425
            const int o = pts[i].obs_begin + bestObs[i];
            pMP->SetDescriptor(kfs[obsKf[o]]->mDescriptors.row(obsFeature[o]).clone());
        }
        if ((what & RUMI_REFRESH_NORMAL_DEPTH) && updated[i]) {                          // :512-517
            pMP->SetDistanceRange(minD[i], maxD[i]);
            pMP->SetNormalVector(Eigen::Vector3f(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]));
        }
    }
    return n;
}

// LocalMapping::ProcessNewKeyFrame, the association loop (LocalMapping.cc:291-305): AddObservation for every matched point first, then one
// refresh of those points.  Returns RefreshMapPoints' value.
template <class KeyFrameT, class RecentListT> int AssociateAndRefresh(KeyFrameT *pCurrentKF, RecentListT &mlpRecentAddedMapPoints) {
    const auto vpMapPointMatches = pCurrentKF->GetMapPointMatches();
    std::vector<typename std::decay<decltype(vpMapPointMatches)>::type::value_type> touched;
    for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
        auto pMP = vpMapPointMatches[i];
        if (!pMP || pMP->isBad()) continue;
        if (!pMP->IsInKeyFrame(pCurrentKF)) { pMP->AddObservation(pCurrentKF, (int)i); touched.push_back(pMP); }
        else mlpRecentAddedMapPoints.push_back(pMP);             // new stereo points inserted by the Tracking (:299-302)
    }
    return RefreshMapPoints(touched);
}

// LocalMapping::SearchInNeighbors, the "Update points" loop (LocalMapping.cc:730-739).
template <class KeyFrameT> int RefreshKeyFramePoints(KeyFrameT *pCurrentKF) {
    return RefreshMapPoints(pCurrentKF->GetMapPointMatches());
}
// The same refresh over a CovisibilityGraph that holds the map (rumi_refresh_map_points_resident): the points go to the device as ids, the
// observer rows, descriptors, centres, positions and reference key-frames are read where the store keeps them, and the write-back leaves the
// store's attribute records current, so that a later TrackLocalMapResident / SearchInNeighborsResident / CreateNewMapPointsResident needs no
// SyncAttributes for these points.  The store must be current for them: Sync(MapPoint*) after the observations changed, SyncFeatures of every
// observer, SyncCentres after SetPose, SyncReferences where mpRefKF changed, SyncAttributes (or MarkDirty + FlushDirty) after SetWorldPos
// (INTEGRATION.md).  NULL, isBad() and repeated points are skipped.  Stereo observations are refused as RefreshMapPoints refuses them, with
// nothing written.  Returns the number of points refreshed, -1 when nothing was written.
template <class GraphT, class MapPointT>
int RefreshMapPointsResident(GraphT &graph, const std::vector<MapPointT *> &vpMPs, int what = RUMI_REFRESH_DESCRIPTOR | RUMI_REFRESH_NORMAL_DEPTH) {
    static const char *where = "MapPointRefresh::RefreshMapPointsResident";
    std::vector<MapPointT *> live;
    std::set<MapPointT *> in;
    for (MapPointT *pMP : vpMPs) {
        if (!pMP || pMP->isBad() || !in.insert(pMP).second) continue;
        const auto observations = pMP->GetObservations();
        for (const auto &o : observations)
            if (std::get<1>(o.second) != -1 || std::get<0>(o.second) == -1 || o.first->NLeft != -1) {
                report(where, RUMI_E_INVALID, "a stereo observation (right index or NLeft != -1): only the monocular branches are built; no point was refreshed");
                return -1;
            }
        if (!observations.empty() && pMP->GetReferenceKeyFrame()->NLeft != -1) {
            report(where, RUMI_E_INVALID, "a stereo reference key-frame (NLeft != -1): only the monocular branches are built; no point was refreshed");
            return -1;
        }
        live.push_back(pMP);
    }
    const int n = (int)live.size();
    if (n == 0) return 0;
    std::vector<int32_t> ids(n);
    for (int i = 0; i < n; i++)
        if ((ids[i] = graph.IdOf(live[i])) < 0) return -1;
    std::vector<int32_t> bestObs(n), bestMedian(n);
    std::vector<uint8_t> desc((size_t)n * 32), updated(n);
    std::vector<float> normal((size_t)n * 3), minD(n), maxD(n);
    RumiRefresh *h = refresh_handle();
    if (!h) return -1;
    if (RUMI_GUARDED("MapPointRefresh / rumi_refresh_map_points_resident", &no_growth,
                     rumi_refresh_map_points_resident(h, graph.handle(), ids.data(), n, what, RUMI_REFRESH_WRITE_BACK, bestObs.data(), bestMedian.data(),
                                                      desc.data(), normal.data(), minD.data(), maxD.data(), updated.data())) != RUMI_OK)
        return -1;
    for (int i = 0; i < n; i++) {
        MapPointT *pMP = live[i];
        if ((what & RUMI_REFRESH_DESCRIPTOR) && bestObs[i] >= 0) {                       // :425
            cv::Mat d;
            d.create(1, 32, CV_8U);
            std::memcpy(d.ptr(0), desc.data() + 32 * (size_t)i, 32);
            pMP->SetDescriptor(d);
        }
        if ((what & RUMI_REFRESH_NORMAL_DEPTH) && updated[i]) {                          // :512-517
            pMP->SetDistanceRange(minD[i], maxD[i]);
            pMP->SetNormalVector(Eigen::Vector3f(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]));
        }
    }
    return n;
}

// The association loop of ProcessNewKeyFrame over the graph: every touched point's new observer row is staged, then one resident refresh.
template <class GraphT, class KeyFrameT, class RecentListT> int AssociateAndRefreshResident(GraphT &graph, KeyFrameT *pCurrentKF, RecentListT &mlpRecentAddedMapPoints) {
    const auto vpMapPointMatches = pCurrentKF->GetMapPointMatches();
    std::vector<typename std::decay<decltype(vpMapPointMatches)>::type::value_type> touched;
    for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
        auto pMP = vpMapPointMatches[i];
        if (!pMP || pMP->isBad()) continue;
        if (!pMP->IsInKeyFrame(pCurrentKF)) { pMP->AddObservation(pCurrentKF, (int)i); touched.push_back(pMP); }
        else mlpRecentAddedMapPoints.push_back(pMP);
    }
    for (auto pMP : touched)
        if (graph.Sync(pMP) != RUMI_OK) return -1;
    return RefreshMapPointsResident(graph, touched);
}

// The "Update points" loop of SearchInNeighbors over the graph (the member's Fuse calls have staged what they changed).
template <class GraphT, class KeyFrameT> int RefreshKeyFramePointsResident(GraphT &graph, KeyFrameT *pCurrentKF) {
    return RefreshMapPointsResident(graph, pCurrentKF->GetMapPointMatches());
}
#endif  // RUMI_HAVE_SOPHUS

}  // namespace rumi_facade
