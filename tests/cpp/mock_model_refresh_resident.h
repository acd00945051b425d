// What rumi_facade::RefreshMapPointsResident (facade/MapPointRefresh.h) and CovisibilityGraph (facade/CovisibilityGraph.h) touch together,
// beyond tests/cpp/mock_model_refresh.h: Map::GetId, the covisibility / spanning-tree getters (this scene has neither connections nor a
// tree), the typed views of the base containers (same objects, same addresses), and the getters SyncAttributes reads, which return the
// members the refresh writes.  Same member names as the reference.
#pragma once
#include <set>

#include "mock_model_refresh.h"

struct KeyFrameRR;
struct MapRR : Map {
    long unsigned int GetId() { return 0; }
};
struct MapPointRR : MapPointRF {
    KeyFrameRR *GetReferenceKeyFrame();
    std::map<KeyFrameRR *, std::tuple<int, int>> GetObservations();
    cv::Mat GetDescriptor() { return mDescriptor; }
    Eigen::Vector3f GetNormal() { return mNormalVector; }
    float GetMinDistance() { return mfMinDistance; }
    float GetMaxDistance() { return mfMaxDistance; }
    bool IsInKeyFrame(KeyFrameRR *k);
    void AddObservation(KeyFrameRR *k, int idx);
};
struct KeyFrameRR : KeyFrameRF {
    MapRR *GetMap() { return static_cast<MapRR *>(map); }
    std::vector<MapPointRR *> GetMapPointMatches() {
        std::vector<MapPointRR *> v;
        for (MapPoint *p : mvpMapPoints) v.push_back(static_cast<MapPointRR *>(p));
        return v;
    }
    std::vector<KeyFrameRR *> GetBestCovisibilityKeyFrames(const int &) { return {}; }
    KeyFrameRR *GetParent() { return nullptr; }
    std::set<KeyFrameRR *> GetChilds() { return {}; }
};
inline KeyFrameRR *MapPointRR::GetReferenceKeyFrame() { return static_cast<KeyFrameRR *>(mpRefKF); }
inline std::map<KeyFrameRR *, std::tuple<int, int>> MapPointRR::GetObservations() {
    std::map<KeyFrameRR *, std::tuple<int, int>> m;
    for (auto &o : obs) m[static_cast<KeyFrameRR *>(o.first)] = o.second;
    return m;
}
inline bool MapPointRR::IsInKeyFrame(KeyFrameRR *k) { return MapPoint::IsInKeyFrame(k); }
inline void MapPointRR::AddObservation(KeyFrameRR *k, int idx) { MapPoint::AddObservation(k, idx); }
