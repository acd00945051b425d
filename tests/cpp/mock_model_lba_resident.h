// What CovisibilityGraph::SyncPoses / SyncPointMaps (facade/CovisibilityGraph.h) and Optimizer::LocalBundleAdjustmentResident (facade/Optimizer.h)
// touch beyond tests/cpp/mock_model_refresh_resident.h: a map
// with an id of its own, and a map point whose GetMap() is that typed map.  The typed views return the same objects at the same addresses.
#pragma once
#include "mock_model_refresh_resident.h"

struct MapLR : MapRR {
    long unsigned int id = 0;
    long unsigned int GetId() { return id; }
};
struct KeyFrameLR;
struct MapPointLR : MapPointRR {
    MapLR *GetMap() { return static_cast<MapLR *>(map); }
    KeyFrameLR *GetReferenceKeyFrame();
    std::map<KeyFrameLR *, std::tuple<int, int>> GetObservations();
};
struct KeyFrameLR : KeyFrameRR {
    MapLR *GetMap() { return static_cast<MapLR *>(map); }
    std::vector<MapPointLR *> GetMapPointMatches() {
        std::vector<MapPointLR *> v;
        for (MapPoint *p : mvpMapPoints) v.push_back(static_cast<MapPointLR *>(p));
        return v;
    }
    std::vector<KeyFrameLR *> GetVectorCovisibleKeyFrames() {
        std::vector<KeyFrameLR *> v;
        for (KeyFrame *k : covis) v.push_back(static_cast<KeyFrameLR *>(k));
        return v;
    }
    Eigen::Vector3f GetCameraCenter() const { return KeyFrame::GetCameraCenter(); }     // follows SetPose (KeyFrameRF keeps a member of its own)
    std::vector<KeyFrameLR *> GetBestCovisibilityKeyFrames(const int &) { return {}; }
    KeyFrameLR *GetParent() { return nullptr; }
    std::set<KeyFrameLR *> GetChilds() { return {}; }
};
inline KeyFrameLR *MapPointLR::GetReferenceKeyFrame() { return static_cast<KeyFrameLR *>(mpRefKF); }
inline std::map<KeyFrameLR *, std::tuple<int, int>> MapPointLR::GetObservations() {
    std::map<KeyFrameLR *, std::tuple<int, int>> m;
    for (auto &o : obs) m[static_cast<KeyFrameLR *>(o.first)] = o.second;
    return m;
}
