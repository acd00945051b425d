// What CovisibilityGraph (facade/CovisibilityGraph.h) asks of the data model beyond tests/cpp/mock_model_newpoints.h, for the resident
// CreateNewMapPoints: Map::GetId, the covisibility / spanning-tree getters (this scene has neither connections nor a tree) and the typed views
// of the base containers (same objects, same addresses).  Same member names as the reference.
#pragma once
#include <cstring>
#include <set>

#include "mock_model_newpoints.h"

struct KeyFrameRS;
struct MapRS : Map {
    long unsigned int GetId() { return 0; }
};
struct MapPointRS : MapPointLM {
    MapPointRS(const Eigen::Vector3f &Pos, KeyFrame *pRefKF, Map *pMap) : MapPointLM(Pos, pRefKF, pMap) {
        desc.create(1, 32, CV_8U);
        std::memset(desc.ptr(0), 0x5A, 32);
    }
    std::map<KeyFrameRS *, std::tuple<int, int>> GetObservations();
};
struct KeyFrameRS : KeyFrameLM {
    MapRS *GetMap() { return static_cast<MapRS *>(map); }
    std::vector<MapPointRS *> GetMapPointMatches() {
        std::vector<MapPointRS *> v;
        for (MapPoint *p : mvpMapPoints) v.push_back(static_cast<MapPointRS *>(p));
        return v;
    }
    std::vector<KeyFrameRS *> GetBestCovisibilityKeyFrames(const int &) { return {}; }
    KeyFrameRS *GetParent() { return nullptr; }
    std::set<KeyFrameRS *> GetChilds() { return {}; }
};
inline std::map<KeyFrameRS *, std::tuple<int, int>> MapPointRS::GetObservations() {
    std::map<KeyFrameRS *, std::tuple<int, int>> m;
    for (auto &o : obs) m[static_cast<KeyFrameRS *>(o.first)] = o.second;
    return m;
}
struct AtlasRS {
    MapRS current;
    std::vector<MapPoint *> added;
    Map *GetCurrentMap() { return &current; }
    void AddMapPoint(MapPoint *p) { added.push_back(p); }
};
