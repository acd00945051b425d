// What LocalMappingStep::KeyFrameCullingResident and CovisibilityGraph (facade/) touch beyond tests/cpp/mock_model_culling.h: Map::GetId, the
// covisibility / spanning-tree getters (this scene has neither connections nor a tree), the typed views of the base containers (same objects,
// same addresses), and the Sync hooks INTEGRATION.md asks of the mutators: KeyFrame::SetBadFlag, MapPoint::EraseObservation and
// MapPoint::SetBadFlag tell the graph which key-frames and points they changed.  The three members are written as in mock_model_culling.h.
#pragma once
#include <functional>
#include <set>

#include "mock_model_culling.h"

struct KeyFrameKR;
struct MapPointKR;
struct SyncHooks {                                       // empty: a map nobody mirrors (the copy the block member works on)
    std::function<void(KeyFrameKR *)> keyframe;
    std::function<void(MapPointKR *)> point;
    std::function<void(KeyFrameKR *)> drop;
};
struct MapKR : Map {
    SyncHooks hooks;
    long unsigned int GetId() { return 0; }
};
struct MapPointKR : MapPointKC {
    std::map<KeyFrameKR *, std::tuple<int, int>> GetObservations();
    void EraseObservation(KeyFrameKR *pKF);
    void SetBadFlag();
    MapKR *GetMap() { return static_cast<MapKR *>(map); }
};
struct KeyFrameKR : KeyFrameKC {
    std::vector<KeyFrameKR *> covisKR;
    MapKR *GetMap() { return static_cast<MapKR *>(map); }
    std::vector<KeyFrameKR *> GetVectorCovisibleKeyFrames() { return covisKR; }
    std::vector<MapPointKR *> GetMapPointMatches() {
        std::vector<MapPointKR *> v;
        for (MapPoint *p : mvpMapPoints) v.push_back(static_cast<MapPointKR *>(p));
        return v;
    }
    MapPointKR *GetMapPoint(size_t i) { return static_cast<MapPointKR *>(mvpMapPoints[i]); }
    std::vector<KeyFrameKR *> GetBestCovisibilityKeyFrames(const int &) { return {}; }
    KeyFrameKR *GetParent() { return nullptr; }
    std::set<KeyFrameKR *> GetChilds() { return {}; }
    void SetBadFlag() {
        if (mnId == map->GetInitKFid()) return;                            // :781-782
        if (mbNotErase) { mbToBeErased = true; return; }                   // :783-785
        for (size_t i = 0; i < mvpMapPoints.size(); i++)                   // :793-797
            if (mvpMapPoints[i]) static_cast<MapPointKR *>(mvpMapPoints[i])->EraseObservation(this);
        bad = true;                                                        // :861
        if (GetMap()->hooks.keyframe) { GetMap()->hooks.keyframe(this); GetMap()->hooks.drop(this); }
    }
};
inline std::map<KeyFrameKR *, std::tuple<int, int>> MapPointKR::GetObservations() {
    std::map<KeyFrameKR *, std::tuple<int, int>> m;
    for (auto &o : obs) m[static_cast<KeyFrameKR *>(o.first)] = o.second;
    return m;
}
inline void MapPointKR::EraseObservation(KeyFrameKR *pKF) {
    bool bBad = false;
    if (obs.count(pKF)) {                                                  // :197
        nObs--;                                                            // :206
        obs.erase(pKF);                                                    // :212
        if (nObs <= 2) bBad = true;                                        // :218
    }
    if (bBad) SetBadFlag();
    else if (GetMap()->hooks.point) GetMap()->hooks.point(this);
}
inline void MapPointKR::SetBadFlag() {
    bad = true;                                                            // :246
    auto o = obs;
    obs.clear();                                                           // :248
    for (auto &e : o) {                                                    // :250-256
        KeyFrameKR *k = static_cast<KeyFrameKR *>(e.first);
        k->EraseMapPointMatch(std::get<0>(e.second));
        if (GetMap()->hooks.keyframe) GetMap()->hooks.keyframe(k);
    }
    if (GetMap()->hooks.point) GetMap()->hooks.point(this);
}
