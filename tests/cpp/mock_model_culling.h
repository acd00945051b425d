// What LocalMappingStep::KeyFrameCulling / CloudKeyFrameCulling (facade/LocalMappingStep.h) touch beyond tests/cpp/mock_model_sophus.h: the
// covisible list, isCloud(), mbNotErase behind the getter INTEGRATION.md asks for, and the three members whose side effects the loop carries,
// written as the reference writes them: KeyFrame::SetBadFlag (KeyFrame.cc:778-861, the part that touches points),
// MapPoint::EraseObservation (MapPoint.cc:192-225) and MapPoint::SetBadFlag (:240-263).  Same member names as the reference.
#pragma once
#include "mock_model_sophus.h"

struct KeyFrameKC;
struct MapPointKC : MapPoint {
    std::map<KeyFrameKC *, std::tuple<int, int>> GetObservations();   // the base map's order: same addresses
    void EraseObservation(KeyFrameKC *pKF);
    void SetBadFlag();
};
struct KeyFrameKC : KeyFrame {
    int NLeft = -1;
    bool mbNotErase = false, mbToBeErased = false, mbCloud = false;
    int nUpdateBestCovisibles = 0;
    std::vector<KeyFrameKC *> covisKC;
    void UpdateBestCovisibles() { nUpdateBestCovisibles++; }
    std::vector<KeyFrameKC *> GetVectorCovisibleKeyFrames() { return covisKC; }
    std::vector<MapPointKC *> GetMapPointMatches() {
        std::vector<MapPointKC *> v;
        for (MapPoint *p : mvpMapPoints) v.push_back(static_cast<MapPointKC *>(p));
        return v;
    }
    bool isCloud() { return mbCloud; }
    bool GetNotErase() { return mbNotErase; }
    void EraseMapPointMatch(int idx) { mvpMapPoints[idx] = nullptr; }     // KeyFrame.cc:EraseMapPointMatch(const int &idx)
    void SetBadFlag() {
        if (mnId == map->GetInitKFid()) return;                            // :781-782
        if (mbNotErase) { mbToBeErased = true; return; }                   // :783-785
        for (size_t i = 0; i < mvpMapPoints.size(); i++)                   // :793-797
            if (mvpMapPoints[i]) static_cast<MapPointKC *>(mvpMapPoints[i])->EraseObservation(this);
        bad = true;                                                        // :861
    }
};
inline std::map<KeyFrameKC *, std::tuple<int, int>> MapPointKC::GetObservations() {
    std::map<KeyFrameKC *, std::tuple<int, int>> m;
    for (auto &o : obs) m[static_cast<KeyFrameKC *>(o.first)] = o.second;
    return m;
}
inline void MapPointKC::EraseObservation(KeyFrameKC *pKF) {
    bool bBad = false;
    if (obs.count(pKF)) {                                                  // :197
        nObs--;                                                            // :206
        obs.erase(pKF);                                                    // :212
        if (nObs <= 2) bBad = true;                                        // :218
    }
    if (bBad) SetBadFlag();
}
inline void MapPointKC::SetBadFlag() {
    bad = true;                                                            // :246
    auto o = obs;
    obs.clear();                                                           // :248
    for (auto &e : o) static_cast<KeyFrameKC *>(e.first)->EraseMapPointMatch(std::get<0>(e.second));   // :250-256
}
