// What LocalMapping::CreateNewMapPoints touches beyond tests/cpp/mock_model_sophus.h: the MapPoint constructor and the two MapPoint members the
// reference calls on a new point, KeyFrame::mfScaleFactor, and an Atlas (the camera's unprojectEig is evaluated on the device, not by the facade).  Same member names as the reference.
#pragma once
#include <list>

#include "mock_model_sophus.h"

struct KeyFrameLM : KeyFrame {
    float mfScaleFactor = 1.2f;
};
struct MapPointLM : MapPoint {
    KeyFrame *mpRefKF = nullptr;
    int nDistinctive = 0, nNormalDepth = 0;
    MapPointLM(const Eigen::Vector3f &Pos, KeyFrame *pRefKF, Map *pMap) : mpRefKF(pRefKF) { pos = Pos; map = pMap; nObs = 0; }     // MapPoint.cc:40-58
    void ComputeDistinctiveDescriptors() { nDistinctive++; }
    void UpdateNormalAndDepth() { nNormalDepth++; }
};
struct Atlas {
    Map current;
    std::vector<MapPoint *> added;
    Map *GetCurrentMap() { return &current; }
    void AddMapPoint(MapPoint *p) { added.push_back(p); }
};
