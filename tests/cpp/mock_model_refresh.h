// What rumi_facade::RefreshMapPoints (facade/MapPointRefresh.h) touches beyond tests/cpp/mock_model_sophus.h: a key-frame's NLeft, and a map
// point with a reference key-frame, a real descriptor, normal and distance range, and the setters the write-back uses.  Same member names as
// the reference (SetDescriptor and SetDistanceRange are the two INTEGRATION.md asks a maintainer to add).
#pragma once
#include "mock_model_sophus.h"

struct MapPointRF;
struct KeyFrameRF : KeyFrame {
    int NLeft = -1;
    float mfScaleFactor = 1.2f;
    Eigen::Vector3f Ow;                                               // the scene's camera centre, bit for bit
    Eigen::Vector3f GetCameraCenter() const { return Ow; }
    std::vector<MapPointRF *> GetMapPointMatches();
};
struct MapPointRF : MapPoint {
    KeyFrameRF *mpRefKF = nullptr;
    cv::Mat mDescriptor;
    Eigen::Vector3f mNormalVector;
    float mfMinDistance = -1.f, mfMaxDistance = -1.f;
    int nSetDescriptor = 0, nSetNormal = 0, nSetRange = 0;
    KeyFrameRF *GetReferenceKeyFrame() { return mpRefKF; }
    std::map<KeyFrameRF *, std::tuple<int, int>> GetObservations() {  // the base map's order: same addresses
        std::map<KeyFrameRF *, std::tuple<int, int>> m;
        for (auto &o : obs) m[static_cast<KeyFrameRF *>(o.first)] = o.second;
        return m;
    }
    void SetDescriptor(const cv::Mat &d) { mDescriptor = d; nSetDescriptor++; }
    void SetNormalVector(const Eigen::Vector3f &n) { mNormalVector = n; nSetNormal++; }
    void SetDistanceRange(float mn, float mx) { mfMinDistance = mn; mfMaxDistance = mx; nSetRange++; }
};
inline std::vector<MapPointRF *> KeyFrameRF::GetMapPointMatches() {
    std::vector<MapPointRF *> v;
    for (MapPoint *p : mvpMapPoints) v.push_back(static_cast<MapPointRF *>(p));
    return v;
}
