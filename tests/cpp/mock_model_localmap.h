// The data model rumi_facade::TrackLocalMapResident (facade/TrackingStep.h) and CovisibilityGraph (facade/CovisibilityGraph.h) touch together,
// with the reference's member names: the covisibility members of mock_model_covis.h and the tracking members of test_facade.cc's mock in one
// set of types.  TEST INFRASTRUCTURE.
#pragma once
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "cv_shim.h"

struct V3f { float v[3]; float operator()(int i) const { return v[i]; } };
struct Q4f { float q[4]; float x() const { return q[0]; } float y() const { return q[1]; } float z() const { return q[2]; } float w() const { return q[3]; } };
struct SE3f { float T[7]; Q4f unit_quaternion() const { return Q4f{{T[0], T[1], T[2], T[3]}}; } V3f translation() const { return V3f{{T[4], T[5], T[6]}}; } };

struct KeyFrame;
struct MapPoint {
    long unsigned int mnId = 0, mnTrackReferenceForFrame = 0;
    bool bad = false;
    std::map<KeyFrame *, std::tuple<int, int>> mObservations;
    V3f pos{{0, 0, 1}}, normal{{0, 0, 1}};
    cv::Mat desc;
    float minD = 0.5f, maxD = 60.f;
    bool mbTrackInView = false, mbTrackInViewR = false;
    float mTrackProjX = 0, mTrackProjY = 0, mTrackViewCos = 1, mTrackDepth = 1;
    int mnTrackScaleLevel = 0;
    long unsigned int mnLastFrameSeen = 0;
    int nVisible = 0, nFound = 0;
    bool isBad() { return bad; }
    std::map<KeyFrame *, std::tuple<int, int>> GetObservations() { return mObservations; }
    int Observations() { return (int)mObservations.size(); }
    V3f GetWorldPos() { return pos; }
    V3f GetNormal() { return normal; }
    cv::Mat GetDescriptor() { return desc; }
    float GetMinDistance() { return minD; }
    float GetMaxDistance() { return maxD; }
    void SetWorldPosXYZ(float x, float y, float z) { pos = V3f{{x, y, z}}; }
    void IncreaseVisible() { nVisible++; }
    void IncreaseFound() { nFound++; }
};
struct Map {
    long unsigned int mnId = 0, mnInitKFid = 0;
    long unsigned int GetId() { return mnId; }
    long unsigned int GetInitKFid() { return mnInitKFid; }
};
struct KeyFrame {
    long unsigned int mnId = 0, mnTrackReferenceForFrame = 0;
    bool bad = false;
    Map *mpMap = nullptr;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    KeyFrame *mpParent = nullptr;
    std::set<KeyFrame *> mspChildrens;
    bool isBad() { return bad; }
    Map *GetMap() { return mpMap; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    KeyFrame *GetParent() { return mpParent; }
    std::set<KeyFrame *> GetChilds() { return mspChildrens; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    // (UpdateConnections is not exercised here; the three members it needs exist so that the class template instantiates)
    void AddConnection(KeyFrame *, const int &) {}
    void SetCovisibility(const std::map<KeyFrame *, int> &, const std::vector<KeyFrame *> &, const std::vector<int> &) {}
    bool FirstConnection() { return false; }
    void SetFirstParent(KeyFrame *) {}
    double mTimeStamp = 0;
};
struct Frame {
    int N = 0;
    long unsigned int mnId = 7;
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    float fx = 535.4f, fy = 539.2f, cx = 320.1f, cy = 247.6f;
    SE3f pose{{0, 0, 0, 1, 0, 0, 0}};
    KeyFrame *mpReferenceKF = nullptr;
    SE3f GetPose() const { return pose; }
    void SetPoseFromQuatTrans(const float *T7) { std::memcpy(pose.T, T7, 28); }
};
