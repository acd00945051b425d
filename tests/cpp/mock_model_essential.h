// Mock data model for Optimizer::OptimizeEssentialGraph (facade/Optimizer.h), both overloads, over tests/cpp/mock_sophus.h: only what the two
// members touch, with the reference's member names -- the spanning tree, loop edges, weighted covisibility, the poses from before a merge and
// the corrected-by fields of the map points.
#pragma once
#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "mock_sophus.h"

struct KeyFrameEG;
struct MapPointEG;
struct MapEG {
    std::mutex mMutexMapUpdate;
    long initId = 0; int changes = 0; unsigned long maxId = 0;
    std::vector<KeyFrameEG *> allKFs; std::vector<MapPointEG *> allMPs;
    long GetInitKFid() { return initId; }
    unsigned long GetMaxKFid() { return maxId; }
    void IncreaseChangeIndex() { changes++; }
    std::vector<KeyFrameEG *> GetAllKeyFrames() { return allKFs; }
    std::vector<MapPointEG *> GetAllMapPoints() { return allMPs; }
};
struct KeyFrameEG {
    unsigned long mnId = 0; MapEG *map = nullptr; bool bad = false, bImu = false;
    KeyFrameEG *mPrevKF = nullptr, *parent = nullptr;
    Sophus::SE3f pose, mTcwBefMerge, mTwcBefMerge;
    std::set<KeyFrameEG *> children, loopEdges;
    std::vector<std::pair<int, KeyFrameEG *>> covis;             // (weight, key-frame), descending weight
    Sophus::SE3f GetPose() const { return pose; }
    Sophus::SE3f GetPoseInverse() const { return pose.inverse(); }
    void SetPose(const Sophus::SE3f &T) { pose = T; }
    bool isBad() { return bad; }
    MapEG *GetMap() { return map; }
    KeyFrameEG *GetParent() { return parent; }
    bool hasChild(KeyFrameEG *p) { return children.count(p) > 0; }
    std::set<KeyFrameEG *> GetLoopEdges() { return loopEdges; }
    std::vector<KeyFrameEG *> GetCovisiblesByWeight(const int &w) {       // KeyFrame.cc: every neighbour of weight >= w, heaviest first
        std::vector<KeyFrameEG *> v;
        for (auto &c : covis) if (c.first >= w) v.push_back(c.second);
        return v;
    }
    int GetWeight(KeyFrameEG *p) { for (auto &c : covis) if (c.second == p) return c.first; return 0; }
};
struct MapPointEG {
    Eigen::Vector3f pos; bool bad = false;
    unsigned long mnCorrectedByKF = 0, mnCorrectedReference = 0;
    KeyFrameEG *ref = nullptr; int nRefresh = 0;
    Eigen::Vector3f GetWorldPos() { return pos; }
    void SetWorldPos(const Eigen::Vector3f &p) { pos = p; }
    bool isBad() { return bad; }
    KeyFrameEG *GetReferenceKeyFrame() { return ref; }
    void EraseObservation(KeyFrameEG *) { ref = nullptr; }
    void UpdateNormalAndDepth() { nRefresh++; }
};
