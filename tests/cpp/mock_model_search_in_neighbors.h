// What LocalMappingStep::SearchInNeighborsResident (facade/LocalMappingStep.h) touches beyond tests/cpp/mock_model_culling_resident.h, with the
// reference's member names: the fuse stamps, the covisibility members CovisibilityGraph::UpdateConnections replays (as
// tests/cpp/mock_model_covis.h has them) and KeyFrame::UpdateConnections itself for the map that takes the reference's member text
// (KeyFrame.cc:487-574); of MapPoint the members ORBmatcher::Fuse calls, written as the reference writes them -- Replace (MapPoint.cc:272-326)
// with the ComputeDistinctiveDescriptors (:353-427) it ends with -- and what MapPointRefresh.h writes back.  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include <list>

#include "mock_model_culling_resident.h"
#include "rumi_match.h"

struct KeyFrameSN;
struct MapPointSN : MapPointKR {
    KeyFrameSN *mpRefKF = nullptr;
    MapPointSN *mpReplaced = nullptr;
    long mnFuseCandidateForKF = -1;
    int nDistinctive = 0;
    KeyFrameSN *GetReferenceKeyFrame() { return mpRefKF; }
    std::map<KeyFrameSN *, std::tuple<int, int>> GetObservations();
    void SetDescriptor(const cv::Mat &d) { desc = d; }
    void SetNormalVector(const Eigen::Vector3f &n) { normal = n; }
    void SetDistanceRange(float mn, float mx) { minD = mn; maxD = mx; }
    void AddObservation(KeyFrame *k, int idx) { if (obs.count(k)) return; obs[k] = std::make_tuple(idx, -1); nObs++; }   // MapPoint.cc:160-190, mono
    void ComputeDistinctiveDescriptors();
    void Replace(MapPointSN *pMP);
};
struct KeyFrameSN : KeyFrameKR {
    long mnFuseTargetForKF = -1;
    double mTimeStamp = 0;
    bool mbFirstConnection = true;
    std::map<KeyFrameSN *, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrameSN *> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    KeyFrameSN *mpParent = nullptr;
    std::set<KeyFrameSN *> mspChildrens;
    std::vector<MapPointSN *> GetMapPointMatches() {
        std::vector<MapPointSN *> v;
        for (MapPoint *p : mvpMapPoints) v.push_back(static_cast<MapPointSN *>(p));
        return v;
    }
    MapPointSN *GetMapPoint(size_t i) { return static_cast<MapPointSN *>(mvpMapPoints[i]); }
    void ReplaceMapPointMatch(int idx, MapPointSN *p) { mvpMapPoints[idx] = p; }
    KeyFrameSN *GetParent() { return mpParent; }
    std::set<KeyFrameSN *> GetChilds() { return mspChildrens; }
    void AddChild(KeyFrameSN *pKF) { mspChildrens.insert(pKF); }
    void AddConnection(KeyFrameSN *pKF, const int &weight) {               // KeyFrame.cc:328-340
        if (!mConnectedKeyFrameWeights.count(pKF)) mConnectedKeyFrameWeights[pKF] = weight;
        else if (mConnectedKeyFrameWeights[pKF] != weight) mConnectedKeyFrameWeights[pKF] = weight;
        else return;
        UpdateBestCovisibles();
    }
    void UpdateBestCovisibles() {                                          // :342-361
        std::vector<std::pair<int, KeyFrameSN *>> vPairs;
        for (auto &e : mConnectedKeyFrameWeights) vPairs.push_back(std::make_pair(e.second, e.first));
        std::sort(vPairs.begin(), vPairs.end());
        std::list<KeyFrameSN *> lKFs;
        std::list<int> lWs;
        for (size_t i = 0; i < vPairs.size(); i++)
            if (!vPairs[i].second->isBad()) { lKFs.push_front(vPairs[i].second); lWs.push_front(vPairs[i].first); }
        mvpOrderedConnectedKeyFrames = std::vector<KeyFrameSN *>(lKFs.begin(), lKFs.end());
        mvOrderedWeights = std::vector<int>(lWs.begin(), lWs.end());
    }
    std::vector<KeyFrameSN *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<KeyFrameSN *> GetBestCovisibilityKeyFrames(const int &N) {  // :376-382
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrameSN *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    void SetCovisibility(const std::map<KeyFrameSN *, int> &w, const std::vector<KeyFrameSN *> &kfs, const std::vector<int> &ws) {
        mConnectedKeyFrameWeights = w; mvpOrderedConnectedKeyFrames = kfs; mvOrderedWeights = ws;
    }
    bool FirstConnection() { return mbFirstConnection; }
    void SetFirstParent(KeyFrameSN *p) { mpParent = p; p->AddChild(this); mbFirstConnection = false; }
    void UpdateConnections() {                                             // :487-574, for the map that runs the reference's member text
        std::map<KeyFrameSN *, int> KFcounter;
        for (MapPointSN *pMP : GetMapPointMatches()) {
            if (!pMP || pMP->isBad()) continue;
            for (auto &o : pMP->GetObservations()) {
                if (o.first->mnId == mnId || o.first->isBad() || o.first->GetMap() != GetMap()) continue;
                KFcounter[o.first]++;
            }
        }
        if (KFcounter.empty()) return;
        int nmax = 0;
        KeyFrameSN *pKFmax = nullptr;
        const int th = 15;
        std::vector<std::pair<int, KeyFrameSN *>> vPairs;
        for (auto &e : KFcounter) {
            if (e.second > nmax) { nmax = e.second; pKFmax = e.first; }
            if (e.second >= th) { vPairs.push_back(std::make_pair(e.second, e.first)); e.first->AddConnection(this, e.second); }
        }
        if (vPairs.empty()) { vPairs.push_back(std::make_pair(nmax, pKFmax)); pKFmax->AddConnection(this, nmax); }
        std::sort(vPairs.begin(), vPairs.end());
        std::list<KeyFrameSN *> lKFs;
        std::list<int> lWs;
        for (size_t i = 0; i < vPairs.size(); i++) { lKFs.push_front(vPairs[i].second); lWs.push_front(vPairs[i].first); }
        mConnectedKeyFrameWeights = KFcounter;
        mvpOrderedConnectedKeyFrames = std::vector<KeyFrameSN *>(lKFs.begin(), lKFs.end());
        mvOrderedWeights = std::vector<int>(lWs.begin(), lWs.end());
        if (mbFirstConnection && mnId != GetMap()->GetInitKFid()) { mpParent = mvpOrderedConnectedKeyFrames.front(); mpParent->AddChild(this); mbFirstConnection = false; }
    }
};
inline std::map<KeyFrameSN *, std::tuple<int, int>> MapPointSN::GetObservations() {
    std::map<KeyFrameSN *, std::tuple<int, int>> m;
    for (auto &o : obs) m[static_cast<KeyFrameSN *>(o.first)] = o.second;
    return m;
}
inline void MapPointSN::ComputeDistinctiveDescriptors() {
    nDistinctive++;
    std::vector<const uint8_t *> rows;
    std::vector<cv::Mat> keep;
    if (bad) return;                                                       // :362
    for (auto &o : GetObservations())
        if (!o.first->isBad()) { keep.push_back(o.first->mDescriptors.row(std::get<0>(o.second))); rows.push_back(keep.back().ptr(0)); }
    if (rows.empty()) return;
    const size_t N = rows.size();
    int BestMedian = INT_MAX, BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(N);
        for (size_t j = 0; j < N; j++) vDists[j] = i == j ? 0 : rumi_descriptor_distance(rows[i], rows[j]);
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t)(0.5 * (N - 1))];
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
    }
    desc = keep[BestIdx].clone();
}
inline void MapPointSN::Replace(MapPointSN *pMP) {
    if (pMP == this) return;
    auto o = GetObservations();
    obs.clear();
    bad = true;
    mpReplaced = pMP;
    for (auto &e : o) {
        KeyFrameSN *pKF = e.first;
        const int leftIndex = std::get<0>(e.second);
        if (!pMP->IsInKeyFrame(pKF)) { pKF->ReplaceMapPointMatch(leftIndex, pMP); pMP->AddObservation(pKF, leftIndex); }
        else pKF->EraseMapPointMatch(leftIndex);
    }
    pMP->ComputeDistinctiveDescriptors();
}
