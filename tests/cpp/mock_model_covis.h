// The data model CovisibilityGraph (facade/CovisibilityGraph.h) touches, with the reference's member names, and the members of the reference
// whose side effects the host replay carries, written as the reference writes them: KeyFrame::AddConnection (KeyFrame.cc:328-340),
// UpdateBestCovisibles (:342-361), GetBestCovisibilityKeyFrames (:376-382), AddChild (:672-675).  SetCovisibility, FirstConnection and
// SetFirstParent are the three small members INTEGRATION.md asks the reference's KeyFrame to grow.  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include <list>
#include <map>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

struct KeyFrame;
struct MapPoint {
    long unsigned int mnId = 0, mnTrackReferenceForFrame = 0;
    bool bad = false;
    std::map<KeyFrame *, std::tuple<int, int>> mObservations;
    bool isBad() { return bad; }
    std::map<KeyFrame *, std::tuple<int, int>> GetObservations() { return mObservations; }
};
struct Map {
    long unsigned int mnId = 0, mnInitKFid = 0;
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> mps;
    long unsigned int GetId() { return mnId; }
    long unsigned int GetInitKFid() { return mnInitKFid; }
    std::vector<KeyFrame *> GetAllKeyFrames() { return kfs; }
    std::vector<MapPoint *> GetAllMapPoints() { return mps; }
};
struct KeyFrame {
    long unsigned int mnId = 0, mnTrackReferenceForFrame = 0;
    double mTimeStamp = 0;
    bool bad = false, mbFirstConnection = true;
    Map *mpMap = nullptr;
    std::vector<MapPoint *> mvpMapPoints;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    KeyFrame *mpParent = nullptr;
    std::set<KeyFrame *> mspChildrens;

    bool isBad() { return bad; }
    Map *GetMap() { return mpMap; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    KeyFrame *GetParent() { return mpParent; }
    std::set<KeyFrame *> GetChilds() { return mspChildrens; }
    void AddChild(KeyFrame *pKF) { mspChildrens.insert(pKF); }
    void AddConnection(KeyFrame *pKF, const int &weight) {
        if (!mConnectedKeyFrameWeights.count(pKF)) mConnectedKeyFrameWeights[pKF] = weight;
        else if (mConnectedKeyFrameWeights[pKF] != weight) mConnectedKeyFrameWeights[pKF] = weight;
        else return;
        UpdateBestCovisibles();
    }
    void UpdateBestCovisibles() {
        std::vector<std::pair<int, KeyFrame *>> vPairs;
        for (auto &e : mConnectedKeyFrameWeights) vPairs.push_back(std::make_pair(e.second, e.first));
        std::sort(vPairs.begin(), vPairs.end());
        std::list<KeyFrame *> lKFs;
        std::list<int> lWs;
        for (size_t i = 0; i < vPairs.size(); i++)
            if (!vPairs[i].second->isBad()) { lKFs.push_front(vPairs[i].second); lWs.push_front(vPairs[i].first); }
        mvpOrderedConnectedKeyFrames = std::vector<KeyFrame *>(lKFs.begin(), lKFs.end());
        mvOrderedWeights = std::vector<int>(lWs.begin(), lWs.end());
    }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    // ---- what INTEGRATION.md asks for
    void SetCovisibility(const std::map<KeyFrame *, int> &w, const std::vector<KeyFrame *> &kfs, const std::vector<int> &ws) {
        mConnectedKeyFrameWeights = w; mvpOrderedConnectedKeyFrames = kfs; mvOrderedWeights = ws;
    }
    bool FirstConnection() { return mbFirstConnection; }
    void SetFirstParent(KeyFrame *p) { mpParent = p; p->AddChild(this); mbFirstConnection = false; }
};
struct Frame {
    long unsigned int mnId = 0;
    int N = 0;
    std::vector<MapPoint *> mvpMapPoints;
    KeyFrame *mpReferenceKF = nullptr;
};
