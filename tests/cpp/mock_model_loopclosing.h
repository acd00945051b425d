// What rumi_facade::CommonRegionsBoWStage (facade/LoopClosingStep.h) reads of a key-frame and a map point, with the reference's member names and
// types (KeyFrame.h, MapPoint.h; DBoW2::FeatureVector is a std::map<unsigned, std::vector<unsigned>>).
#pragma once
#include <map>
#include <set>
#include <vector>

#include "cv_shim.h"

struct MapPointLC {
    int id = 0;
    bool bad = false;
    bool isBad() { return bad; }
};
struct KeyFrameLC {
    int id = 0, N = 0, NLeft = -1;
    bool bad = false;
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    std::map<unsigned, std::vector<unsigned>> mFeatVec;
    std::vector<MapPointLC *> mvpMapPoints;
    std::vector<float> mvScaleFactors = std::vector<float>(8, 1.f);
    int mnMinX = 0, mnMinY = 0, mnMaxX = 640, mnMaxY = 480;
    std::vector<KeyFrameLC *> covisibles;                     // ordered, best first
    std::set<KeyFrameLC *> connected;
    bool isBad() { return bad; }
    std::vector<MapPointLC *> GetMapPointMatches() { return mvpMapPoints; }
    std::set<KeyFrameLC *> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrameLC *> GetBestCovisibilityKeyFrames(const int &N_) {
        if ((int)covisibles.size() < N_) return covisibles;
        return std::vector<KeyFrameLC *>(covisibles.begin(), covisibles.begin() + N_);
    }
};
