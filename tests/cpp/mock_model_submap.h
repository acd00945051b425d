// What rumi_facade::MatchSubmapKeyPoints (facade/CloudMergingStep.h) reads of a key-frame and a map point, with the reference's member names and
// types (KeyFrame.h: mnMinX / mnMinY and the grid sizes are ints, the inverse cell sizes floats).
#pragma once
#include <vector>

#include "cv_shim.h"

struct MapPointSM { int id = 0; };
struct KeyFrameSM {
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<MapPointSM *> mvpMapPoints;
    int mnMinX = 0, mnMinY = 0, mnGridCols = 64, mnGridRows = 48, NLeft = -1;
    float mfGridElementWidthInv = 0.1f, mfGridElementHeightInv = 0.1f;
    std::vector<MapPointSM *> GetMapPointMatches() { return mvpMapPoints; }
};
