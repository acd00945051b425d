// The key-frame rumi_facade::ComputeSubmapSim3 (facade/CloudMergingStep.h) reads: the mock data model of mock_model_sophus.h plus what the key-point
// match reads of a key-frame (KeyFrame.h: grid sizes are ints, the inverse cell sizes floats, NLeft == -1 for a monocular key-frame).
#pragma once
#include "mock_model_sophus.h"

struct KeyFrameCM : KeyFrame {
    int mnGridCols = 64, mnGridRows = 48, NLeft = -1;
    float mfGridElementWidthInv = 64.f / 640.f, mfGridElementHeightInv = 48.f / 480.f;
};
