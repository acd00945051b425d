// Stand-in for the reference header of the same name: the mock data model of tests/cpp/mock_model_essential.h, visible as ORB_SLAM3::KeyFrame /
// MapPoint / Map, for compiling rumi_slam_amd/facade/shells/Optimizer_essential.cc.
#pragma once
#include "mock_model_essential.h"
namespace ORB_SLAM3 { using KeyFrame = ::KeyFrameEG; using MapPoint = ::MapPointEG; using Map = ::MapEG; }
