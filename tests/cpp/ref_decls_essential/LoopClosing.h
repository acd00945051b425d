// Stand-in for the reference's LoopClosing.h: the one typedef Optimizer::OptimizeEssentialGraph takes (LoopClosing.h:50-51).
#pragma once
#include <map>
#include "KeyFrame.h"
namespace ORB_SLAM3 {
class LoopClosing {
public:
    typedef std::map<KeyFrame *, g2o::Sim3, std::less<KeyFrame *>> KeyFrameAndPose;
};
}  // namespace ORB_SLAM3
