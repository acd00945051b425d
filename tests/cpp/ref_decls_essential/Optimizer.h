// The two OptimizeEssentialGraph members of the reference's all-static Optimizer as include/cloud_edge_slam_lib/Optimizer.h declares them
// (signatures only, over the mock data model), for compiling rumi_slam_amd/facade/shells/Optimizer_essential.cc here.
#ifndef OPTIMIZER_H
#define OPTIMIZER_H
#include <map>
#include <set>
#include <vector>

#include "KeyFrame.h"
#include "LoopClosing.h"
#include "Map.h"
#include "MapPoint.h"

namespace ORB_SLAM3 {
using std::map; using std::set; using std::vector;
class Optimizer {
public:
    void static OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3, const map<KeyFrame *, set<KeyFrame *>> &LoopConnections,
                                       const bool &bFixScale);
    void static OptimizeEssentialGraph(KeyFrame *pCurKF, vector<KeyFrame *> &vpFixedKFs, vector<KeyFrame *> &vpFixedCorrectedKFs,
                                       vector<KeyFrame *> &vpNonFixedKFs, vector<MapPoint *> &vpNonCorrectedMPs);
};
}  // namespace ORB_SLAM3
#endif
