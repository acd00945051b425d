// Definitions of the two Optimizer::OptimizeEssentialGraph members of the reference (include/cloud_edge_slam_lib/Optimizer.h), with the
// reference's exact signatures, each a forward to the MI355X facade templates (../Optimizer.h).  Build this file NEXT TO lib_src/Optimizer.cc
// and Optimizer_hot.cc, and remove (or put under #ifndef RUMI_HIP) the reference's own definitions of
//   OptimizeEssentialGraph (Map *, ...) (:1357-1623) and OptimizeEssentialGraph (KeyFrame *pCurKF, ...) (:1625-1918).
// OptimizeEssentialGraph4DoF and the inertial members stay with the reference.  Compile with -DRUMI_HAVE_SOPHUS, as the other Sophus-typed facades.
#include "Optimizer.h"           // the REFERENCE's header

#include "KeyFrame.h"
#include "LoopClosing.h"
#include "Map.h"
#include "MapPoint.h"

#ifndef RUMI_FACADE_NAMESPACE
#define RUMI_FACADE_NAMESPACE rumi_facade_impl
#endif
#include "../Optimizer.h"        // the facade templates (this repository)

namespace ORB_SLAM3 {

void Optimizer::OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3, const map<KeyFrame *, set<KeyFrame *>> &LoopConnections,
                                       const bool &bFixScale) {
    RUMI_FACADE_NAMESPACE::Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale);
}
void Optimizer::OptimizeEssentialGraph(KeyFrame *pCurKF, vector<KeyFrame *> &vpFixedKFs, vector<KeyFrame *> &vpFixedCorrectedKFs,
                                       vector<KeyFrame *> &vpNonFixedKFs, vector<MapPoint *> &vpNonCorrectedMPs) {
    RUMI_FACADE_NAMESPACE::Optimizer::OptimizeEssentialGraph(pCurKF, vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs, vpNonCorrectedMPs);
}

}  // namespace ORB_SLAM3
