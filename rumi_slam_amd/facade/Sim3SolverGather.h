// The correspondences the constructor of Sim3Solver keeps (R/lib_src/Sim3Solver.cc:78-126), gathered once for both callers: shells/Sim3Solver.cc
// (which fills the reference's members from them) and Sim3RansacStage (PlaceRecognitionStages.h).  Templated on the data model.
#pragma once
#include <cstddef>
#include <tuple>
#include <vector>

namespace rumi_facade {

// What the constructor of Sim3Solver keeps (Sim3Solver.cc:78-126): one entry per usable correspondence.
struct Sim3Correspondences {
    std::vector<float> X1, X2, sigma2_1, sigma2_2;               // mvX3Dc1 / mvX3Dc2 (3 floats each), mvLevelSigma2 at the two key-points' octaves
    std::vector<size_t> indices1;                                // mvnIndices1
    int mN1 = 0;
    int N() const { return (int)indices1.size(); }
};
// vpKeyFrameMatchedMP empty: every match was found in pKF2.  mvX3Dc2 uses pKF2's pose even for a point matched in a covisible (pKFm, :96-97 read
// Rcw2 / tcw2 of pKF2), while the key-point and its sigma come from pKFm (:84-88).
template <class KeyFrameT, class MapPointT>
void sim3_solver_gather(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<MapPointT *> &vpMatched12, const std::vector<KeyFrameT *> &vpKeyFrameMatchedMP,
                        Sim3Correspondences &c) {
    const bool bDifferentKFs = !vpKeyFrameMatchedMP.empty();
    const std::vector<MapPointT *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    c.mN1 = (int)vpMatched12.size();
    const auto Rcw1 = pKF1->GetRotation(), Rcw2 = pKF2->GetRotation();
    const auto tcw1 = pKF1->GetTranslation(), tcw2 = pKF2->GetTranslation();
    KeyFrameT *pKFm = pKF2;
    for (int i1 = 0; i1 < c.mN1; i1++) {
        if (!vpMatched12[i1]) continue;
        MapPointT *pMP1 = vpKeyFrameMP1[i1], *pMP2 = vpMatched12[i1];
        if (!pMP1) continue;
        if (pMP1->isBad() || pMP2->isBad()) continue;
        if (bDifferentKFs) pKFm = vpKeyFrameMatchedMP[i1];
        const int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1)), indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKFm));
        if (indexKF1 < 0 || indexKF2 < 0) continue;
        const auto &kp1 = pKF1->mvKeysUn[indexKF1];
        const auto &kp2 = pKFm->mvKeysUn[indexKF2];
        c.sigma2_1.push_back(pKF1->mvLevelSigma2[kp1.octave]);
        c.sigma2_2.push_back(pKFm->mvLevelSigma2[kp2.octave]);
        c.indices1.push_back((size_t)i1);
        const auto X3D1w = pMP1->GetWorldPos(), X3D2w = pMP2->GetWorldPos();
        const auto a = Rcw1 * X3D1w + tcw1, b = Rcw2 * X3D2w + tcw2;
        for (int k = 0; k < 3; k++) { c.X1.push_back(a(k)); c.X2.push_back(b(k)); }
    }
}

}  // namespace rumi_facade
