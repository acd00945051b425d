// LocalMapping::CreateNewMapPoints (R/lib_src/LocalMapping.cc:354-647, monocular pinhole) over the MI355X C ABI (include/rumi_mapping.h).
// A member template over the data-model types, like the rest of facade/: it compiles against the reference's KeyFrame / MapPoint / Atlas (the
// member names used are theirs) and against the mock types of tests/cpp.  Everything here is marshalling and the replay of the map mutations:
// one C call searches, triangulates and gates every neighbour; the points come back in the order the reference creates them.
//
// In LocalMapping.cc the body of CreateNewMapPoints from `float th = 0.6f;` (:373) to its end becomes
//     rumi::LocalMappingStep step;                                   // = ORBmatcher matcher(0.6f, false)
//     step.CreateNewMapPoints<MapPoint>(mpCurrentKeyFrame, vpNeighKFs, mpAtlas, mlpRecentAddedMapPoints, mbFarPoints, mThFarPoints,
//                                       [this] { return CheckNewKeyFrames(); }, bCoarse);
// (the neighbour list, its inertial extension :362-371 and bCoarse :423 stay the caller's).
#pragma once
#include <utility>
#include <vector>

#include "ORBmatcher.h"
#include "rumi_mapping.h"

namespace RUMI_FACADE_NAMESPACE {

class LocalMappingStep : public ORBmatcher {
public:
    // LocalMapping.cc:373-375: `ORBmatcher matcher(th = 0.6f, false)`
    explicit LocalMappingStep(bool checkOri = false) : ORBmatcher(0.6f, checkOri) {}

#ifdef RUMI_HAVE_SOPHUS
    // MapPointT is the type the reference constructs (`new MapPoint(x3D, mpCurrentKeyFrame, mpAtlas->GetCurrentMap())`, :629).
    // CheckNewKeyFrames is asked before every neighbour but the first (:398-399); when it answers true the points of the neighbours so far
    // stay and the rest are dropped, which is what the reference's early return leaves (the results of the first i neighbours do not depend
    // on later ones).  Returns the number of points created, -1 when the device call failed (reported through rumi_status.h).
    // deferRefresh: when not NULL, the two per-point members (:639-641) are not called here; the created points are appended to it and the
    // caller refreshes them in one batch (rumi_facade::RefreshMapPoints, MapPointRefresh.h) -- same results, as neither member reads
    // another point.  NULL, the default, keeps the per-point calls.
    template <class MapPointT, class KeyFrameT, class AtlasT, class RecentListT, class CheckFn>
    int CreateNewMapPoints(KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpNeighKFs, AtlasT *pAtlas, RecentListT &mlpRecentAddedMapPoints,
                           bool bFarPoints, float thFarPoints, CheckFn CheckNewKeyFrames, bool bCoarse = false,
                           std::vector<MapPointT *> *deferRefresh = nullptr) {
        const int nn = (int)vpNeighKFs.size();
        if (nn == 0) return 0;
        if (nn > RUMI_NEWPTS_MAX_NEIGH) {
            rumi_facade::report("LocalMappingStep::CreateNewMapPoints", RUMI_E_INVALID, "more neighbours than RUMI_NEWPTS_MAX_NEIGH; no point was created");
            return -1;
        }
        for (KeyFrameT *pKF : vpNeighKFs)
            if (has_stereo(pKF) || has_stereo(pCurrentKF)) {   // stereo / two-camera branches (:446-504, 518-545, 576-607) are not built: say so, do not run them as mono
                rumi_facade::report("LocalMappingStep::CreateNewMapPoints", RUMI_E_INVALID, "a key-frame has stereo key-points (mvuRight >= 0): only the monocular branch is built; no point was created");
                return -1;
            }
        std::vector<Marshalled> hold(nn + 1);
        std::vector<RumiNewPointsKF> kf(nn + 1);
        marshal(pCurrentKF, false, hold[0], kf[0]);
        const Sophus::SE3f T1w = pCurrentKF->GetPose();
        const Eigen::Vector3f Cw = pCurrentKF->GetCameraCenter();
        const Eigen::Matrix3f K1 = pCurrentKF->mpCamera->toK_();
        for (int k = 0; k < nn; k++) {
            KeyFrameT *pKF2 = vpNeighKFs[k];
            marshal(pKF2, true, hold[1 + k], kf[1 + k]);
            // the epipole and F12 with the reference's own expressions, as SearchForTriangulation above forms them (ORBmatcher.cc:815-818,
            // GeometricTools::ComputeF12 / Pinhole::epipolarConstrain)
            const Sophus::SE3f T2w = pKF2->GetPose(), Tw2 = pKF2->GetPoseInverse();
            const Eigen::Vector3f C2 = T2w * Cw;
            const Eigen::Vector2f ep = pKF2->mpCamera->project(C2);
            const Sophus::SE3f T12 = T1w * Tw2;
            const Eigen::Matrix3f R12 = T12.rotationMatrix();
            const Eigen::Vector3f t12 = T12.translation();
            const Eigen::Matrix3f t12x = Sophus::SO3f::hat(t12);
            const Eigen::Matrix3f K2 = pKF2->mpCamera->toK_();
            const Eigen::Matrix3f F12 = K1.transpose().inverse() * t12x * R12 * K2.inverse();
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) kf[1 + k].F12[r * 3 + c] = F12(r, c);
            kf[1 + k].epipole2[0] = ep(0); kf[1 + k].epipole2[1] = ep(1);
        }
        RumiNewPointsParams prm;
        prm.coarse = bCoarse; prm.check_orientation = mbCheckOrientation; prm.far_points = bFarPoints; prm.th_far_points = thFarPoints;
        prm.ratio_factor = 1.5f * pCurrentKF->mfScaleFactor;                    // :391
        std::vector<RumiNewPoint> pts((size_t)(pCurrentKF->N > 0 ? pCurrentKF->N : 1));
        std::vector<int32_t> per(nn);
        std::vector<uint8_t> skipped(nn);
        int32_t nOut = 0;
        if (RUMI_GUARDED("LocalMappingStep / rumi_create_new_map_points", &ORBmatcher::grow_arena,
                         rumi_create_new_map_points(arena(), &kf[0], &kf[1], nn, &prm, pts.data(), (int32_t)pts.size(), &nOut, per.data(),
                                                    skipped.data())) != RUMI_OK)
            return -1;
        // :628-644 for every returned point, in the returned order, neighbour by neighbour
        int created = 0, next = 0;
        for (int i = 0; i < nn; i++) {
            if (i > 0 && CheckNewKeyFrames()) return created;                   // :398-399
            KeyFrameT *pKF2 = vpNeighKFs[i];
            for (int j = 0; j < per[i]; j++, next++) {
                const RumiNewPoint &P = pts[next];
                const Eigen::Vector3f x3D(P.x3D[0], P.x3D[1], P.x3D[2]);
                MapPointT *pMP = new MapPointT(x3D, pCurrentKF, pAtlas->GetCurrentMap());
                pMP->AddObservation(pCurrentKF, P.idx1);
                pMP->AddObservation(pKF2, P.idx2);
                pCurrentKF->AddMapPoint(pMP, P.idx1);
                pKF2->AddMapPoint(pMP, P.idx2);
                if (deferRefresh) deferRefresh->push_back(pMP);
                else {
                    pMP->ComputeDistinctiveDescriptors();
                    pMP->UpdateNormalAndDepth();
                }
                pAtlas->AddMapPoint(pMP);
                mlpRecentAddedMapPoints.push_back(pMP);
                created++;
            }
        }
        return created;
    }

protected:
    struct Marshalled { Csr fv; std::vector<int32_t> mp; std::vector<float> pos; };

    template <class KeyFrameT> static bool has_stereo(KeyFrameT *pKF) {
        for (float u : pKF->mvuRight) if (u >= 0) return true;
        return false;
    }

    template <class KeyFrameT> static void marshal(KeyFrameT *pKF, bool neighbour, Marshalled &h, RumiNewPointsKF &o) {
        o.feat = view(*pKF);
        h.fv = csr(pKF->mFeatVec);
        o.fv = RumiFeatureVector{(int32_t)h.fv.nodes.size(), h.fv.nodes.data(), h.fv.off.data(), h.fv.idx.data()};
        const auto vp = pKF->GetMapPointMatches();
        h.mp.assign(pKF->N, -1);
        h.pos.assign(neighbour ? (size_t)pKF->N * 3 : 0, 0.f);
        for (size_t i = 0; i < vp.size() && i < h.mp.size(); i++) {
            if (!vp[i]) continue;
            h.mp[i] = 0;
            if (neighbour) {                                                    // KeyFrame::ComputeSceneMedianDepth reads GetWorldPos() of every point (KeyFrame.cc:966-973)
                const Eigen::Vector3f X = vp[i]->GetWorldPos();
                for (int c = 0; c < 3; c++) h.pos[3 * i + c] = X(c);
            }
        }
        o.kf_mp = h.mp.data();
        o.mp_pos = neighbour ? h.pos.data() : nullptr;
        o.K4[0] = pKF->fx; o.K4[1] = pKF->fy; o.K4[2] = pKF->cx; o.K4[3] = pKF->cy;
        const Sophus::SE3f Tcw = pKF->GetPose();                                // eigTcw = sophTcw.matrix3x4() = [R | t] (:377-381, 427-431)
        const Eigen::Matrix3f R = Tcw.rotationMatrix();
        const Eigen::Vector3f t = Tcw.translation(), Ow = pKF->GetCameraCenter();
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o.Tcw[r * 4 + c] = R(r, c); o.Tcw[r * 4 + 3] = t(r); o.Ow[r] = Ow(r); }
        for (float &f : o.F12) f = 0.f;
        o.epipole2[0] = o.epipole2[1] = 0.f;
    }
#endif  // RUMI_HAVE_SOPHUS
};

}  // namespace RUMI_FACADE_NAMESPACE

namespace rumi { using LocalMappingStep = RUMI_FACADE_NAMESPACE::LocalMappingStep; }
