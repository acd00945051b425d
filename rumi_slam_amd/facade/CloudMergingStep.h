// Facade for the key-point match of CloudMerging::ComputeSubmapSim3 (R/lib_src/CloudMerging.cc:503-551): the loop over mKfMatch12 that looks every
// key-point of key-frame 1 up in key-frame 2 with KeyFrame::GetFeaturesInArea(u, v, 3) and keeps the nearest candidate where both slots hold a map
// point.  All pairs go to the GPU in one call (include/rumi_match.h: rumi_submap_match); this side marshals the key-frames and fills the four maps
// the loop fills.  ComputeSubmapSim3 below (with -DRUMI_HAVE_SOPHUS) is the whole function over the alignment session of include/rumi_opt.h
// (rumi_submap_sim3_*): the score set of ComputeInliersNum uploaded once, the RANSAC of every Sim3Solver in one call.  The per-call path
// (Sim3Scoring.h, shells/Sim3Solver.cc) stays valid.
//
// Each key-frame's grid is rebuilt on the device from mvKeysUn by the Frame::PosInGrid rule with the key-frame's own mnMinX, mnMinY and inverse cell
// sizes.  That equals mGrid for every key-frame built from a Frame (KeyFrame's constructor copies Frame::mGrid, which AssignFeaturesToGrid filled
// by that rule); the cloud map's key-frames are built that way (cloud_edge_main.cpp:944-948).
//
// Templated on the key-frame and map-point types, so that it instantiates against the reference's classes and against the stand-ins of tests/cpp.
#pragma once
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "rumi_match.h"
#include "rumi_status.h"
#ifdef RUMI_HAVE_SOPHUS
#include <cmath>
#include "Optimizer.h"
#include "RandLookahead.h"
#include "Sim3SolverGather.h"
#endif

namespace rumi_facade {

namespace submap_detail {
// One matcher arena per calling thread (handles are not re-entrant); the call's own blocks grow on demand, so there is nothing to double.
inline RumiMatcher *arena() {
    struct Holder { RumiMatcher *h = nullptr; ~Holder() { if (h) rumi_match_destroy(h); } };
    thread_local Holder holder;
    if (!holder.h) {
        const int rc = rumi_match_create(1, 1, -1, &holder.h);
        if (rc != RUMI_OK) { report("MatchSubmapKeyPoints: matcher arena", rc); holder.h = nullptr; }
    }
    return holder.h;
}

struct Marshalled { std::vector<float> keys, un; std::vector<uint8_t> mp; };
}  // namespace submap_detail

// Returns matchMapPointNum.  The four maps are filled as :546-550 fill them, keyed by vpMap1KeyFrames[iter->first]: vpMatchedPoints12 sized to
// key-frame 1's slots (NULL where there is no match), the two pair lists (equal, as in the reference) and matchNum.  Refused, with a report through
// rumi_status.h, 0 returned and the maps left empty: a key-frame with NLeft != -1 (the two-camera branch of GetFeaturesInArea is not built) or a
// grid other than 64 x 48; likewise when the device call fails.
template <class KeyFrameT, class MapPointT>
int MatchSubmapKeyPoints(const std::vector<KeyFrameT *> &vpMap1KeyFrames, const std::vector<KeyFrameT *> &vpMap2KeyFrames, const std::map<int, int> &mKfMatch12,
                         float tolerance, std::map<KeyFrameT *, std::vector<MapPointT *>> &mvpMatchedPoints12,
                         std::map<KeyFrameT *, std::vector<std::pair<int, int>>> &mvpMatchedKeyPoints12,
                         std::map<KeyFrameT *, std::vector<std::pair<int, int>>> &mvpValidMatchedKeyPoints12, std::map<KeyFrameT *, int> &mvpMatchedPointsNum12) {
    static const char *where = "CloudMergingStep::MatchSubmapKeyPoints / rumi_submap_match";
    if (mKfMatch12.empty()) return 0;
    // the frame table: every key-frame once, however many pairs name it
    std::map<KeyFrameT *, int> index;
    std::vector<KeyFrameT *> kfs;
    std::vector<std::vector<MapPointT *>> slots;
    std::vector<int32_t> f1, f2;
    auto frame_of = [&](KeyFrameT *pKF) {
        auto it = index.find(pKF);
        if (it != index.end()) return it->second;
        index[pKF] = (int)kfs.size();
        kfs.push_back(pKF);
        return (int)kfs.size() - 1;
    };
    for (const auto &m : mKfMatch12) {
        KeyFrameT *pKF1 = vpMap1KeyFrames[m.first], *pKF2 = vpMap2KeyFrames[m.second];
        for (KeyFrameT *pKF : {pKF1, pKF2})
            if (pKF->NLeft != -1 || pKF->mnGridCols != 64 || pKF->mnGridRows != 48) {
                // (the reason travels in the call site's name: the status did not come from the library, so its error string says nothing here)
                RUMI_GUARDED("CloudMergingStep::MatchSubmapKeyPoints: a key-frame with NLeft != -1 or a grid other than 64 x 48 (only the monocular 64 x 48 "
                             "lookup is built; no key-point was matched)", &no_growth, RUMI_E_INVALID);
                return 0;
            }
        f1.push_back(frame_of(pKF1)); f2.push_back(frame_of(pKF2));
    }
    std::vector<submap_detail::Marshalled> data(kfs.size());
    std::vector<RumiSubmapFrame> table(kfs.size());
    size_t sumQ = 0;
    for (size_t k = 0; k < kfs.size(); k++) {
        KeyFrameT *pKF = kfs[k];
        slots.push_back(pKF->GetMapPointMatches());
        const size_t n = pKF->mvKeys.size();
        auto &d = data[k];
        d.keys.resize(2 * n); d.un.resize(2 * n); d.mp.resize(n);
        for (size_t i = 0; i < n; i++) {
            d.keys[2 * i] = pKF->mvKeys[i].pt.x; d.keys[2 * i + 1] = pKF->mvKeys[i].pt.y;
            d.un[2 * i] = pKF->mvKeysUn[i].pt.x; d.un[2 * i + 1] = pKF->mvKeysUn[i].pt.y;
            d.mp[i] = i < slots[k].size() && slots[k][i] != nullptr;
        }
        table[k] = RumiSubmapFrame{(int32_t)n, d.keys.data(), d.un.data(), d.mp.data(), (float)pKF->mnMinX, (float)pKF->mnMinY,
                                   pKF->mfGridElementWidthInv, pKF->mfGridElementHeightInv, 0};
    }
    for (int32_t f : f1) sumQ += (size_t)table[f].n;
    std::vector<int32_t> best2(sumQ + 1), pairStart(f1.size() + 1), matches(2 * sumQ + 2);
    RumiMatcher *h = submap_detail::arena();
    if (!h) return 0;                                       // reported by arena()
    if (RUMI_GUARDED(where, &no_growth, rumi_submap_match(h, (int32_t)table.size(), table.data(), (int32_t)f1.size(), f1.data(), f2.data(), tolerance,
                                                          best2.data(), pairStart.data(), matches.data())) != RUMI_OK)
        return 0;
    int p = 0;
    for (const auto &m : mKfMatch12) {
        KeyFrameT *pKF1 = vpMap1KeyFrames[m.first];
        const auto &slots1 = slots[f1[p]], &slots2 = slots[f2[p]];
        std::vector<MapPointT *> vpMatchedPoints12(slots1.size(), static_cast<MapPointT *>(nullptr));
        std::vector<std::pair<int, int>> vpMatchedKeyPoints12;
        for (int k = pairStart[p]; k < pairStart[p + 1]; k++) {
            const int i1 = matches[2 * k], i2 = matches[2 * k + 1];
            vpMatchedPoints12[i1] = slots2[i2];
            vpMatchedKeyPoints12.push_back(std::pair<int, int>(i1, i2));
        }
        mvpMatchedPointsNum12[pKF1] = pairStart[p + 1] - pairStart[p];
        mvpMatchedPoints12[pKF1] = vpMatchedPoints12;
        mvpMatchedKeyPoints12[pKF1] = vpMatchedKeyPoints12;
        mvpValidMatchedKeyPoints12[pKF1] = vpMatchedKeyPoints12;
        p++;
    }
    return pairStart[f1.size()];
}

#ifdef RUMI_HAVE_SOPHUS
// ---- CloudMerging::ComputeSubmapSim3 (R/lib_src/CloudMerging.cc:434-825) over the alignment session ---------------------------------------------
namespace submap_detail {
struct Hessian77 { double m[7][7]; void setZero() { for (auto &r : m) for (double &x : r) x = 0; } };   // OptimizeCloudSim3 zeroes it, nobody reads it (:800-803)
template <class S> inline void push_sim3(std::vector<double> &v, const S &g) {
    const auto q = g.rotation(); const auto t = g.translation();
    const double a[8] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2), g.scale()};
    v.insert(v.end(), a, a + 8);
}
// What the Umeyama functor returns, as g2o::Sim3 (:591-595): Sim3Solver::umeyamaSolve's 4 x 4 matrix goes through Sophus::Sim3d as upstream; a functor
// that returns a g2o::Sim3 is taken as it is.
inline g2o::Sim3 umeyama_sim3(const g2o::Sim3 &S) { return S; }
template <class M4> inline g2o::Sim3 umeyama_sim3(const M4 &T) {
    const Sophus::Sim3<double> s(T);
    return g2o::Sim3(s.rotationMatrix(), s.translation(), s.scale());
}
}  // namespace submap_detail

// Filled when the caller passes one: what the RANSAC call was given and used.
struct SubmapSim3Stats { int solvers_sent = 0, iterations_sent = 0, iterations_consumed = 0, degenerate_sets = 0, converged_solver = -1; };

// The function's own text in order: MatchSubmapKeyPoints (:503-551), one gather of the score set and rumi_submap_sim3_begin, Umeyama of the camera
// centres through the functor (:582-595), score (:611), per entry of `order` (the shuffled vMatch1Indexes of :639-642: the caller shuffles) the < 5
// skip of :663 and the Sim3Solver constructor's filter (Sim3SolverGather.h) with SetRansacParameters(0.99, 5, 300) -- solvers with
// N < mRansacMinInliers draw nothing upstream and are not sent --, one rumi_submap_sim3_ransac, rand() advanced by three draws per iteration consumed,
// gRANSACSw1w2 (:732-738), score (:748), the choice of :785-791, Optimizer::OptimizeCloudSim3 (:803), score (:809), the test of :815, end.
// Returns 1 / 0 = true / false; -1 = refused with a report (rumi_status.h) and gSw1w2 / mvpMatchedKeyPoints12 untouched: a key-frame with
// NLeft != -1 or a grid other than 64 x 48, no matched key-frame pair, a failed device call.  On -1 the caller keeps the reference's function.
// Upstream reads bRANSACConverge uninitialised when no solver converges (:630, :745); here it starts false.
template <class KeyFrameT, class MapPointT, class Umeyama>
int ComputeSubmapSim3(const std::vector<KeyFrameT *> &vpMap1KeyFrames, const std::vector<KeyFrameT *> &vpMap2KeyFrames, const std::map<int, int> &mKfMatch12,
                      const std::map<int, int> &mRandSelectKfMatch12, const std::vector<int> &order, bool bFixScale, g2o::Sim3 &gSw1w2,
                      std::map<KeyFrameT *, std::vector<std::pair<int, int>>> &mvpMatchedKeyPoints12, Umeyama umeyamaSolve, SubmapSim3Stats *stats = nullptr) {
    using Opt = RUMI_FACADE_NAMESPACE::Optimizer;
    static const char *where = "CloudMergingStep::ComputeSubmapSim3";
    for (const auto &m : mKfMatch12)
        for (KeyFrameT *pKF : {vpMap1KeyFrames[m.first], vpMap2KeyFrames[m.second]})
            if (pKF->NLeft != -1 || pKF->mnGridCols != 64 || pKF->mnGridRows != 48) {
                RUMI_GUARDED("CloudMergingStep::ComputeSubmapSim3: a key-frame with NLeft != -1 or a grid other than 64 x 48 (only the monocular 64 x 48 lookup is "
                             "built; nothing was computed)", &no_growth, RUMI_E_INVALID);
                return -1;
            }
    if (mKfMatch12.empty()) { RUMI_GUARDED("CloudMergingStep::ComputeSubmapSim3: no matched key-frame pair", &no_growth, RUMI_E_INVALID); return -1; }
    std::map<KeyFrameT *, std::vector<MapPointT *>> mvpMatchedPoints12;
    std::map<KeyFrameT *, std::vector<std::pair<int, int>>> matchedKP, mvpValidMatchedKeyPoints12;
    std::map<KeyFrameT *, int> mvpMatchedPointsNum12;
    clear_status();
    MatchSubmapKeyPoints<KeyFrameT, MapPointT>(vpMap1KeyFrames, vpMap2KeyFrames, mKfMatch12, 3.f, mvpMatchedPoints12, matchedKP, mvpValidMatchedKeyPoints12, mvpMatchedPointsNum12);
    if (last_status() != RUMI_OK) return -1;                                  // reported there
    std::vector<KeyFrameT *> matchMap1KeyFrames, matchMap2KeyFrames;          // :566-579
    std::vector<std::vector<MapPointT *>> avpMatchedPoints;
    std::vector<std::vector<std::pair<int, int>>> avpValidKPMatches;
    for (const auto &m : mKfMatch12) {
        matchMap1KeyFrames.push_back(vpMap1KeyFrames[m.first]); matchMap2KeyFrames.push_back(vpMap2KeyFrames[m.second]);
        avpMatchedPoints.push_back(mvpMatchedPoints12[vpMap1KeyFrames[m.first]]);
        avpValidKPMatches.push_back(mvpValidMatchedKeyPoints12[vpMap1KeyFrames[m.first]]);
    }
    // the data ComputeInliersNum reads (Sim3Solver.cc:586-664), gathered once
    std::vector<int32_t> pairStart(1, 0), denom;
    std::vector<double> Sc1w1, Sc2w2;
    std::vector<float> X1, X2, k1, k2, s1, s2;
    std::vector<uint8_t> e1, e2;
    std::vector<g2o::Sim3> gSc1w1s, gSc2w2s;
    float K1[4] = {0, 0, 0, 0}, K2[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < matchMap1KeyFrames.size(); i++) {
        KeyFrameT *KF1 = matchMap1KeyFrames[i], *KF2 = matchMap2KeyFrames[i];
        if (!KF1 || !KF2) continue;
        const auto Tc1w1 = KF1->GetPose(); const auto Tc2w2 = KF2->GetPose();
        gSc1w1s.emplace_back(Tc1w1.rotationMatrix().template cast<double>(), Tc1w1.translation().template cast<double>(), 1.0);
        gSc2w2s.emplace_back(Tc2w2.rotationMatrix().template cast<double>(), Tc2w2.translation().template cast<double>(), 1.0);
        submap_detail::push_sim3(Sc1w1, g2o::Sim3(KF1->GetRotation().template cast<double>(), KF1->GetTranslation().template cast<double>(), 1.0));
        submap_detail::push_sim3(Sc2w2, g2o::Sim3(KF2->GetRotation().template cast<double>(), KF2->GetTranslation().template cast<double>(), 1.0));
        K1[0] = KF1->fx; K1[1] = KF1->fy; K1[2] = KF1->cx; K1[3] = KF1->cy;
        K2[0] = KF2->fx; K2[1] = KF2->fy; K2[2] = KF2->cx; K2[3] = KF2->cy;
        const auto vpMPs1 = KF1->GetMapPointMatches(), vpMPs2 = KF2->GetMapPointMatches();
        for (const auto &m : avpValidKPMatches[i]) {
            auto *p1 = vpMPs1[m.first]; auto *p2 = vpMPs2[m.second];
            if (!p1 || !p2) continue;
            const auto P1 = p1->GetWorldPos(), P2 = p2->GetWorldPos();
            for (int c = 0; c < 3; c++) { X1.push_back(P1(c)); X2.push_back(P2(c)); }
            const auto &kp1 = KF1->mvKeys[m.first]; const auto &kp2 = KF2->mvKeys[m.second];
            k1.push_back(kp1.pt.x); k1.push_back(kp1.pt.y); k2.push_back(kp2.pt.x); k2.push_back(kp2.pt.y);
            s1.push_back(KF1->mvLevelSigma2[kp1.octave]); s2.push_back(KF2->mvLevelSigma2[kp2.octave]);
            e1.push_back(p1->isEdge); e2.push_back(p2->isEdge);
        }
        pairStart.push_back((int32_t)e1.size());
        denom.push_back((int32_t)avpValidKPMatches[i].size());
    }
    const int nPairs = (int)denom.size();
    if (nPairs == 0) { RUMI_GUARDED("CloudMergingStep::ComputeSubmapSim3: no matched key-frame pair", &no_growth, RUMI_E_INVALID); return -1; }
    const RumiSim3ScoreSet set{nPairs, pairStart.data(), denom.data(), Sc1w1.data(), Sc2w2.data(), nullptr, nullptr, K1, K2,
                               X1.data(), X2.data(), k1.data(), k2.data(), s1.data(), s2.data(), e1.data(), e2.data()};
    if (!Opt::arena()) return -1;                                             // reported by arena()
    bool open = false;
    auto begin = [&]() { open = RUMI_GUARDED("CloudMergingStep::ComputeSubmapSim3 / rumi_submap_sim3_begin", &no_growth, rumi_submap_sim3_begin(Opt::arena(), &set)) == RUMI_OK; return open; };
    auto refuse = [&]() { if (open && Opt::arena_slot()) (void)rumi_submap_sim3_end(Opt::arena_slot()); return -1; };
    if (!begin()) return -1;
    // ComputeInliersNum of one transform on the resident set: the composed transforms as Sim3Scoring.h forms them (:620-621)
    auto score = [&](g2o::Sim3 &S, float &ratio) {
        std::vector<double> A, B;
        for (int p = 0; p < nPairs; p++) {
            const g2o::Sim3 gSc2w1 = gSc2w2s[p] * S.inverse(), gSc1w2 = gSc1w1s[p] * S;
            submap_detail::push_sim3(A, gSc1w2); submap_detail::push_sim3(B, gSc2w1);
        }
        return RUMI_GUARDED("CloudMergingStep::ComputeSubmapSim3 / rumi_submap_sim3_score", &no_growth,
                            rumi_submap_sim3_score(Opt::arena(), 1, A.data(), B.data(), nullptr, nullptr, &ratio)) == RUMI_OK;
    };
    // Umeyama of the camera centres (:582-595)
    std::vector<Eigen::Vector3d> map1MatchKFPoints, map2MatchKFPoints;
    for (const auto &m : mRandSelectKfMatch12) {
        map1MatchKFPoints.push_back(vpMap1KeyFrames[m.first]->GetPoseInverse().translation().template cast<double>());
        map2MatchKFPoints.push_back(vpMap2KeyFrames[m.second]->GetPoseInverse().translation().template cast<double>());
    }
    g2o::Sim3 gUmeyamaSw1w2 = submap_detail::umeyama_sim3(umeyamaSolve(map2MatchKFPoints, map1MatchKFPoints));
    float umeyamaInliersRatio = 0.f;
    if (!score(gUmeyamaSw1w2, umeyamaInliersRatio)) return refuse();          // :611
    // the solvers of :643-741, in the caller's order
    const int nSolveSim3Inliers = 5;
    std::vector<RumiSubmapSolver> solvers;
    std::vector<std::pair<KeyFrameT *, KeyFrameT *>> solverKFs;
    std::vector<float> cX1, cX2, cS1, cS2;
    for (int match1Index : order) {
        KeyFrameT *pKF1 = vpMap1KeyFrames[match1Index], *pKF2 = vpMap2KeyFrames[mRandSelectKfMatch12.at(match1Index)];
        const auto num = mvpMatchedPointsNum12.find(pKF1);
        if (num == mvpMatchedPointsNum12.end() || num->second < 5) continue;  // :663
        const std::vector<MapPointT *> &vpMatchedPoints12 = mvpMatchedPoints12[pKF1];
        const std::vector<KeyFrameT *> vpKeyFrameMatchedMP12(vpMatchedPoints12.size(), pKF2);
        Sim3Correspondences c;
        sim3_solver_gather(pKF1, pKF2, vpMatchedPoints12, vpKeyFrameMatchedMP12, c);
        const int N = c.N();
        if (N < nSolveSim3Inliers) continue;                                  // iterate returns bNoMore at once and draws nothing
        RumiSubmapSolver r;
        r.first = (int32_t)cS1.size(); r.n = N; r.min_inliers = nSolveSim3Inliers; r.fix_scale = bFixScale ? 1 : 0;
        const float epsilon = (float)nSolveSim3Inliers / N;                   // SetRansacParameters(0.99, 5, 300), Sim3Solver.cc:134-157
        int nIterations;
        if (nSolveSim3Inliers == N) nIterations = 1;
        else nIterations = (int)std::ceil(std::log(1 - 0.99) / std::log(1 - std::pow(epsilon, 3)));
        r.its = std::max(1, std::min(nIterations, 300));
        for (int k = 0; k < 4; k++) { r.K4_1[k] = pKF1->mpCamera->getParameter(k); r.K4_2[k] = pKF2->mpCamera->getParameter(k); }
        std::vector<double> kf;
        submap_detail::push_sim3(kf, g2o::Sim3(pKF1->GetRotation().template cast<double>(), pKF1->GetTranslation().template cast<double>(), 1.0));   // gSc1w (Sim3Solver.cc:342)
        submap_detail::push_sim3(kf, g2o::Sim3(pKF2->GetRotation().template cast<double>(), pKF2->GetTranslation().template cast<double>(), 1.0));   // gSc2w (:343)
        for (int k = 0; k < 8; k++) { r.S_kf1w[k] = kf[k]; r.S_kf2w[k] = kf[8 + k]; }
        cX1.insert(cX1.end(), c.X1.begin(), c.X1.end()); cX2.insert(cX2.end(), c.X2.begin(), c.X2.end());
        cS1.insert(cS1.end(), c.sigma2_1.begin(), c.sigma2_1.end()); cS2.insert(cS2.end(), c.sigma2_2.begin(), c.sigma2_2.end());
        solvers.push_back(r);
        solverKFs.emplace_back(pKF1, pKF2);
    }
    bool bRANSACConverge = false;
    g2o::Sim3 gRANSACSw1w2;
    if (!solvers.empty()) {
        size_t H = 0;
        for (const auto &r : solvers) H += (size_t)r.its;
        std::vector<int32_t> tri(H * 3);
        {                                                                     // Sim3Solver.cc:321-331 on a copy of the generator
            RandLookahead ahead;
            std::vector<int32_t> avail;
            size_t h = 0;
            for (const auto &r : solvers)
                for (int it = 0; it < r.its; it++, h++) {
                    avail.resize(r.n);
                    for (int k = 0; k < r.n; k++) avail[k] = k;
                    for (int i = 0; i < 3; i++) {
                        const int randi = ahead.RandomInt(0, (int)avail.size() - 1);
                        tri[h * 3 + i] = avail[randi];
                        avail[randi] = avail.back();
                        avail.pop_back();
                    }
                }
        }
        std::vector<RumiSubmapSolverResult> res(solvers.size());
        std::vector<float> Tall(stats ? H * 16 : 0);
        int32_t used = 0;
        if (RUMI_GUARDED("CloudMergingStep::ComputeSubmapSim3 / rumi_submap_sim3_ransac", &no_growth,
                         rumi_submap_sim3_ransac(Opt::arena(), (int32_t)solvers.size(), solvers.data(), (int32_t)cS1.size(), cX1.data(), cX2.data(), cS1.data(), cS2.data(),
                                                 tri.data(), 0.f, res.data(), &used, nullptr, nullptr, stats ? Tall.data() : nullptr)) != RUMI_OK)
            return refuse();
        rand_advance(used);                                                   // rand() stands where upstream's loop leaves it
        if (stats) {
            stats->solvers_sent = (int)solvers.size(); stats->iterations_sent = (int)H; stats->iterations_consumed = used;
            for (int h = 0; h < used; h++) stats->degenerate_sets += Tall[(size_t)h * 16 + 13] == 0.f;
        }
        for (size_t j = 0; j < solvers.size(); j++) {
            if (res[j].state != RUMI_SIM3_CONVERGED) continue;
            bRANSACConverge = true;                                           // :729-739
            if (stats) stats->converged_solver = (int)j;
            Eigen::Matrix3f R; Eigen::Vector3f t;
            for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) R(a, b) = res[j].T12[a * 3 + b]; t(a) = res[j].T12[9 + a]; }
            const g2o::Sim3 gSc1c2(R.template cast<double>(), t.template cast<double>(), (double)res[j].T12[12]);
            KeyFrameT *pKF1 = solverKFs[j].first, *pKF2 = solverKFs[j].second;
            const g2o::Sim3 gSc1w(pKF1->GetRotation().template cast<double>(), pKF1->GetTranslation().template cast<double>(), 1.0);
            const g2o::Sim3 gSc2w(pKF2->GetRotation().template cast<double>(), pKF2->GetTranslation().template cast<double>(), 1.0);
            gRANSACSw1w2 = gSc1w.inverse() * gSc1c2 * gSc2w;
        }
    }
    float RANSACInliersRatio = 0;
    if (bRANSACConverge && !score(gRANSACSw1w2, RANSACInliersRatio)) return refuse();   // :748
    g2o::Sim3 S = umeyamaInliersRatio >= RANSACInliersRatio ? gUmeyamaSw1w2 : gRANSACSw1w2;   // :785-791
    submap_detail::Hessian77 mHessian7x7;
    const int scale = Opt::arena_scale();
    clear_status();
    Opt::OptimizeCloudSim3(matchMap1KeyFrames, matchMap2KeyFrames, avpMatchedPoints, S, 10, true, mHessian7x7, true);   // :803
    if (last_status() != RUMI_OK) return refuse();
    if (Opt::arena_scale() != scale && !begin()) return -1;                   // the optimiser grew its arena: a new handle, the set goes up again
    float OptimizeInliersRatio = 0.f;
    if (!score(S, OptimizeInliersRatio)) return refuse();                     // :809
    (void)rumi_submap_sim3_end(Opt::arena());
    gSw1w2 = S;
    for (const auto &kv : matchedKP) mvpMatchedKeyPoints12[kv.first] = kv.second;   // :549
    return OptimizeInliersRatio > 0.1 ? 1 : 0;                                // :815
}
#endif  // RUMI_HAVE_SOPHUS

}  // namespace rumi_facade
