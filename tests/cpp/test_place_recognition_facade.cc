// LoopClosingStep::DetectCommonRegionsFromBoWResident (facade/LoopClosingStep.h: the function stage by stage, every candidate in one device call a
// stage) against the reference's text of LoopClosing.cc:576-853 over the per-call facade members -- ORBmatcher::SearchByBoW, a shell-style solver on
// rumi_sim3_ransac in blocks of 20, Optimizer::OptimizeSim3, the per-call SearchByProjection -- on a copy of the same map, on the GPU.  Reads a map
// written by tests/test_place_recognition_facade_gpu.py.  Map A belongs to a graph and takes the member; map B takes the text.  Both sides start
// with srand reset, after one device call has been made (the runtime may draw from rand() while it loads).  Prints, per side,
//   D side ret matchedKF nNumCoincidences notErase lastCurrentKF nextRand | g2oScw as 8 doubles in hex | vpMPs ids | vpMatchedMPs ids
//   T B cand numBoWMatches converged numProjMatches numOptMatches numProjOptMatches nNumKFs         what the text saw of every candidate
//   R A ret status untouched|TOUCHED                                                              a refused call
//   K / P side ...                                                                                the map
#define RUMI_HAVE_SOPHUS 1
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "mock_sophus.h"

#include "CovisibilityGraph.h"
#include "LoopClosingStep.h"
#include "Optimizer.h"

#include "sim3_projection_world.h"

static void print(const char *tag, World &w) {
    for (size_t k = 0; k < w.kfs.size(); k++) {
        std::printf("K %s %zu %d |", tag, k, (int)w.kfs[k]->mbNotErase);
        for (MapPoint *p : w.kfs[k]->mvpMapPoints) std::printf(" %d", p ? w.pi[p] : -1);
        std::printf("\n");
    }
    for (size_t i = 0; i < w.mps.size(); i++) {
        MapPointSN *p = w.mps[i].get();
        std::printf("P %s %zu %d %zu %08x\n", tag, i, (int)p->bad, p->obs.size(), *reinterpret_cast<const uint32_t *>(p->desc.ptr(0)));
    }
}
static void ids(World &w, const std::vector<MapPointSN *> &v) { for (MapPointSN *p : v) std::printf(" %d", p ? w.pi[p] : -1); }

// ---- the per-candidate solver of side B: shells/Sim3Solver.cc's iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge) over this data model ----
struct RefSolver {
    rumi_facade::Sim3Correspondences c;
    float K1[4], K2[4];
    bool fix;
    int minInliers = 0, maxIts = 0, its = 0, nBest = 0;
    Eigen::Matrix3f R; Eigen::Vector3f t; float s = 1.f;
    RefSolver(KeyFrameSN *pKF1, KeyFrameSN *pKF2, const std::vector<MapPointSN *> &m12, bool bFixScale, const std::vector<KeyFrameSN *> &kfm) : fix(bFixScale) {
        rumi_facade::sim3_solver_gather(pKF1, pKF2, m12, kfm, c);
        for (int i = 0; i < 4; i++) { K1[i] = pKF1->mpCamera->getParameter(i); K2[i] = pKF2->mpCamera->getParameter(i); }
    }
    void SetRansacParameters(double p, int minIn, int maxIt) { minInliers = minIn; maxIts = rumi_facade::sim3_ransac_max_its(p, minIn, maxIt, c.N()); its = 0; }
    void iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, bool &bConverge) {
        bNoMore = false; bConverge = false; nInliers = 0;
        vbInliers.assign((size_t)c.mN1, false);
        const int N = c.N();
        if (N < minInliers) { bNoMore = true; return; }
        const int count = std::max(0, std::min(nIterations, maxIts - its));
        std::vector<int32_t> tri((size_t)count * 3), nIn(count);
        std::vector<float> T((size_t)count * 16);
        std::vector<uint8_t> inl((size_t)count * N + 1);
        {
            rumi_facade::RandLookahead ahead;
            std::vector<int32_t> avail;
            for (int h = 0; h < count; h++) {
                avail.resize(N);
                for (int i = 0; i < N; i++) avail[i] = i;
                for (int i = 0; i < 3; i++) { const int r = ahead.RandomInt(0, (int)avail.size() - 1); tri[(size_t)h * 3 + i] = avail[r]; avail[r] = avail.back(); avail.pop_back(); }
            }
        }
        if (count > 0 && rumi_sim3_ransac(ORB_SLAM3::Optimizer::arena(), N, c.X1.data(), c.X2.data(), c.sigma2_1.data(), c.sigma2_2.data(), K1, K2, fix ? 1 : 0, count, tri.data(), nullptr,
                                          T.data(), nIn.data(), inl.data(), nullptr, nullptr) != RUMI_OK) { bNoMore = true; return; }
        int cur = 0;                                               // mnInliersi: a degenerate set keeps the previous iteration's
        for (int h = 0; h < count; h++) {
            its++;
            rumi_facade::rand_advance(1);
            const float *Th = &T[(size_t)h * 16];
            if (Th[13] != 0.f) cur = nIn[h];
            if (cur >= nBest && Th[13] != 0.f) {
                nBest = cur; nInliers = cur;
                for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) R(r, q) = Th[r * 3 + q]; t(r) = Th[9 + r]; }
                s = Th[12];
                if (cur > minInliers) {
                    for (int i = 0; i < N; i++) if (inl[(size_t)h * N + i]) vbInliers[c.indices1[i]] = true;
                    bConverge = true;
                    return;
                }
            }
        }
        if (its >= maxIts) bNoMore = true;
    }
};

// LoopClosing.cc:868-914 and :855-866 as written, over the facade's per-call SearchByProjection
static int FindMatchesByProjection(KeyFrameSN *pCurrentKF, KeyFrameSN *pMatchedKFw, g2o::Sim3 &g2oScw, std::vector<MapPointSN *> &vpMapPoints,
                                   std::vector<MapPointSN *> &vpMatchedMapPoints) {
    int nNumCovisibles = 10;
    std::vector<KeyFrameSN *> vpCovKFm = pMatchedKFw->GetBestCovisibilityKeyFrames(nNumCovisibles);
    int nInitialCov = vpCovKFm.size();
    vpCovKFm.push_back(pMatchedKFw);
    if (nInitialCov < nNumCovisibles) {
        for (int i = 0; i < nInitialCov; ++i) {
            std::vector<KeyFrameSN *> vpKFs = vpCovKFm[i]->GetBestCovisibilityKeyFrames(nNumCovisibles);
            vpCovKFm.insert(vpCovKFm.end(), vpKFs.begin(), vpKFs.end());
        }
    }
    std::set<MapPointSN *> spMapPoints;
    vpMapPoints.clear();
    vpMatchedMapPoints.clear();
    for (KeyFrameSN *pKFi : vpCovKFm)
        for (MapPointSN *pMPij : pKFi->GetMapPointMatches()) {
            if (!pMPij || pMPij->isBad()) continue;
            if (spMapPoints.find(pMPij) == spMapPoints.end()) { spMapPoints.insert(pMPij); vpMapPoints.push_back(pMPij); }
        }
    Sophus::Sim3f mScw = toSophusMock(g2oScw);
    rumi::LoopClosingStep matcher;
    vpMatchedMapPoints.resize(pCurrentKF->GetMapPointMatches().size(), static_cast<MapPointSN *>(NULL));
    return matcher.SearchByProjection(pCurrentKF, mScw, vpMapPoints, vpMatchedMapPoints, 3, 1.5);
}
static bool DetectCommonRegionsFromLastKF(KeyFrameSN *pCurrentKF, KeyFrameSN *pMatchedKF, g2o::Sim3 &gScw, int &nNumProjMatches, std::vector<MapPointSN *> &vpMPs,
                                          std::vector<MapPointSN *> &vpMatchedMPs) {
    nNumProjMatches = FindMatchesByProjection(pCurrentKF, pMatchedKF, gScw, vpMPs, vpMatchedMPs);
    int nProjMatches = 30;
    return nNumProjMatches >= nProjMatches;
}

using Th = rumi::LoopClosingStep::PlaceRecognitionThresholds;

// :542-853 as written (the counters of the function's debug output left out)
static bool DetectCommonRegionsFromBoW(World &w, const Th &th, bool mbFixScale, std::vector<KeyFrameSN *> &vpBowCand, KeyFrameSN *&pMatchedKF2, KeyFrameSN *&pLastCurrentKF,
                                       g2o::Sim3 &g2oScw, int &nNumCoincidences, std::vector<MapPointSN *> &vpMPs, std::vector<MapPointSN *> &vpMatchedMPs) {
    KeyFrameSN *mpCurrentKF = w.cur;
    const int nBoWMatches = th.nBoWMatches, nBoWInliers = th.nBoWInliers, nSim3Inliers = th.nSim3Inliers, nProjMatches = th.nProjMatches, nProjOptMatches = th.nProjOptMatches;
    std::set<KeyFrameSN *> spConnectedKeyFrames;
    for (auto &e : mpCurrentKF->mConnectedKeyFrameWeights) spConnectedKeyFrames.insert(e.first);      // GetConnectedKeyFrames()
    int nNumCovisibles = th.nNumCovisibles;
    ORB_SLAM3::ORBmatcher matcherBoW(0.9, true);
    rumi::LoopClosingStep matcher;
    KeyFrameSN *pBestMatchedKF = nullptr;
    int nBestMatchesReproj = 0, nBestNumCoindicendes = 0;
    g2o::Sim3 g2oBestScw;
    std::vector<MapPointSN *> vpBestMapPoints, vpBestMatchedMapPoints;
    for (KeyFrameSN *pKFi : vpBowCand) {
        if (!pKFi || pKFi->isBad()) continue;
        std::vector<KeyFrameSN *> vpCovKFi = pKFi->GetBestCovisibilityKeyFrames(nNumCovisibles);
        if (vpCovKFi.empty()) vpCovKFi.push_back(pKFi);
        else { vpCovKFi.push_back(vpCovKFi[0]); vpCovKFi[0] = pKFi; }
        bool bAbortByNearKF = false;
        for (size_t j = 0; j < vpCovKFi.size(); ++j)
            if (spConnectedKeyFrames.find(vpCovKFi[j]) != spConnectedKeyFrames.end()) { bAbortByNearKF = true; break; }
        if (bAbortByNearKF) { std::printf("T B %d aborted\n", w.ki[pKFi]); continue; }
        std::vector<std::vector<MapPointSN *>> vvpMatchedMPs;
        vvpMatchedMPs.resize(vpCovKFi.size());
        std::set<MapPointSN *> spMatchedMPi;
        int numBoWMatches = 0;
        KeyFrameSN *pMostBoWMatchesKF = pKFi;
        int nMostBoWNumMatches = 0;
        std::vector<MapPointSN *> vpMatchedPoints = std::vector<MapPointSN *>(mpCurrentKF->GetMapPointMatches().size(), static_cast<MapPointSN *>(NULL));
        std::vector<KeyFrameSN *> vpKeyFrameMatchedMP = std::vector<KeyFrameSN *>(mpCurrentKF->GetMapPointMatches().size(), static_cast<KeyFrameSN *>(NULL));
        for (size_t j = 0; j < vpCovKFi.size(); ++j) {
            if (!vpCovKFi[j] || vpCovKFi[j]->isBad()) continue;
            int num = matcherBoW.SearchByBoW(mpCurrentKF, vpCovKFi[j], vvpMatchedMPs[j]);
            if (num > nMostBoWNumMatches) nMostBoWNumMatches = num;
        }
        for (size_t j = 0; j < vpCovKFi.size(); ++j)
            for (size_t k = 0; k < vvpMatchedMPs[j].size(); ++k) {
                MapPointSN *pMPi_j = vvpMatchedMPs[j][k];
                if (!pMPi_j || pMPi_j->isBad()) continue;
                if (spMatchedMPi.find(pMPi_j) == spMatchedMPi.end()) {
                    spMatchedMPi.insert(pMPi_j);
                    numBoWMatches++;
                    vpMatchedPoints[k] = pMPi_j;
                    vpKeyFrameMatchedMP[k] = vpCovKFi[j];
                }
            }
        int conv = 0, t716 = -1, tOpt = -1, t738 = -1, tKFs = -1;
        if (numBoWMatches >= nBoWMatches) {
            bool bFixedScale = mbFixScale;
            RefSolver solver(mpCurrentKF, pMostBoWMatchesKF, vpMatchedPoints, bFixedScale, vpKeyFrameMatchedMP);
            solver.SetRansacParameters(0.99, nBoWInliers, 300);
            bool bNoMore = false; std::vector<bool> vbInliers; int nInliers; bool bConverge = false;
            while (!bConverge && !bNoMore) solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
            conv = bConverge;
            if (bConverge) {
                vpCovKFi.clear();
                vpCovKFi = pMostBoWMatchesKF->GetBestCovisibilityKeyFrames(nNumCovisibles);
                vpCovKFi.push_back(pMostBoWMatchesKF);
                std::set<MapPointSN *> spMapPoints;
                std::vector<MapPointSN *> vpMapPoints;
                std::vector<KeyFrameSN *> vpKeyFrames;
                for (KeyFrameSN *pCovKFi : vpCovKFi)
                    for (MapPointSN *pCovMPij : pCovKFi->GetMapPointMatches()) {
                        if (!pCovMPij || pCovMPij->isBad()) continue;
                        if (spMapPoints.find(pCovMPij) == spMapPoints.end()) { spMapPoints.insert(pCovMPij); vpMapPoints.push_back(pCovMPij); vpKeyFrames.push_back(pCovKFi); }
                    }
                g2o::Sim3 gScm(solver.R.cast<double>(), solver.t.cast<double>(), (double)solver.s);
                g2o::Sim3 gSmw(pMostBoWMatchesKF->GetRotation().cast<double>(), pMostBoWMatchesKF->GetTranslation().cast<double>(), 1.0);
                g2o::Sim3 gScw = gScm * gSmw;
                Sophus::Sim3f mScw = toSophusMock(gScw);
                std::vector<MapPointSN *> vpMatchedMP;
                vpMatchedMP.resize(mpCurrentKF->GetMapPointMatches().size(), static_cast<MapPointSN *>(NULL));
                std::vector<KeyFrameSN *> vpMatchedKF;
                vpMatchedKF.resize(mpCurrentKF->GetMapPointMatches().size(), static_cast<KeyFrameSN *>(NULL));
                int numProjMatches = matcher.SearchByProjection(mpCurrentKF, mScw, vpMapPoints, vpKeyFrames, vpMatchedMP, vpMatchedKF, 8, 1.5);
                t716 = numProjMatches;
                if (numProjMatches >= nProjMatches) {
                    Eigen::Matrix77d mHessian7x7;
                    int numOptMatches = ORB_SLAM3::Optimizer::OptimizeSim3(mpCurrentKF, pKFi, vpMatchedMP, gScm, 10, mbFixScale, mHessian7x7, true);
                    tOpt = numOptMatches;
                    if (numOptMatches >= nSim3Inliers) {
                        g2o::Sim3 gSmw(pMostBoWMatchesKF->GetRotation().cast<double>(), pMostBoWMatchesKF->GetTranslation().cast<double>(), 1.0);
                        g2o::Sim3 gScw = gScm * gSmw;
                        Sophus::Sim3f mScw = toSophusMock(gScw);
                        std::vector<MapPointSN *> vpMatchedMP;
                        vpMatchedMP.resize(mpCurrentKF->GetMapPointMatches().size(), static_cast<MapPointSN *>(NULL));
                        int numProjOptMatches = matcher.SearchByProjection(mpCurrentKF, mScw, vpMapPoints, vpMatchedMP, 5, 1.0);
                        t738 = numProjOptMatches;
                        if (numProjOptMatches >= nProjOptMatches) {
                            int nNumKFs = 0;
                            std::vector<KeyFrameSN *> vpCurrentCovKFs = mpCurrentKF->GetBestCovisibilityKeyFrames(nNumCovisibles);
                            size_t j = 0;
                            while (nNumKFs < 3 && j < vpCurrentCovKFs.size()) {
                                KeyFrameSN *pKFj = vpCurrentCovKFs[j];
                                const Sophus::SE3f Tjc = pKFj->GetPose() * mpCurrentKF->GetPoseInverse();
                                const auto q = Tjc.unit_quaternion(); const auto t = Tjc.translation();
                                g2o::Sim3 gSjc(Eigen::Quaterniond(q.w(), q.x(), q.y(), q.z()), Eigen::Vector3d(t(0), t(1), t(2)), 1.0);
                                g2o::Sim3 gSjw = gSjc * gScw;
                                int numProjMatches_j = 0;
                                std::vector<MapPointSN *> vpMatchedMPs_j;
                                bool bValid = DetectCommonRegionsFromLastKF(pKFj, pMostBoWMatchesKF, gSjw, numProjMatches_j, vpMapPoints, vpMatchedMPs_j);
                                if (bValid) nNumKFs++;
                                j++;
                            }
                            tKFs = nNumKFs;
                            if (nBestMatchesReproj < numProjOptMatches) {
                                nBestMatchesReproj = numProjOptMatches;
                                nBestNumCoindicendes = nNumKFs;
                                pBestMatchedKF = pMostBoWMatchesKF;
                                g2oBestScw = gScw;
                                vpBestMapPoints = vpMapPoints;
                                vpBestMatchedMapPoints = vpMatchedMP;
                            }
                        }
                    }
                }
            }
        }
        std::printf("T B %d %d %d %d %d %d %d\n", w.ki[pKFi], numBoWMatches, conv, t716, tOpt, t738, tKFs);
    }
    if (nBestMatchesReproj > 0) {
        pLastCurrentKF = mpCurrentKF;
        nNumCoincidences = nBestNumCoindicendes;
        pMatchedKF2 = pBestMatchedKF;
        pMatchedKF2->mbNotErase = true;                            // SetNotErase()
        g2oScw = g2oBestScw;
        vpMPs = vpBestMapPoints;
        vpMatchedMPs = vpBestMatchedMapPoints;
        return nNumCoincidences >= 3;
    }
    return false;
}

struct Outputs {
    KeyFrameSN *pMatchedKF2 = nullptr, *pLastCurrentKF = nullptr;
    g2o::Sim3 g2oScw;
    int nNumCoincidences = -7;
    std::vector<MapPointSN *> vpMPs, vpMatchedMPs;
};
static void show(const char *tag, World &w, int ret, Outputs &o, int next) {
    double S[8];
    ORB_SLAM3::Optimizer::sim3_to8(o.g2oScw, S);
    std::printf("D %s %d %d %d %d %d %d |", tag, ret, o.pMatchedKF2 ? w.ki[o.pMatchedKF2] : -1, o.nNumCoincidences, o.pMatchedKF2 ? (int)o.pMatchedKF2->mbNotErase : -1,
                o.pLastCurrentKF ? w.ki[o.pLastCurrentKF] : -1, next);
    for (double d : S) { uint64_t u; std::memcpy(&u, &d, 8); std::printf(" %016llx", (unsigned long long)u); }
    std::printf(" |"); ids(w, o.vpMPs); std::printf(" |"); ids(w, o.vpMatchedMPs); std::printf("\n");
}

// header (h[5] = mode): 0 as is, 3 the IMU case; then argv[2..]: the thresholds nBoWMatches nBoWInliers nSim3Inliers nProjMatches nProjOptMatches
int main(int argc, char **argv) {
    if (argc < 7) { std::printf("usage: test_place_recognition_facade map.bin nBoWMatches nBoWInliers nSim3Inliers nProjMatches nProjOptMatches\n"); return 2; }
    int32_t h[8];
    World A, B;
    if (!load(argv[1], h, A) || !load(argv[1], h, B)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    Th th;
    th.nBoWMatches = std::atoi(argv[2]); th.nBoWInliers = std::atoi(argv[3]); th.nSim3Inliers = std::atoi(argv[4]); th.nProjMatches = std::atoi(argv[5]);
    th.nProjOptMatches = std::atoi(argv[6]);
    const bool mbFixScale = false;

    using Graph = CovisibilityGraph<KeyFrameSN, MapPointSN>;
    Graph graph(h[0] + 4, h[1] + 64);
    if (!graph.ok()) return 3;
    for (int k = 0; k < h[0]; k++)
        if (graph.Sync(A.kfs[k].get()) != RUMI_OK || graph.SyncFeatures(A.kfs[k].get()) != RUMI_OK) return 3;
    std::vector<MapPointSN *> all;
    for (int i = 0; i < h[1]; i++) {
        if (graph.Sync(A.mps[i].get()) != RUMI_OK) return 3;
        all.push_back(A.mps[i].get());
    }
    if (graph.SyncAttributes(all) != RUMI_OK) return 3;
    if (!ORB_SLAM3::Optimizer::arena()) return 3;                        // the first device calls of the process, before either side seeds rand()
    { std::vector<MapPointSN *> v; ORB_SLAM3::ORBmatcher warm(0.9, true); warm.SearchByBoW(B.cur, B.cand.back(), v); }

    // ---- side A: the member ----
    rumi::LoopClosingStep step;
    ORB_SLAM3::ORBmatcher matcherBoW(0.9, true);
    std::set<KeyFrameSN *> spConnectedKeyFrames;
    for (auto &e : A.cur->mConnectedKeyFrameWeights) spConnectedKeyFrames.insert(e.first);
    Outputs a, b;
    a.vpMPs.assign(2, A.mps[0].get()); a.vpMatchedMPs.assign(2, A.mps[0].get());
    srand(4321);
    rumi_facade::clear_status();
    const int retA = step.DetectCommonRegionsFromBoWResident(graph, A.cur, A.cand, spConnectedKeyFrames, matcherBoW, mbFixScale, h[5] == 3, th, a.pMatchedKF2, a.pLastCurrentKF,
                                                            a.g2oScw, a.nNumCoincidences, a.vpMPs, a.vpMatchedMPs, toSophusMock);
    const int nextA = rand();
    if (retA < 0) {
        const bool same = !a.pMatchedKF2 && !a.pLastCurrentKF && a.nNumCoincidences == -7 && a.vpMPs == std::vector<MapPointSN *>(2, A.mps[0].get()) && a.vpMatchedMPs == a.vpMPs;
        std::printf("R A %d %d %s\n", retA, rumi_facade::last_status(), same ? "untouched" : "TOUCHED");
        print("A", A); print("B", B);
        return 0;
    }
    show("A", A, retA, a, nextA);
    // ---- side B: the text ----
    srand(4321);
    const bool retB = DetectCommonRegionsFromBoW(B, th, mbFixScale, B.cand, b.pMatchedKF2, b.pLastCurrentKF, b.g2oScw, b.nNumCoincidences, b.vpMPs, b.vpMatchedMPs);
    const int nextB = rand();
    show("B", B, retB ? 1 : 0, b, nextB);
    print("A", A); print("B", B);
    return 0;
}
