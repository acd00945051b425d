// LoopClosingStep::SearchByProjectionResident and CovisibleCheckResident (facade/LoopClosingStep.h) over a CovisibilityGraph and the mock data
// model of tests/cpp/mock_model_sim3_projection.h, against the reference's text of LoopClosing.cc:711-738 and :773-795 (with
// DetectCommonRegionsFromLastKF :855-866 and FindMatchesByProjection :868-914) over the per-call rumi_facade::ORBmatcher::SearchByProjection, on a
// copy of the same map, on the GPU.  Reads a map written by tests/test_sim3_projection_facade_gpu.py.  Map A belongs to a graph and takes the
// two members; map B takes the text.  Prints
//   S map c n716 n738 | vpMatchedMP ids | vpMatchedKF ids | the second vpMatchedMP ids        per candidate
//   C map visited nNumKFs | vpMapPoints ids      and   N B the count of every covisible the text searched
//   R A ret status | the pre-filled outputs                                                    a refused call
//   K / P map ...                                                                              the map, as tests/cpp/test_search_and_fuse_facade.cc prints it
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

#include "mock_model_sim3_projection.h"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

struct World {
    MapKR map;
    std::vector<std::unique_ptr<KeyFrameSN>> kfs;
    std::vector<std::unique_ptr<MapPointSN>> mps;
    KeyFrameSN *cur = nullptr;
    std::vector<KeyFrameSN *> cand;
    float sim3[8];                                                 // of the current key-frame: q xyzw, t, s
    std::map<const void *, int> pi, ki;
};

// header: n_kf n_pts nleftKf unsyncedKf unseenPoint mode (0: as is, 2: 641 jobs) cur n_cand
static bool load(const char *path, int32_t *h, World &w) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    if (!rd(f, h, 8)) return false;
    std::vector<std::vector<int32_t>> cov(h[0]);
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameSN> kf(new KeyFrameSN());
        int32_t n, nc;
        float T7[7];
        if (!rd(f, &n, 1) || !rd(f, T7, 7)) return false;
        kf->N = n; kf->mnId = k + 1; kf->map = &w.map; kf->mTimeStamp = k;
        kf->mvKeysUn.resize(n);
        kf->mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
        std::vector<int32_t> row(n);
        static_assert(sizeof(cv::KeyPoint) == 28, "the file holds 28-byte key-points");
        if (!rd(f, kf->mvKeysUn.data(), n) || !rd(f, kf->mDescriptors.ptr(0), (size_t)n * 32) || !rd(f, row.data(), n)) return false;
        if (!rd(f, &nc, 1)) return false;
        cov[k].resize(nc);
        if (!rd(f, cov[k].data(), nc)) return false;
        kf->mvScaleFactors.assign(8, 1.f);
        for (int l = 1; l < 8; l++) kf->mvScaleFactors[l] = kf->mvScaleFactors[l - 1] * 1.2f;
        kf->mnScaleLevels = 8; kf->mfLogScaleFactor = std::log(1.2f);
        kf->fx = kf->fy = 500.f; kf->cx = 320.f; kf->cy = 240.f;
        kf->cam.fx = kf->cam.fy = 500.f; kf->cam.cx = 320.f; kf->cam.cy = 240.f;
        kf->pose = Sophus::SE3f(Eigen::Quaternionf(T7[3], T7[0], T7[1], T7[2]), Eigen::Vector3f(T7[4], T7[5], T7[6]));
        kf->mvuRight.assign(n, -1.f);
        kf->mvpMapPoints.assign(n, nullptr);
        if (k == h[2]) kf->NLeft = 0;
        w.kfs.push_back(std::move(kf));
        for (int i = 0; i < n; i++) w.kfs.back()->mvpMapPoints[i] = reinterpret_cast<MapPoint *>((intptr_t)(row[i] + 1));   // ids for now
    }
    for (int k = 0; k < h[0]; k++) {
        std::vector<KeyFrameSN *> ord;
        std::map<KeyFrameSN *, int> wts;
        std::vector<int> ws;
        for (size_t i = 0; i < cov[k].size(); i++) {
            if (cov[k][i] < 0 || cov[k][i] >= h[0]) return false;
            ord.push_back(w.kfs[cov[k][i]].get()); wts[ord.back()] = 100 - (int)i; ws.push_back(100 - (int)i);
        }
        w.kfs[k]->SetCovisibility(wts, ord, ws);
    }
    std::vector<int32_t> cand(h[7]);
    if (!rd(f, w.sim3, 8) || !rd(f, cand.data(), cand.size()) || h[6] < 0 || h[6] >= h[0]) return false;
    w.cur = w.kfs[h[6]].get();
    for (int32_t c : cand) { if (c < 0 || c >= h[0]) return false; w.cand.push_back(w.kfs[c].get()); }
    for (int i = 0; i < h[1]; i++) {
        std::unique_ptr<MapPointSN> p(new MapPointSN());
        float a[8];
        int32_t bad;
        p->desc.create(1, 32, CV_8U);
        if (!rd(f, a, 8) || !rd(f, p->desc.ptr(0), 32) || !rd(f, &bad, 1)) return false;
        p->pos = Eigen::Vector3f(a[0], a[1], a[2]); p->normal = Eigen::Vector3f(a[3], a[4], a[5]); p->minD = a[6]; p->maxD = a[7];
        p->bad = bad != 0; p->map = &w.map; p->nObs = 0;
        w.mps.push_back(std::move(p));
    }
    std::fclose(f);
    for (auto &kf : w.kfs)
        for (int i = 0; i < kf->N; i++) {
            const intptr_t id = reinterpret_cast<intptr_t>(kf->mvpMapPoints[i]) - 1;
            MapPointSN *p = id >= 0 ? w.mps[id].get() : nullptr;
            kf->mvpMapPoints[i] = p;
            if (p && !p->bad) { p->obs[kf.get()] = std::make_tuple(i, -1); p->nObs++; if (!p->mpRefKF) p->mpRefKF = kf.get(); }
        }
    for (size_t i = 0; i < w.mps.size(); i++) w.pi[w.mps[i].get()] = (int)i;
    for (size_t k = 0; k < w.kfs.size(); k++) w.ki[w.kfs[k].get()] = (int)k;
    return true;
}

static void print(const char *tag, World &w) {
    for (size_t k = 0; k < w.kfs.size(); k++) {
        std::printf("K %s %zu |", tag, k);
        for (MapPoint *p : w.kfs[k]->mvpMapPoints) std::printf(" %d", p ? w.pi[p] : -1);
        std::printf("\n");
    }
    for (size_t i = 0; i < w.mps.size(); i++) {
        MapPointSN *p = w.mps[i].get();
        std::map<int, int> o;
        for (auto &e : p->obs) o[w.ki[e.first]] = std::get<0>(e.second);
        std::printf("P %s %zu %d %d %zu", tag, i, (int)p->bad, p->mpReplaced ? w.pi[p->mpReplaced] : -1, o.size());
        for (auto &e : o) std::printf(" %d %d", e.first, e.second);
        std::printf(" | ");
        for (int b = 0; b < 32; b++) std::printf("%02x", p->desc.ptr(0)[b]);
        std::printf("\n");
    }
}

static void ids(World &w, const std::vector<MapPointSN *> &v) { for (MapPointSN *p : v) std::printf(" %d", p ? w.pi[p] : -1); }
static void ids(World &w, const std::vector<KeyFrameSN *> &v) { for (KeyFrameSN *k : v) std::printf(" %d", k ? w.ki[k] : -1); }

// What reaches :716 for a candidate: the points of the candidate and of its covisibles, each with the key-frame it was found in (:655-700)
static void candidate_points(KeyFrameSN *pKFi, std::vector<MapPointSN *> &vpMapPoints, std::vector<KeyFrameSN *> &vpKeyFrames) {
    std::vector<KeyFrameSN *> vpCovKFi = pKFi->GetBestCovisibilityKeyFrames(5);
    vpCovKFi.insert(vpCovKFi.begin(), pKFi);
    std::set<MapPointSN *> spMapPoints;
    for (KeyFrameSN *pCovKFi : vpCovKFi)
        for (MapPointSN *pCovMPij : pCovKFi->GetMapPointMatches()) {
            if (!pCovMPij || pCovMPij->isBad()) continue;
            if (spMapPoints.find(pCovMPij) == spMapPoints.end()) { spMapPoints.insert(pCovMPij); vpMapPoints.push_back(pCovMPij); vpKeyFrames.push_back(pCovKFi); }
        }
}

static Sophus::Sim3f scw_of(const World &w, int c) {                // the Sim3 estimate of candidate c: the current key-frame's, nudged
    const float *a = w.sim3;
    return Sophus::Sim3f(Eigen::Quaternionf(a[3], a[0], a[1], a[2]).toRotationMatrix(), Eigen::Vector3f(a[4] + 0.01f * c, a[5] - 0.005f * c, a[6]), a[7]);
}
static g2o::Sim3 gscw_of(const World &w) {
    const float *a = w.sim3;
    return g2o::Sim3(Eigen::Quaterniond(a[3], a[0], a[1], a[2]), Eigen::Vector3d(a[4], a[5], a[6]), (double)a[7]);
}

// LoopClosing.cc:868-914 as written, over the facade's SearchByProjection
static int FindMatchesByProjection(World &w, KeyFrameSN *pCurrentKF, KeyFrameSN *pMatchedKFw, g2o::Sim3 &g2oScw, std::set<MapPointSN *> &spMatchedMPinOrigin,
                                   std::vector<MapPointSN *> &vpMapPoints, std::vector<MapPointSN *> &vpMatchedMapPoints) {
    int nNumCovisibles = 10;
    std::vector<KeyFrameSN *> vpCovKFm = pMatchedKFw->GetBestCovisibilityKeyFrames(nNumCovisibles);
    int nInitialCov = vpCovKFm.size();
    vpCovKFm.push_back(pMatchedKFw);
    std::set<KeyFrameSN *> spCheckKFs(vpCovKFm.begin(), vpCovKFm.end());
    std::set<KeyFrameSN *> spCurrentCovisbles;
    for (auto &e : pCurrentKF->mConnectedKeyFrameWeights) spCurrentCovisbles.insert(e.first);       // GetConnectedKeyFrames()
    if (nInitialCov < nNumCovisibles) {
        for (int i = 0; i < nInitialCov; ++i) {
            std::vector<KeyFrameSN *> vpKFs = vpCovKFm[i]->GetBestCovisibilityKeyFrames(nNumCovisibles);
            int nInserted = 0;
            size_t j = 0;
            while (j < vpKFs.size() && nInserted < nNumCovisibles) {
                if (spCheckKFs.find(vpKFs[j]) == spCheckKFs.end() && spCurrentCovisbles.find(vpKFs[j]) == spCurrentCovisbles.end()) {
                    spCheckKFs.insert(vpKFs[j]);
                    ++nInserted;
                }
                ++j;
            }
            vpCovKFm.insert(vpCovKFm.end(), vpKFs.begin(), vpKFs.end());
        }
    }
    std::set<MapPointSN *> spMapPoints;
    vpMapPoints.clear();
    vpMatchedMapPoints.clear();
    for (KeyFrameSN *pKFi : vpCovKFm) {
        for (MapPointSN *pMPij : pKFi->GetMapPointMatches()) {
            if (!pMPij || pMPij->isBad()) continue;
            if (spMapPoints.find(pMPij) == spMapPoints.end()) { spMapPoints.insert(pMPij); vpMapPoints.push_back(pMPij); }
        }
    }
    Sophus::Sim3f mScw = toSophusMock(g2oScw);
    rumi::LoopClosingStep matcher;
    vpMatchedMapPoints.resize(pCurrentKF->GetMapPointMatches().size(), static_cast<MapPointSN *>(NULL));
    int num_matches = matcher.SearchByProjection(pCurrentKF, mScw, vpMapPoints, vpMatchedMapPoints, 3, 1.5);
    return num_matches;
}

// :855-866
static bool DetectCommonRegionsFromLastKF(World &w, KeyFrameSN *pCurrentKF, KeyFrameSN *pMatchedKF, g2o::Sim3 &gScw, int &nNumProjMatches,
                                          std::vector<MapPointSN *> &vpMPs, std::vector<MapPointSN *> &vpMatchedMPs) {
    std::set<MapPointSN *> spAlreadyMatchedMPs(vpMatchedMPs.begin(), vpMatchedMPs.end());
    nNumProjMatches = FindMatchesByProjection(w, pCurrentKF, pMatchedKF, gScw, spAlreadyMatchedMPs, vpMPs, vpMatchedMPs);
    int nProjMatches = 30;
    if (nNumProjMatches >= nProjMatches) return true;
    return false;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_sim3_projection_facade map.bin\n"); return 2; }
    int32_t h[8];
    World A, B;
    if (!load(argv[1], h, A) || !load(argv[1], h, B)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    const int mode = h[5];

    using Graph = CovisibilityGraph<KeyFrameSN, MapPointSN>;
    Graph graph(h[0] + 4, h[1] + 64);
    if (!graph.ok()) return 3;
    for (int k = 0; k < h[0]; k++)
        if (k != h[3] && (graph.Sync(A.kfs[k].get()) != RUMI_OK || graph.SyncFeatures(A.kfs[k].get()) != RUMI_OK)) return 3;
    std::vector<MapPointSN *> all;
    for (int i = 0; i < h[1]; i++) {
        if (i == h[4]) continue;                                   // a point the graph is never given
        if (graph.Sync(A.mps[i].get()) != RUMI_OK) return 3;
        all.push_back(A.mps[i].get());
    }
    if (graph.SyncAttributes(all) != RUMI_OK) return 3;

    using Job = rumi::LoopClosingStep::Sim3ProjectionJob<KeyFrameSN, MapPointSN>;
    rumi::LoopClosingStep step;
    const size_t nC = A.cand.size();
    // ---- :711-738 for every candidate: map A in one call
    std::vector<std::vector<MapPointSN *>> ptsA(nC), m1(nC), m2(nC);
    std::vector<std::vector<KeyFrameSN *>> kfsA(nC), k1(nC);
    std::vector<int> n1(nC, -7), n2(nC, -7);
    std::vector<Job> jobs;
    for (size_t c = 0; c < nC; c++) {
        candidate_points(A.cand[c], ptsA[c], kfsA[c]);
        if (h[4] >= 0 && (int)c == 0 && !A.mps[h[4]]->obs.size()) ptsA[c].push_back(A.mps[h[4]].get()), kfsA[c].push_back(A.cand[c]);   // a point no key-frame holds
        m1[c].assign(3, A.mps[0].get()); m2[c].assign(3, A.mps[0].get()); k1[c].assign(3, A.cur);                                   // pre-filled: a refusal leaves them
        jobs.push_back(Job{A.cur, scw_of(A, (int)c), &ptsA[c], &kfsA[c], 8, 1.5f, &m1[c], &k1[c], &n1[c]});
        jobs.push_back(Job{A.cur, scw_of(A, (int)c), &ptsA[c], nullptr, 5, 1.0f, &m2[c], nullptr, &n2[c]});
    }
    if (mode == 2) while (jobs.size() <= (size_t)RUMI_FUSE_MAX_TARGETS) jobs.push_back(jobs[jobs.size() % 2]);
    rumi_facade::clear_status();
    int ret = step.SearchByProjectionResident(graph, jobs);
    const int status = rumi_facade::last_status();
    // ---- :773-795 for the first candidate
    std::vector<MapPointSN *> vpMapPointsA = ptsA.empty() ? std::vector<MapPointSN *>() : ptsA[0];
    const std::vector<MapPointSN *> before = vpMapPointsA;
    int nNumKFsA = 0;
    std::vector<KeyFrameSN *> covA = A.cur->GetBestCovisibilityKeyFrames(10);
    if (mode == 2) while (covA.size() <= (size_t)RUMI_FUSE_MAX_TARGETS) covA.push_back(covA[covA.size() % 3]);
    rumi_facade::clear_status();
    const int visited = step.CovisibleCheckResident(graph, A.cur, A.cand[0], gscw_of(A), covA, vpMapPointsA, &nNumKFsA, toSophusMock);
    const int status2 = rumi_facade::last_status();
    if (ret < 0 || visited < 0) {
        std::printf("R A %d %d %d %d |", ret, status, visited, status2);
        bool same = visited >= 0 || (vpMapPointsA == before && nNumKFsA == 0);      // (a point no key-frame holds reaches only the first member)
        if (ret >= 0) same = false;                                 // every refusal of this test refuses the first member
        for (size_t c = 0; c < nC; c++)
            same = same && m1[c] == std::vector<MapPointSN *>(3, A.mps[0].get()) && m2[c] == m1[c] && k1[c] == std::vector<KeyFrameSN *>(3, A.cur) && n1[c] == -7 && n2[c] == -7;
        std::printf(" %s\n", same ? "untouched" : "TOUCHED");
        print("A", A);
        print("B", B);
        return 0;
    }
    for (size_t c = 0; c < nC; c++) {
        std::printf("S A %zu %d %d |", c, n1[c], n2[c]); ids(A, m1[c]); std::printf(" |"); ids(A, k1[c]); std::printf(" |"); ids(A, m2[c]); std::printf("\n");
    }
    std::printf("C A %d %d |", visited, nNumKFsA); ids(A, vpMapPointsA); std::printf("\n");

    // ---- map B: the text
    rumi::LoopClosingStep matcher;
    KeyFrameSN *mpCurrentKF = B.cur;
    for (size_t c = 0; c < nC; c++) {
        std::vector<MapPointSN *> vpMapPoints;
        std::vector<KeyFrameSN *> vpKeyFrames;
        candidate_points(B.cand[c], vpMapPoints, vpKeyFrames);
        Sophus::Sim3f mScw = scw_of(B, (int)c);
        std::vector<MapPointSN *> vpMatchedMP;                      // :711-716
        vpMatchedMP.resize(mpCurrentKF->GetMapPointMatches().size(), static_cast<MapPointSN *>(NULL));
        std::vector<KeyFrameSN *> vpMatchedKF;
        vpMatchedKF.resize(mpCurrentKF->GetMapPointMatches().size(), static_cast<KeyFrameSN *>(NULL));
        int numProjMatches = matcher.SearchByProjection(mpCurrentKF, mScw, vpMapPoints, vpKeyFrames, vpMatchedMP, vpMatchedKF, 8, 1.5);
        std::vector<MapPointSN *> vpMatchedMP2;                     // :735-738
        vpMatchedMP2.resize(mpCurrentKF->GetMapPointMatches().size(), static_cast<MapPointSN *>(NULL));
        int numProjOptMatches = matcher.SearchByProjection(mpCurrentKF, mScw, vpMapPoints, vpMatchedMP2, 5, 1.0);
        std::printf("S B %zu %d %d |", c, numProjMatches, numProjOptMatches); ids(B, vpMatchedMP); std::printf(" |"); ids(B, vpMatchedKF); std::printf(" |"); ids(B, vpMatchedMP2);
        std::printf("\n");
    }
    {
        std::vector<MapPointSN *> vpMapPoints, unusedKFpts;
        std::vector<KeyFrameSN *> vpKeyFrames;
        candidate_points(B.cand[0], vpMapPoints, vpKeyFrames);
        KeyFrameSN *pMostBoWMatchesKF = B.cand[0];
        g2o::Sim3 gScw = gscw_of(B);
        int nNumKFs = 0;                                            // :768-795
        std::vector<KeyFrameSN *> vpCurrentCovKFs = mpCurrentKF->GetBestCovisibilityKeyFrames(10);
        size_t j = 0;
        std::printf("N B");
        while (nNumKFs < 3 && j < vpCurrentCovKFs.size()) {
            KeyFrameSN *pKFj = vpCurrentCovKFs[j];
            const Sophus::SE3f Tjc = pKFj->GetPose() * mpCurrentKF->GetPoseInverse();
            const auto q = Tjc.unit_quaternion(); const auto t = Tjc.translation();
            g2o::Sim3 gSjc(Eigen::Quaterniond(q.w(), q.x(), q.y(), q.z()), Eigen::Vector3d(t(0), t(1), t(2)), 1.0);      // mTjc = (...).cast<double>()
            g2o::Sim3 gSjw = gSjc * gScw;
            int numProjMatches_j = 0;
            std::vector<MapPointSN *> vpMatchedMPs_j;
            bool bValid = DetectCommonRegionsFromLastKF(B, pKFj, pMostBoWMatchesKF, gSjw, numProjMatches_j, vpMapPoints, vpMatchedMPs_j);
            std::printf(" %d", numProjMatches_j);
            if (bValid) nNumKFs++;
            j++;
        }
        std::printf(" of %zu\n", vpCurrentCovKFs.size());
        std::printf("C B %zu %d |", j, nNumKFs); ids(B, vpMapPoints); std::printf("\n");
    }
    print("A", A);
    print("B", B);
    return 0;
}
