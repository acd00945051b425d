// rumi_facade::Relocalization (rumi_slam_amd/facade/TrackingStep.h) over a mock data model and a scripted solver, against a per-hypothesis replay
// of the single-entry facade members -- ORBmatcher::SearchByBoW(pKF, F), Optimizer::PoseOptimization(&F), ORBmatcher::SearchByProjection(F, pKF,
// sFound, th, ORBdist) -- in the control flow of Tracking.cc:3226-3348 on a copy of the same frame.  Equal afterwards: the return value, mvpMapPoints,
// mvbOutlier (the layers earlier hypotheses and earlier stages left included) and the pose, with speculateRound on and off; the scripted solver
// counts how often each candidate's step ran.
//
// The scene: the frame the tracker extracted from the image given on the command line, one true pose, map points that are back-projections of
// frame features.  A candidate key-frame copies some of the frame's features: those under FeatureVector node 1 are found by the BoW search (the
// frame keeps all its features under node 1), those under node 2 are not and wait for the projection search.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "ORBextractor.h"
#include "ORBmatcher.h"
#include "Optimizer.h"
#include "TrackingStep.h"
#include "rumi_status.h"

struct V3f { float v[3]; float operator()(int i) const { return v[i]; } };
struct Q4f { float q[4]; float x() const { return q[0]; } float y() const { return q[1]; } float z() const { return q[2]; } float w() const { return q[3]; } };
struct SE3f { float T[7]; Q4f unit_quaternion() const { return Q4f{{T[0], T[1], T[2], T[3]}}; } V3f translation() const { return V3f{{T[4], T[5], T[6]}}; } };
struct MapPoint {
    static std::mutex mGlobalMutex;
    V3f pos{{0, 0, 0}}, normal{{0, 0, 1}}; cv::Mat desc; bool bad = false; float minD = 0.1f, maxD = 60.f;
    V3f GetWorldPos() { return pos; }
    V3f GetNormal() { return normal; }
    cv::Mat GetDescriptor() { return desc; }
    int Observations() { return 1; }
    bool isBad() { return bad; }
    float GetMinDistance() { return minD; }
    float GetMaxDistance() { return maxD; }
    bool mbTrackInView = false, mbTrackInViewR = false; float mTrackProjX = 0, mTrackProjY = 0, mTrackViewCos = 1, mTrackDepth = 1; int mnTrackScaleLevel = 0;
    long mnLastFrameSeen = -1;
};
std::mutex MapPoint::mGlobalMutex;
struct Frame {
    int N = 0; long mnId = 7;
    std::vector<cv::KeyPoint> mvKeysUn; cv::Mat mDescriptors; std::vector<MapPoint *> mvpMapPoints; std::vector<bool> mvbOutlier;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2, mvuRight;
    float mnMinX = 0, mnMinY = 0, mnMaxX = 640, mnMaxY = 480, fx = 535.4f, fy = 539.2f, cx = 320.1f, cy = 247.6f;
    SE3f pose{{0, 0, 0, 1, 0, 0, 0}};
    float mfLogScaleFactor = std::log(1.2f); int mnScaleLevels = 8;
    std::map<unsigned, std::vector<unsigned>> mFeatVec;
    SE3f GetPose() const { return pose; }
    void SetPoseFromQuatTrans(const float *T7) { std::memcpy(pose.T, T7, 28); }
};
struct KeyFrame : Frame {
    bool bad = false;
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    bool isBad() { return bad; }
};

static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); fails++; } } while (0)

static const double kTrue[7] = {0.02, -0.03, 0.01, 1.0, 0.10, -0.05, 0.20};
static const double kNear[7] = {0.021, -0.0295, 0.0108, 1.0, 0.104, -0.053, 0.197};
static void pose7(const double *in, float *T7) {
    const double n = std::sqrt(in[0] * in[0] + in[1] * in[1] + in[2] * in[2] + in[3] * in[3]);
    for (int i = 0; i < 4; i++) T7[i] = (float)(in[i] / n);
    for (int i = 4; i < 7; i++) T7[i] = (float)in[i];
}
// the world point that the true pose projects onto (u, v) at depth z
static V3f backproject(const Frame &F, double u, double v, double z) {
    float T[7];
    pose7(kTrue, T);
    const double x = T[0], y = T[1], zq = T[2], w = T[3];
    const double R[9] = {1 - 2 * (y * y + zq * zq), 2 * (x * y - zq * w), 2 * (x * zq + y * w), 2 * (x * y + zq * w), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - x * w),
                         2 * (x * zq - y * w), 2 * (y * zq + x * w), 1 - 2 * (x * x + y * y)};
    const double c[3] = {(u - F.cx) / F.fx * z - T[4], (v - F.cy) / F.fy * z - T[5], z - T[6]};
    return V3f{{(float)(R[0] * c[0] + R[3] * c[1] + R[6] * c[2]), (float)(R[1] * c[0] + R[4] * c[1] + R[7] * c[2]), (float)(R[2] * c[0] + R[5] * c[1] + R[8] * c[2])}};
}

// a key-frame that copies the frame's features `bow` (FeatureVector node 1) and `planted` (node 2), each with a clean map point
static KeyFrame *make_kf(const Frame &F, const std::vector<int> &bow, const std::vector<int> &planted) {
    KeyFrame *k = new KeyFrame();
    k->mvScaleFactors = F.mvScaleFactors; k->mvInvLevelSigma2 = F.mvInvLevelSigma2;
    std::vector<int> all(bow);
    all.insert(all.end(), planted.begin(), planted.end());
    k->N = (int)all.size();
    k->mDescriptors.create(k->N, 32, CV_8U);
    for (int j = 0; j < k->N; j++) {
        const int f = all[j];
        k->mvKeysUn.push_back(F.mvKeysUn[f]);
        std::memcpy(k->mDescriptors.ptr(j), F.mDescriptors.ptr(f), 32);
        MapPoint *p = new MapPoint();
        const double z = 2.0 + std::fmod(f * 0.6180339887, 1.0) * 4.0;
        p->pos = backproject(F, F.mvKeysUn[f].pt.x, F.mvKeysUn[f].pt.y, z);
        p->desc.create(1, 32, CV_8U);
        std::memcpy(p->desc.ptr(0), F.mDescriptors.ptr(f), 32);
        const double xn = (F.mvKeysUn[f].pt.x - F.cx) / F.fx, yn = (F.mvKeysUn[f].pt.y - F.cy) / F.fy, dist = z * std::sqrt(1 + xn * xn + yn * yn);
        p->maxD = (float)(dist * std::pow(1.2, F.mvKeysUn[f].octave - 0.5));          // PredictScale = ceil(octave - 0.5): the feature's octave
        p->minD = 0.05f;
        k->mvpMapPoints.push_back(p);
        k->mFeatVec[j < (int)bow.size() ? 1u : 2u].push_back((unsigned)j);
    }
    k->mvbOutlier.assign(k->N, false);
    return k;
}

struct Step { bool bTcw, bNoMore; const double *pose; int nInl; };
struct Solver {
    std::vector<Step> script; size_t at = 0; int calls = 0;
    std::vector<int> matched;                                // the frame features the BoW search gave this candidate
};
static Solver *bind_solver(Solver *s, const Frame &F, const std::vector<MapPoint *> &m) {
    s->at = 0; s->calls = 0; s->matched.clear();
    for (int f = 0; f < F.N; f++) if (m[f]) s->matched.push_back(f);
    return s;
}
static bool solver_step(Solver *s, int N, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, float *T7) {
    s->calls++;
    const Step st = s->script[s->at < s->script.size() ? s->at : s->script.size() - 1];
    s->at++;
    bNoMore = st.bNoMore;
    vbInliers.assign(N, false);
    nInliers = 0;
    for (int k = 0; k < st.nInl && k < (int)s->matched.size(); k++) { vbInliers[s->matched[k]] = true; nInliers++; }
    if (st.bTcw) pose7(st.pose, T7);
    return st.bTcw;
}

// Tracking.cc:3226-3348 over the single-entry facade members
static bool reference(Frame &F, const std::vector<KeyFrame *> &cands, std::vector<Solver> &solvers) {
    const int nKFs = (int)cands.size();
    ORB_SLAM3::ORBmatcher matcher(0.75f, true);
    std::vector<std::vector<MapPoint *>> vvp(nKFs);
    std::vector<bool> vbDiscarded(nKFs, false);
    std::vector<Solver *> vpSolvers(nKFs, nullptr);
    int nCandidates = 0;
    for (int i = 0; i < nKFs; i++) {
        if (cands[i]->isBad()) { vbDiscarded[i] = true; continue; }
        const int nm = matcher.SearchByBoW(cands[i], F, vvp[i]);
        if (nm < 15) { vbDiscarded[i] = true; continue; }
        vpSolvers[i] = bind_solver(&solvers[i], F, vvp[i]);
        nCandidates++;
    }
    bool bMatch = false;
    ORB_SLAM3::ORBmatcher matcher2(0.9f, true);
    while (nCandidates > 0 && !bMatch) {
        for (int i = 0; i < nKFs; i++) {
            if (vbDiscarded[i]) continue;
            std::vector<bool> vbInliers; int nInliers; bool bNoMore; float T7[7];
            const bool bTcw = solver_step(vpSolvers[i], F.N, bNoMore, vbInliers, nInliers, T7);
            if (bNoMore) { vbDiscarded[i] = true; nCandidates--; }
            if (!bTcw) continue;
            F.SetPoseFromQuatTrans(T7);
            std::set<MapPoint *> sFound;
            for (int j = 0; j < (int)vbInliers.size(); j++) {
                if (vbInliers[j]) { F.mvpMapPoints[j] = vvp[i][j]; sFound.insert(vvp[i][j]); }
                else F.mvpMapPoints[j] = nullptr;
            }
            int nGood = ORB_SLAM3::Optimizer::PoseOptimization(&F);
            if (nGood < 10) continue;
            for (int io = 0; io < F.N; io++) if (F.mvbOutlier[io]) F.mvpMapPoints[io] = nullptr;
            if (nGood < 50) {
                int nadditional = matcher2.SearchByProjection(F, cands[i], sFound, 10, 100);
                if (nadditional + nGood >= 50) {
                    nGood = ORB_SLAM3::Optimizer::PoseOptimization(&F);
                    if (nGood > 30 && nGood < 50) {
                        sFound.clear();
                        for (int ip = 0; ip < F.N; ip++) if (F.mvpMapPoints[ip]) sFound.insert(F.mvpMapPoints[ip]);
                        nadditional = matcher2.SearchByProjection(F, cands[i], sFound, 3, 64);
                        if (nGood + nadditional >= 50) {
                            nGood = ORB_SLAM3::Optimizer::PoseOptimization(&F);
                            for (int io = 0; io < F.N; io++) if (F.mvbOutlier[io]) F.mvpMapPoints[io] = nullptr;
                        }
                    }
                }
            }
            if (nGood >= 50) { bMatch = true; break; }
        }
    }
    return bMatch;
}

static bool same_frame(const Frame &a, const Frame &b) {
    return a.mvpMapPoints == b.mvpMapPoints && a.mvbOutlier == b.mvbOutlier && std::memcmp(a.pose.T, b.pose.T, 28) == 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_reloc_facade frame.bin (640x480 u8)\n"); return 2; }
    std::vector<uint8_t> im(640 * 480);
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f || std::fread(im.data(), 1, im.size(), f) != im.size()) { std::printf("cannot read %s\n", argv[1]); return 2; }
        std::fclose(f);
    }
    ORB_SLAM3::ORBextractor ext(1000, 1.2f, 8, 20, 7);
    Frame F0;
    cv::Mat image(480, 640, CV_8U, im.data(), 640);
    CHECK(rumi_facade::ExtractFrame(F0, image, ext) >= 0 && F0.N > 600, "ExtractFrame");
    if (fails) return 1;
    F0.mvScaleFactors = ext.GetScaleFactors(); F0.mvInvLevelSigma2 = ext.GetInverseScaleSigmaSquares();
    F0.mvuRight.assign(F0.N, -1.f);
    for (int f = 0; f < F0.N; f++) F0.mFeatVec[1].push_back((unsigned)f);
    for (int f = 0; f < F0.N; f += 5) F0.mvbOutlier[f] = true;          // stale flags of earlier stages: only PoseOptimization's writes may change them
    // features a key-frame may copy: inside the image, descriptor unique in the frame
    std::vector<int> pool;
    for (int f = 0; f < F0.N; f++) {
        const cv::KeyPoint &k = F0.mvKeysUn[f];
        if (k.pt.x < 70 || k.pt.x > 570 || k.pt.y < 70 || k.pt.y > 410) continue;
        bool unique = true;
        for (int g = 0; g < F0.N && unique; g++) unique = g == f || std::memcmp(F0.mDescriptors.ptr(f), F0.mDescriptors.ptr(g), 32) != 0;
        if (unique) pool.push_back(f);
    }
    CHECK(pool.size() >= 220, "enough features to build the key-frames from");
    if (fails) return 1;
    size_t at = 0;
    auto take = [&](int n) { std::vector<int> v(pool.begin() + at, pool.begin() + at + n); at += n; return v; };
    KeyFrame *kfWinP1 = make_kf(F0, take(60), {}), *kfWinS1 = make_kf(F0, take(30), take(25)), *kfLose = make_kf(F0, take(20), {}), *kfFew = make_kf(F0, take(10), {}),
             *kfBad = make_kf(F0, take(20), {}), *kfLose2 = make_kf(F0, take(20), {});
    kfBad->bad = true;

    struct Scenario { const char *name; std::vector<KeyFrame *> cands; std::vector<std::vector<Step>> scripts; bool want; std::vector<int> stepsSpec, stepsSeq; int winner; };
    const Step none{false, false, kTrue, 0};
    std::vector<Scenario> scenarios = {
        {"second round, S1 + P2 wins; the candidate behind it has iterated under speculation",
         {kfLose, kfBad, kfWinS1, kfFew, kfWinP1},
         {{{true, false, kNear, 20}, {true, true, kTrue, 20}}, {}, {none, {true, false, kNear, 30}}, {}, {none, {true, false, kTrue, 60}}},
         true, {2, 0, 2, 0, 2}, {2, 0, 2, 0, 1}, 2},
        {"first round, P1 wins at once", {kfWinP1, kfLose}, {{{true, false, kNear, 60}}, {{true, false, kTrue, 20}}}, true, {1, 1}, {1, 0}, 0},
        {"every candidate runs out: false, the frame as the last hypothesis left it",
         {kfLose, kfLose2}, {{{true, false, kTrue, 20}, {true, true, kNear, 20}}, {none, {true, true, kNear, 20}}}, false, {2, 2}, {2, 2}, -1},
        {"no live candidate", {kfBad, kfFew}, {{}, {}}, false, {0, 0}, {0, 0}, -1},
    };
    for (const Scenario &S : scenarios) {
        std::vector<Solver> refSolvers(S.cands.size());
        for (size_t i = 0; i < S.cands.size(); i++) refSolvers[i].script = S.scripts[i];
        Frame Fr = F0;
        const bool refOk = reference(Fr, S.cands, refSolvers);
        CHECK(refOk == S.want, S.name);
        for (int spec = 1; spec >= 0; spec--) {
            std::vector<Solver> solvers(S.cands.size());
            std::vector<int> live;
            for (size_t i = 0; i < S.cands.size(); i++) { solvers[i].script = S.scripts[i]; }
            Frame Fd = F0;
            size_t made = 0;
            std::vector<Solver *> order;                     // make() is called for the live candidates in order
            for (size_t i = 0; i < S.cands.size(); i++) if (refSolvers[i].calls > 0 || !refSolvers[i].matched.empty()) order.push_back(&solvers[i]);
            auto make = [&](Frame &Fx, const std::vector<MapPoint *> &m) { return bind_solver(order[made++], Fx, m); };
            auto step = [&](Solver *s, bool &bNoMore, std::vector<bool> &inl, int &nInl, float *T7) { return solver_step(s, Fd.N, bNoMore, inl, nInl, T7); };
            rumi_facade::TrackStep st;
            const bool ok = rumi_facade::Relocalization(Fd, S.cands, make, step, &st, spec != 0);
            CHECK(ok == refOk, S.name);
            CHECK(same_frame(Fd, Fr), "mvpMapPoints, mvbOutlier (layers included) and pose == the per-hypothesis replay of the single entries");
            const std::vector<int> &want = spec ? S.stepsSpec : S.stepsSeq;
            bool steps = true;
            for (size_t i = 0; i < S.cands.size(); i++) steps &= solvers[i].calls == want[i];
            CHECK(steps, spec ? "solver steps with speculateRound" : "solver steps without speculateRound: exactly the reference's");
            if (!spec) for (size_t i = 0; i < S.cands.size(); i++) CHECK(solvers[i].calls == refSolvers[i].calls, "sequential == reference solver calls");
            CHECK(st.relocWinner == S.winner && made == order.size(), "winner and make() calls");
            if (S.winner >= 0) CHECK(st.relocGood >= 50, "nGood of the winner");
            if (spec && S.winner == 2) CHECK(st.relocRefines == 2 && st.relocRounds == 2 && st.relocHypotheses == 4, "one refine call a round");
            if (!spec && S.winner == 2) CHECK(st.relocRefines == 3 && st.relocRounds == 2, "one refine call a hypothesis");
        }
        if (S.winner == 2) {
            int held = 0, flagged = 0;
            for (int f = 0; f < Fr.N; f++) { held += Fr.mvpMapPoints[f] != nullptr; flagged += Fr.mvbOutlier[f]; }
            CHECK(held == 55 && flagged > 100, "the S1 winner holds its 30 + 25 points; stale outlier flags elsewhere survive");
        }
    }
    std::printf(fails ? "%d checks failed\n" : "reloc facade ok\n", fails);
    return fails ? 1 : 0;
}
