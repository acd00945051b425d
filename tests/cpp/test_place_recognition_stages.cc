// Sim3RansacStage and OptimizeSim3Stage (facade/PlaceRecognitionStages.h) against the reference's text of LoopClosing.cc:655-676 and :728 over the
// per-candidate members -- the Sim3Solver shell (facade/shells/Sim3Solver.cc on rumi_sim3_ransac) and Optimizer::OptimizeSim3 (facade/Optimizer.h on
// rumi_optimize_sim3) -- on the GPU, over the mock data model of tests/cpp/ref_decls.  Both sides start with srand reset.  Five candidates:
//   0  converges; every fifth match was found in a covisible of the candidate (vpKeyFrameMatchedMP), whose key-point sits at another octave
//   1  below nBoWMatches: no solver
//   2  almost only wrong matches: the solver uses all of its mRansacMaxIts
//   3  converges, fewer correspondences
//   4  fewer correspondences than nBoWInliers: bNoMore at once, nothing drawn
// Equal afterwards: bConverge, nInliers, vbInliers, the estimated R, t, s (bytes), the next rand(); then per converged candidate the return value of
// OptimizeSim3, g2oS12 (bytes) and vpMatches1.
#define RUMI_HAVE_SOPHUS 1
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "Sim3Solver.h"          // ref_decls
#include "Optimizer.h"           // ref_decls

#define RUMI_SHELLS_NO_EIGEN_GEOMETRY 1
#include "../../rumi_slam_amd/facade/shells/Sim3Solver.cc"
#include "../../rumi_slam_amd/facade/PlaceRecognitionStages.h"

static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); fails++; } } while (0)

using ORB_SLAM3::KeyFrame;
using ORB_SLAM3::MapPoint;

struct Candidate {                                               // what BowStageResult hands to :655
    KeyFrame *pKFi = nullptr;
    std::vector<MapPoint *> vpMatchedPoints;
    std::vector<KeyFrame *> vpKeyFrameMatchedMP;
    int numBoWMatches = 0;
};

struct Scene {
    KeyFrame A;
    std::vector<std::unique_ptr<KeyFrame>> kfs;
    std::vector<std::unique_ptr<MapPoint>> pts;
    std::vector<Candidate> cand;
};

static void sigmas(KeyFrame &k) {
    k.mvLevelSigma2.assign(8, 1.f); k.mvInvLevelSigma2.assign(8, 1.f);
    for (int l = 1; l < 8; l++) { k.mvLevelSigma2[l] = k.mvLevelSigma2[l - 1] * 1.44f; k.mvInvLevelSigma2[l] = 1.f / k.mvLevelSigma2[l]; }
}

// NP points seen by A (feature i of A) and by candidate key-frame B under X_a = sc * X_b + t; every `outlierEvery`-th match is wrong
static void add_candidate(Scene &w, std::mt19937 &rng, int NP, float sc, int outlierEvery, int numBoW, bool covisible) {
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    std::unique_ptr<KeyFrame> B(new KeyFrame()), C(new KeyFrame());
    B->mnId = 10 + (long)w.cand.size(); C->mnId = 100 + (long)w.cand.size();
    B->pose = Sophus::SE3f(Eigen::Quaternionf(1, 0, 0, 0), Eigen::Vector3f(-0.2f + 0.05f * w.cand.size(), 0.1f, 0.f));
    C->pose = B->pose;
    sigmas(*B); sigmas(*C);
    Candidate c;
    c.pKFi = B.get(); c.numBoWMatches = numBoW;
    c.vpMatchedPoints.assign(w.A.N, nullptr);
    c.vpKeyFrameMatchedMP.assign(w.A.N, nullptr);
    for (int i = 0; i < NP; i++) {
        MapPoint *pa = w.A.mvpMapPoints[i];
        const Eigen::Vector3f Xa = w.A.pose * pa->pos;
        const Eigen::Vector3f Xb = (Xa - Eigen::Vector3f(0.3f, -0.1f, 0.2f)) * (1.f / sc);
        Eigen::Vector3f nb = Xb;
        if (i % outlierEvery == 0) nb = Xb + Eigen::Vector3f(0.6f * U(rng), 0.6f * U(rng), 0.6f * U(rng));
        std::unique_ptr<MapPoint> pb(new MapPoint());
        pb->pos = B->pose.inverse() * nb;
        cv::KeyPoint kb; kb.octave = (i + 1) % 4;
        kb.pt.x = B->cam.fx * nb(0) / nb(2) + B->cam.cx; kb.pt.y = B->cam.fy * nb(1) / nb(2) + B->cam.cy;
        B->mvKeysUn.push_back(kb); B->mvKeys.push_back(kb); B->mvpMapPoints.push_back(pb.get());
        pb->obs[B.get()] = std::make_tuple(i, -1);
        KeyFrame *found = B.get();
        if (covisible && i % 5 == 0) {                           // matched in the covisible: its own key-point, two octaves up
            cv::KeyPoint kc = kb; kc.octave = kb.octave + 2;
            pb->obs[C.get()] = std::make_tuple((int)C->mvKeysUn.size(), -1);
            C->mvKeysUn.push_back(kc); C->mvKeys.push_back(kc); C->mvpMapPoints.push_back(pb.get());
            found = C.get();
        }
        if (i % 11 != 0) { c.vpMatchedPoints[i] = pb.get(); c.vpKeyFrameMatchedMP[i] = found; }
        w.pts.push_back(std::move(pb));
    }
    B->N = (int)B->mvKeysUn.size(); C->N = (int)C->mvKeysUn.size();
    w.cand.push_back(c);
    w.kfs.push_back(std::move(B)); w.kfs.push_back(std::move(C));
}

static void build(Scene &w) {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    const int NA = 130;
    w.A.mnId = 1;
    w.A.pose = Sophus::SE3f(Eigen::Quaternionf(1, 0, 0, 0), Eigen::Vector3f(0.1f, 0.f, 0.2f));
    sigmas(w.A);
    for (int i = 0; i < NA; i++) {
        const Eigen::Vector3f Xa(2.f * U(rng), 1.5f * U(rng), 4.f + 2.f * U(rng));
        std::unique_ptr<MapPoint> pa(new MapPoint());
        pa->pos = w.A.pose.inverse() * Xa;
        cv::KeyPoint ka; ka.octave = i % 4;
        ka.pt.x = w.A.cam.fx * Xa(0) / Xa(2) + w.A.cam.cx; ka.pt.y = w.A.cam.fy * Xa(1) / Xa(2) + w.A.cam.cy;
        w.A.mvKeysUn.push_back(ka); w.A.mvKeys.push_back(ka); w.A.mvpMapPoints.push_back(pa.get());
        pa->obs[&w.A] = std::make_tuple(i, -1);
        w.pts.push_back(std::move(pa));
    }
    w.A.N = NA;
    add_candidate(w, rng, 120, 1.3f, 7, 90, true);
    add_candidate(w, rng, 60, 1.1f, 7, 10, false);
    add_candidate(w, rng, 40, 1.2f, 1, 30, false);
    add_candidate(w, rng, 70, 0.9f, 5, 55, true);
    add_candidate(w, rng, 12, 1.0f, 7, 25, false);
}

struct Ransac { bool conv = false; int nIn = 0; std::vector<bool> inl; float R[9], t[3], s = 0; };

int main() {
    Scene SA, SB;
    build(SA); build(SB);
    const int nBoWMatches = 20, nBoWInliers = 15;
    const bool bFixedScale = false;
    const size_t nC = SA.cand.size();

    // the first device call of a process creates the arena and loads the kernels; whatever the runtime draws from rand() while it does is not the
    // stage's: both sides start from a process that has made a call
    { std::vector<rumi_facade::Sim3RansacOutcome> warm; rumi_facade::Sim3RansacStage(&SA.A, SA.cand, bFixedScale, nBoWMatches, nBoWInliers, warm); }

    // ---- side A: the stage ----
    srand(1234);
    std::vector<rumi_facade::Sim3RansacOutcome> out;
    const int rounds = rumi_facade::Sim3RansacStage(&SA.A, SA.cand, bFixedScale, nBoWMatches, nBoWInliers, out, 250);
    const int nextA = rand();
    srand(1234);
    std::vector<rumi_facade::Sim3RansacOutcome> out20;
    const int rounds20 = rumi_facade::Sim3RansacStage(&SA.A, SA.cand, bFixedScale, nBoWMatches, nBoWInliers, out20, 20);
    const int nextA20 = rand();
    srand(1234);
    std::vector<rumi_facade::Sim3RansacOutcome> outD;                // the default: 20 for every solver still running (three, then two)
    const int roundsD = rumi_facade::Sim3RansacStage(&SA.A, SA.cand, bFixedScale, nBoWMatches, nBoWInliers, outD);
    const int nextAD = rand();
    CHECK(rounds == 1 && rounds20 == 4 && roundsD == 2, "one round at a window of 250, four at 20, two at the default");

    // ---- side B: :655-676 as written, over the shell ----
    srand(1234);
    std::vector<Ransac> ref(nC);
    std::vector<int> its(nC, 0);
    for (size_t k = 0; k < nC; k++) {
        Candidate &c = SB.cand[k];
        if (c.numBoWMatches >= nBoWMatches) {
            ORB_SLAM3::Sim3Solver solver = ORB_SLAM3::Sim3Solver(&SB.A, c.pKFi, c.vpMatchedPoints, bFixedScale, c.vpKeyFrameMatchedMP);
            solver.SetRansacParameters(0.99, nBoWInliers, 300);
            bool bNoMore = false; std::vector<bool> vbInliers; int nInliers; bool bConverge = false;
            Eigen::Matrix4f mTcm;
            while (!bConverge && !bNoMore) mTcm = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
            ref[k].conv = bConverge; ref[k].nIn = bConverge ? nInliers : 0; ref[k].inl = vbInliers;
            if (bConverge) {
                const Eigen::Matrix3f R = solver.GetEstimatedRotation(); const Eigen::Vector3f t = solver.GetEstimatedTranslation();
                for (int r = 0; r < 3; r++) { for (int cc = 0; cc < 3; cc++) ref[k].R[r * 3 + cc] = R(r, cc); ref[k].t[r] = t(r); }
                ref[k].s = solver.GetEstimatedScale();
            }
        }
    }
    const int nextB = rand();
    CHECK(nextA == nextB, "rand() stands where the per-candidate loops leave it");
    CHECK(nextA20 == nextB, "rand() stands where the per-candidate loops leave it, in rounds of 20");
    CHECK(nextAD == nextB, "rand() stands where the per-candidate loops leave it, at the default window");
    for (size_t k = 0; k < nC; k++) {
        for (const auto *o : {&out[k], &out20[k], &outD[k]}) {
            CHECK(o->reached == (SA.cand[k].numBoWMatches >= nBoWMatches), "reached");
            CHECK(o->bConverge == ref[k].conv && o->nInliers == ref[k].nIn, "bConverge / nInliers");
            if (ref[k].conv) {
                CHECK(o->vbInliers == ref[k].inl, "vbInliers");
                CHECK(!std::memcmp(o->R, ref[k].R, 36) && !std::memcmp(o->t, ref[k].t, 12) && !std::memcmp(&o->s, &ref[k].s, 4), "estimated R, t, s: bytes");
            }
        }
        std::printf("candidate %zu: reached %d converged %d inliers %d iterations %d\n", k, (int)out[k].reached, (int)out[k].bConverge, out[k].nInliers, out[k].iterations);
    }
    CHECK(out[0].bConverge && !out[1].reached && out[2].reached && !out[2].bConverge && out[2].iterations > 20 && out[3].bConverge && out[4].reached && !out[4].bConverge &&
              out[4].iterations == 0, "the five candidates end as constructed");

    // ---- :728 for the converged candidates: one call against one call each ----
    using Job = rumi_facade::OptimizeSim3Job<KeyFrame, MapPoint, g2o::Sim3>;
    std::vector<Job> jobs;
    std::vector<std::vector<MapPoint *>> mA(nC), mB(nC);
    std::vector<g2o::Sim3> gA(nC), gB(nC);
    std::vector<int> nA(nC, -7), nB(nC, -7);
    for (size_t k = 0; k < nC; k++) {
        if (!ref[k].conv) continue;
        Eigen::Matrix3f R; Eigen::Vector3f t;
        for (int r = 0; r < 3; r++) { for (int cc = 0; cc < 3; cc++) R(r, cc) = ref[k].R[r * 3 + cc]; t(r) = ref[k].t[r]; }
        gA[k] = gB[k] = g2o::Sim3(R.cast<double>(), t.cast<double>(), (double)ref[k].s);      // gScm, :706
        mA[k] = SA.cand[k].vpMatchedPoints; mB[k] = SB.cand[k].vpMatchedPoints;
        jobs.push_back(Job{&SA.A, SA.cand[k].pKFi, &mA[k], &gA[k], 10.f, k == 3, true, &nA[k]});
    }
    CHECK(rumi_facade::OptimizeSim3Stage(jobs) == (int)jobs.size() && jobs.size() == 2, "OptimizeSim3Stage ran both jobs");
    for (size_t k = 0; k < nC; k++) {
        if (!ref[k].conv) continue;
        Eigen::Matrix77d mHessian7x7;
        nB[k] = rumi_facade_impl::Optimizer::OptimizeSim3(&SB.A, SB.cand[k].pKFi, mB[k], gB[k], 10.f, k == 3, mHessian7x7, true);
        double a[8], b[8];
        rumi_facade_impl::Optimizer::sim3_to8(gA[k], a); rumi_facade_impl::Optimizer::sim3_to8(gB[k], b);
        CHECK(nA[k] == nB[k] && nA[k] >= 20, "numOptMatches");
        CHECK(!std::memcmp(a, b, sizeof a), "g2oS12: bytes");
        bool same = mA[k].size() == mB[k].size();
        int kept = 0, dropped = 0;
        for (size_t i = 0; same && i < mA[k].size(); i++) {
            same = (mA[k][i] == nullptr) == (mB[k][i] == nullptr);
            kept += mA[k][i] != nullptr; dropped += !mA[k][i] && SA.cand[k].vpMatchedPoints[i];
        }
        CHECK(same && dropped > 0, "vpMatches1: the same matches removed");
        std::printf("candidate %zu: OptimizeSim3 %d / %d, %d matches kept, %d removed\n", k, nA[k], nB[k], kept, dropped);
    }
    std::printf("place recognition stages: %d failure(s); rounds %d / %d, next rand %d / %d / %d\n", fails, rounds, rounds20, nextA, nextA20, nextB);
    return fails ? 1 : 0;
}
