// The two stages of DetectCommonRegionsFromBoW (R/lib_src/LoopClosing.cc:542-853; CloudMerging.cc:1019 ff. is the same text) that sit between the
// batched searches of LoopClosingStep.h, for EVERY candidate in one device call each:
//   Sim3RansacStage    :655-676   Sim3Solver(mpCurrentKF, pMostBoWMatchesKF, vpMatchedPoints, bFixedScale, vpKeyFrameMatchedMP), SetRansacParameters(0.99,
//                                 nBoWInliers, 300) and `while (!bConverge && !bNoMore) iterate(20, ...)` per candidate -> rumi_sim3_ransac_batch in rounds
//   OptimizeSim3Stage  :728       Optimizer::OptimizeSim3 per candidate that passed :719 -> one rumi_optimize_sim3_batch call
// (include/rumi_opt.h).  The solvers of the reference share the process-wide rand(): the stage draws every solver's view of a window of
// the stream on a copy of the generator (RandLookahead.h), the device applies the sequential rule, and rand() is moved by three draws per iteration
// the reference's loops would have run -- the candidates' results and the next rand() are those of the per-candidate text.
// The per-candidate path (shells/Sim3Solver.cc, Optimizer::OptimizeSim3) remains valid and gives the same bytes.
// Templated on the data model as the other facade members.  Needs RUMI_HAVE_SOPHUS (Optimizer.h's Sim3 section).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <tuple>
#include <vector>

#include "Optimizer.h"
#include "RandLookahead.h"
#include "Sim3SolverGather.h"
#include "rumi_opt.h"
#include "rumi_status.h"

namespace rumi_facade {

// mRansacMaxIts of SetRansacParameters(probability, minInliers, maxIterations) for N correspondences (:134-157)
inline int sim3_ransac_max_its(double probability, int minInliers, int maxIterations, int N) {
    const float epsilon = (float)minInliers / N;
    int nIterations;
    if (minInliers == N) nIterations = 1;
    else nIterations = (int)std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
    return std::max(1, std::min(nIterations, maxIterations));
}

// Per candidate, what :676-709 read of its solver.
struct Sim3RansacOutcome {
    bool reached = false;                                        // numBoWMatches >= nBoWMatches: a solver was built (:655)
    bool bConverge = false;
    int nInliers = 0, iterations = 0;                            // mnIterations of the solver when its loop ended
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1.f;   // GetEstimatedRotation (row-major) / Translation / Scale of a converged solver
    std::vector<bool> vbInliers;                                 // over vpMatchedPoints (mN1)
};

// :655-676 for every entry of `results` (BowStageResult of LoopClosingStep.h, or anything with pKFi, vpMatchedPoints, vpKeyFrameMatchedMP and
// numBoWMatches), in order.  window: iterations of the shared stream a round evaluates; 0 = 20 for every solver still running, the reference's
// block (DESIGN.md 4x has the device-entry times of other windows).  Returns the rounds used, or -1 with a report: a failed device call; rand() then stands where the rounds
// completed so far left it, and the outcomes not yet decided stay unconverged.
template <class KeyFrameT, class ResultT>
int Sim3RansacStage(KeyFrameT *pCurrentKF, const std::vector<ResultT> &results, bool bFixedScale, int nBoWMatches, int nBoWInliers, std::vector<Sim3RansacOutcome> &out,
                    int window = 0) {
    struct Solver { size_t cand; Sim3Correspondences c; int maxIts, its; float K1[4], K2[4]; };
    out.assign(results.size(), Sim3RansacOutcome());
    std::vector<Solver> solvers;
    for (size_t k = 0; k < results.size(); k++) {
        const ResultT &r = results[k];
        if (r.numBoWMatches < nBoWMatches) continue;
        out[k].reached = true;
        Solver s;
        s.cand = k; s.its = 0;
        sim3_solver_gather(pCurrentKF, r.pKFi, r.vpMatchedPoints, r.vpKeyFrameMatchedMP, s.c);
        out[k].vbInliers.assign((size_t)s.c.mN1, false);
        if (s.c.N() < nBoWInliers) continue;                     // :228-231: bNoMore at once, nothing drawn
        s.maxIts = sim3_ransac_max_its(0.99, nBoWInliers, 300, s.c.N());
        for (int i = 0; i < 4; i++) { s.K1[i] = pCurrentKF->mpCamera->getParameter(i); s.K2[i] = r.pKFi->mpCamera->getParameter(i); }
        solvers.push_back(std::move(s));
    }
    int rounds = 0;
    std::vector<size_t> pending(solvers.size());
    for (size_t i = 0; i < pending.size(); i++) pending[i] = i;
    while (!pending.empty()) {
        const size_t J = pending.size();
        const int R = window > 0 ? window : 20 * (int)J;
        std::vector<RumiSim3RansacSolver> rec(J);
        std::vector<float> X1, X2, s1, s2;
        std::vector<int32_t> tri(J * (size_t)R * 3);
        for (size_t j = 0; j < J; j++) {
            const Solver &s = solvers[pending[j]];
            const int N = s.c.N();
            rec[j].first = (int32_t)s1.size(); rec[j].n = N; rec[j].min_inliers = nBoWInliers; rec[j].its_left = s.maxIts - s.its; rec[j].fix_scale = bFixedScale ? 1 : 0;
            std::memcpy(rec[j].K4_1, s.K1, 16); std::memcpy(rec[j].K4_2, s.K2, 16);
            X1.insert(X1.end(), s.c.X1.begin(), s.c.X1.end()); X2.insert(X2.end(), s.c.X2.begin(), s.c.X2.end());
            s1.insert(s1.end(), s.c.sigma2_1.begin(), s.c.sigma2_1.end()); s2.insert(s2.end(), s.c.sigma2_2.begin(), s.c.sigma2_2.end());
            RandLookahead ahead;                                 // every solver reads the same window of the stream with its own N (:249-259)
            std::vector<int32_t> avail((size_t)N);
            for (int h = 0; h < R; h++) {
                for (int i = 0; i < N; i++) avail[i] = i;
                int left = N;
                for (int i = 0; i < 3; i++) {
                    const int randi = ahead.RandomInt(0, left - 1);
                    tri[(j * (size_t)R + h) * 3 + i] = avail[randi];
                    avail[randi] = avail[left - 1];
                    left--;
                }
            }
        }
        std::vector<RumiSim3RansacResult> res(J);
        std::vector<uint8_t> inl(s1.size() + 1);
        if (!RUMI_FACADE_NAMESPACE::Optimizer::arena()) return -1;                                   // reported by arena()
        if (RUMI_GUARDED("Sim3RansacStage / rumi_sim3_ransac_batch", &RUMI_FACADE_NAMESPACE::Optimizer::grow_arena,
                         rumi_sim3_ransac_batch(RUMI_FACADE_NAMESPACE::Optimizer::arena(), (int32_t)J, rec.data(), (int32_t)s1.size(), X1.data(), X2.data(), s1.data(), s2.data(),
                                                R, tri.data(), res.data(), inl.data(), nullptr, nullptr)) != RUMI_OK)
            return -1;
        rounds++;
        int consumed = 0;
        std::vector<size_t> still;
        for (size_t j = 0; j < J; j++) {
            Solver &s = solvers[pending[j]];
            Sim3RansacOutcome &o = out[s.cand];
            s.its += res[j].its; consumed += res[j].its;
            o.iterations = s.its;
            if (res[j].state == RUMI_SIM3_CONVERGED) {
                o.bConverge = true; o.nInliers = res[j].n_inliers;
                std::memcpy(o.R, res[j].T12, 36); std::memcpy(o.t, res[j].T12 + 9, 12); o.s = res[j].T12[12];
                for (int i = 0; i < s.c.N(); i++) if (inl[(size_t)rec[j].first + i]) o.vbInliers[s.c.indices1[i]] = true;
            } else if (res[j].state != RUMI_SIM3_EXHAUSTED) still.push_back(pending[j]);
        }
        rand_advance(consumed);
        pending = still;
    }
    return rounds;
}

// One call of Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) (Optimizer.cc:1920-2167).
template <class KeyFrameT, class MapPointT, class Sim3T> struct OptimizeSim3Job {
    KeyFrameT *pKF1, *pKF2;
    std::vector<MapPointT *> *vpMatches1;
    Sim3T *g2oS12;
    float th2;
    bool bFixScale, bAllPoints;
    int *numOptMatches;                                          // the member's return value
};

// :728 for every candidate that passed :719, in one device call; matches, estimates and return values as Optimizer::OptimizeSim3 (Optimizer.h)
// leaves them.  mAcumHessian is zeroed by the reference and never accumulated: the caller zeroes its own.  Returns the number of jobs, or -1
// with a report and nothing written: a failed device call.
template <class KeyFrameT, class MapPointT, class Sim3T>
int OptimizeSim3Stage(const std::vector<OptimizeSim3Job<KeyFrameT, MapPointT, Sim3T>> &jobs) {
    using Opt = RUMI_FACADE_NAMESPACE::Optimizer;
    if (jobs.empty()) return 0;
    const size_t J = jobs.size();
    std::vector<Opt::Sim3Gather> g(J);
    std::vector<RumiSim3OptProblem> rec(J);
    std::vector<float> P1c, P2c, obs1, obs2, w1, w2;
    std::vector<double> S(J * 8);
    for (size_t j = 0; j < J; j++) {
        const auto &job = jobs[j];
        const int N = (int)job.vpMatches1->size();
        const auto vpMapPoints1 = job.pKF1->GetMapPointMatches();
        for (int i = 0; i < N; i++) {
            if (!(*job.vpMatches1)[i]) continue;
            Opt::sim3_gather(g[j], job.pKF1, job.pKF2, vpMapPoints1[i], (*job.vpMatches1)[i], (size_t)i, 0, job.bAllPoints);
        }
        rec[j].first = (int32_t)w1.size(); rec[j].n = g[j].n(); rec[j].th2 = job.th2; rec[j].fix_scale = job.bFixScale ? 1 : 0; rec[j].robust_first_pass = 1;
        const float K1[4] = {job.pKF1->fx, job.pKF1->fy, job.pKF1->cx, job.pKF1->cy}, K2[4] = {job.pKF2->fx, job.pKF2->fy, job.pKF2->cx, job.pKF2->cy};
        std::memcpy(rec[j].K4_1, K1, 16); std::memcpy(rec[j].K4_2, K2, 16);
        P1c.insert(P1c.end(), g[j].P1c.begin(), g[j].P1c.end()); P2c.insert(P2c.end(), g[j].P2c.begin(), g[j].P2c.end());
        obs1.insert(obs1.end(), g[j].obs1.begin(), g[j].obs1.end()); obs2.insert(obs2.end(), g[j].obs2.begin(), g[j].obs2.end());
        w1.insert(w1.end(), g[j].w1.begin(), g[j].w1.end()); w2.insert(w2.end(), g[j].w2.begin(), g[j].w2.end());
        Opt::sim3_to8(*job.g2oS12, &S[j * 8]);
    }
    const int32_t total = (int32_t)w1.size();
    std::vector<uint8_t> status((size_t)total + 1);
    std::vector<int32_t> res(J * 3, 0);
    P1c.resize(P1c.size() + 3); P2c.resize(P2c.size() + 3); obs1.resize(obs1.size() + 2); obs2.resize(obs2.size() + 2); w1.push_back(0); w2.push_back(0);   // (never an empty array)
    if (!Opt::arena()) return -1;                                                                    // reported by arena()
    if (RUMI_GUARDED("OptimizeSim3Stage / rumi_optimize_sim3_batch", &Opt::grow_arena,
                     rumi_optimize_sim3_batch(Opt::arena(), (int32_t)J, rec.data(), total, P1c.data(), P2c.data(), obs1.data(), obs2.data(), w1.data(), w2.data(), S.data(),
                                              status.data(), res.data())) != RUMI_OK)
        return -1;
    for (size_t j = 0; j < J; j++) {
        const auto &job = jobs[j];
        const int32_t *r3 = &res[j * 3];
        const uint8_t *st = status.data() + rec[j].first;
        for (int k = 0; k < g[j].n(); k++)
            if (st[k] == 1 || (!r3[2] && st[k] == 2)) (*job.vpMatches1)[g[j].index[k]] = static_cast<MapPointT *>(nullptr);   // :2112, :2156
        if (r3[2]) { if (job.numOptMatches) *job.numOptMatches = 0; continue; }                      // :2135-2136: g2oS12 keeps its value
        *job.g2oS12 = Opt::template sim3_from8<Sim3T>(&S[j * 8]);                                    // :2163-2164
        if (job.numOptMatches) *job.numOptMatches = r3[0];
    }
    return (int)J;
}

}  // namespace rumi_facade
