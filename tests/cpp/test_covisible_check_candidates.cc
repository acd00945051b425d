// LoopClosingStep::CovisibleCheckResident over SEVERAL candidates (facade/LoopClosingStep.h: every (candidate, covisible) search of the loop
// LoopClosing.cc:773-795 in one device call) against one call of the single-candidate member per candidate -- which
// tests/cpp/test_sim3_projection_facade.cc holds against the reference's text -- on the GPU.  Reads a map written by
// tests/test_covisible_check_candidates_gpu.py (the file format of tests/test_sim3_projection_facade_gpu.py).  Candidate c has its own matched
// key-frame and its own gScw; the last candidate arrives with nNumKFs = 3 already, so its loop visits nothing and its vpMapPoints must stay.  Prints
//   C side c visited nNumKFs | vpMapPoints ids         side A: the overload, side B: one call per candidate
//   R A ret status untouched|TOUCHED                   a refused call
#define RUMI_HAVE_SOPHUS 1
#include <climits>
#include <cstdio>
#include <set>
#include <vector>

#include "mock_sophus.h"

#include "CovisibilityGraph.h"
#include "LoopClosingStep.h"

#include "sim3_projection_world.h"

static g2o::Sim3 gscw_of(const World &w, int c) {                  // the Sim3 estimate of candidate c: the current key-frame's, nudged
    const float *a = w.sim3;
    return g2o::Sim3(Eigen::Quaterniond(a[3], a[0], a[1], a[2]), Eigen::Vector3d(a[4] + 0.01 * c, a[5] - 0.005 * c, a[6]), (double)a[7]);
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_covisible_check_candidates map.bin\n"); return 2; }
    int32_t h[8];
    World A;
    if (!load(argv[1], h, A)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    using Graph = CovisibilityGraph<KeyFrameSN, MapPointSN>;
    Graph graph(h[0] + 4, h[1] + 64);
    if (!graph.ok()) return 3;
    for (int k = 0; k < h[0]; k++)
        if (k != h[3] && (graph.Sync(A.kfs[k].get()) != RUMI_OK || graph.SyncFeatures(A.kfs[k].get()) != RUMI_OK)) return 3;
    std::vector<MapPointSN *> all;
    for (int i = 0; i < h[1]; i++) {
        if (graph.Sync(A.mps[i].get()) != RUMI_OK) return 3;
        all.push_back(A.mps[i].get());
    }
    if (graph.SyncAttributes(all) != RUMI_OK) return 3;

    rumi::LoopClosingStep step;
    std::vector<KeyFrameSN *> matched = A.cand;                     // one more: the first matched key-frame again, arriving with nNumKFs = 3
    matched.push_back(A.cand[0]);
    const size_t nK = matched.size();
    const std::vector<KeyFrameSN *> cov = A.cur->GetBestCovisibilityKeyFrames(10);
    const std::vector<MapPointSN *> marker(3, A.mps[0].get());

    using Cand = rumi::LoopClosingStep::CovisibleCheckCandidate<KeyFrameSN, MapPointSN, g2o::Sim3>;
    std::vector<std::vector<MapPointSN *>> ptsA(nK, marker), ptsB(nK, marker);
    std::vector<int> nA(nK, 0), nB(nK, 0);
    nA[nK - 1] = nB[nK - 1] = 3;
    std::vector<Cand> cands;
    for (size_t c = 0; c < nK; c++) cands.push_back(Cand{matched[c], gscw_of(A, (int)c), &ptsA[c], &nA[c], -7});
    rumi_facade::clear_status();
    const int ret = step.CovisibleCheckResident(graph, A.cur, cands, cov, toSophusMock);
    if (ret < 0) {
        bool same = true;
        for (size_t c = 0; c < nK; c++) same = same && ptsA[c] == marker && nA[c] == (c == nK - 1 ? 3 : 0) && cands[c].visited == -7;
        std::printf("R A %d %d %s\n", ret, rumi_facade::last_status(), same ? "untouched" : "TOUCHED");
        return 0;
    }
    for (size_t c = 0; c < nK; c++) {
        std::printf("C A %zu %d %d |", c, cands[c].visited, nA[c]);
        for (MapPointSN *p : ptsA[c]) std::printf(" %d", p ? A.pi[p] : -1);
        std::printf("\n");
    }
    for (size_t c = 0; c < nK; c++) {
        const int visited = step.CovisibleCheckResident(graph, A.cur, matched[c], gscw_of(A, (int)c), cov, ptsB[c], &nB[c], toSophusMock);
        std::printf("C B %zu %d %d |", c, visited, nB[c]);
        for (MapPointSN *p : ptsB[c]) std::printf(" %d", p ? A.pi[p] : -1);
        std::printf("\n");
    }
    std::printf("J %d %zu\n", ret, cov.size());
    return 0;
}
